"""The rollout's forward mode in the initial state with the Gauss-Newton normal equations of the fit of x0 on the GPU
(cpmpc_sim_rollout_gn_x0_batch; sim_rollout_gauss_newton_x0, sim_estimate_state, WindowEstimator) against the parent's one-tick
calls, against the rollout's adjoint, and against the numpy reference of tests/helpers/sim_rollout_gn_x0_ref.py, which
tests/test_sim_rollout_gn_x0_ref.py pins.

Shapes: the grid of tests/test_gpu_sim_rollout_gn.py.  B = 130 -- two full waves and a 2-lane tail -- and B = 1; (dt, T) =
(0.0105, 5), (0.02, 3), (0.001, 8), (0, 3): 11 / 20 / 1 / 0 sub-steps a tick; both models, both dtypes; the states of
sim_jac_ref.states; shared forces, [4, B] forces, per-problem parameters DYN (1 +- 20 %), "w", positions-only state weights, and
"tw", random per-sample weights in [0, 2].  The recording x_obs is the parent's sim_rollout_states trajectory plus uniform +-0.1.

1. Against the float64 recurrence Phi_{t+1} = A_t Phi_t on the parent's sim_step_jacobian A_t at the parent's checkpoints,
   elementwise.  Phi_final within f Pabs, f = 4 (NX + 1) T max(n_sub, 1) eps and Pabs the recurrence on absolute values (the bound
   of sections 5g / 5h).  H, g, cost within the first-order propagation of that through their sums, with c = 4 NX T eps for the
   sums themselves and dx = 4 T max(n_sub, 1) eps max(1, |x|) for the kernel's own states against the parent's:
       H:    (2 f + c) sum om Pabs^T W Pabs
       g:    (f + c) sum om Pabs^T W |r|  +  sum om Pabs^T W dx
       cost: c 1/2 sum om |r|^T W |r|    +  sum om |r|^T W dx
2. Forward against reverse: g equals sim_rollout_vjp(gbar[t] = -om_t W r_t)["x"] within g's bound of 1.
3. T = 1: Phi_final against sim_step_jacobian's A and x_final against its x_new within 1's bound, and bitwise.
4. fp64 against the oracle's reference: x_final within T 1e-12, Phi_final, g, H within T 1e-7 of the lane's largest reference entry.
5. fp32: per lane the distance of each output from the fp64 kernel's at the same float-rounded inputs, relative to the lane's
   largest entry; median and 99th percentile at most 4 x those of the parent's float chain (per tick sim_step_jacobian, then
   Phi <- A Phi, the residual and the sums in float torch).
6. bitwise and structural properties.  7. estimation (sim_estimate_state), fp64.  8. WindowEstimator.
Every test prints its figures before it asserts; DESIGN.md section 5j is where they are recorded."""
import numpy as np
import pytest

from helpers import sim_jac_ref as sj
from helpers import sim_rollout_gn_x0_ref as gx

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = 130
DT_T = ((0.0105, 5), (0.02, 3), (0.001, 8), (0.0, 3))
# (model, dt, T, kind): kind None, "shared" forces, "per"-problem forces, "dyn" per-problem parameters, "w" positions-only
# state weights, "tw" per-sample weights
CASES = [(m, dt, nt, None) for m in ("single", "double") for dt, nt in DT_T] + \
        [("single", 0.0105, 5, "shared"), ("single", 0.0105, 5, "per"), ("single", 0.0105, 5, "dyn"), ("double", 0.0105, 5, "dyn"),
         ("single", 0.0105, 5, "w"), ("double", 0.0105, 5, "tw")]
IDS = ["%s-%g-%d-%s" % c for c in CASES]
DTYPES = [torch.float64, torch.float32]
SHARED_F = ((1.5, 0.0), (-2.0, 1.0))
OUTS = ("cost", "g", "H", "Phi_final", "x_final")
TRIV = {"single": (), "double": (0, 3)}   # the columns of the step Jacobian that the dynamics never read


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1
    assert callable(pkg.sim_rollout_gauss_newton_x0)   # imports the batch module; fails on a tree without the call


def Tn(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _eps(dtype):
    return float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)


_IN = {}


def inputs(case, nb=B):
    """numpy inputs of a case, made once and left unchanged: x0 [nx, nb], us [T, nb], the recording's noise [T, nx, nb], forces
    (None, 4 shared numbers or [4, nb]), parameters (np numbers or [np, nb]), state weights (None or nx numbers) and per-sample
    weights (None or [T, nb])."""
    key = (case, nb)
    if key not in _IN:
        model, dt, nt, kind = case
        nx = sj.NX[model]
        x, _ = sj.states(model, nb)
        rng = np.random.default_rng(41)
        us = rng.uniform(-20.0, 20.0, (nt, nb))
        noise = rng.uniform(-0.1, 0.1, (nt, nx, nb))
        f = None
        if kind == "shared":
            f = np.array([SHARED_F[0][0], SHARED_F[0][1], SHARED_F[1][0], SHARED_F[1][1]])
        elif kind == "per":
            f = np.random.default_rng(21).uniform(-3.0, 3.0, (4, nb))
        prm = np.array(sj.DYN[model])
        if kind == "dyn":
            prm = np.tile(prm[:, None], (1, nb)) * np.random.default_rng(43).uniform(0.8, 1.2, (len(prm), nb))
        w = np.array([1.0] * (nx // 2) + [0.0] * (nx // 2)) if kind == "w" else None
        om = np.random.default_rng(45).uniform(0.0, 2.0, (nt, nb)) if kind == "tw" else None
        _IN[key] = (x, us, noise, f, prm, w, om)
        for a in _IN[key]:
            if a is not None:
                a.setflags(write=False)
    return _IN[key]


def tensors(pkg, case, dtype, nb=B):
    """-> x0, u, x_obs (the parent's trajectory in `dtype` plus the noise), xs (that trajectory), params (list or tensor), the
    keywords every package call of the case takes and those of the new call alone"""
    x, us, noise, f, prm, w, om = inputs(case, nb)
    kw = dict(model=case[0])
    if case[3] == "shared":
        kw.update(f_base=SHARED_F[0], f_mass=SHARED_F[1])
    elif case[3] == "per":
        kw.update(fext=Tn(f, dtype))
    params = Tn(prm, dtype) if prm.ndim == 2 else [float(v) for v in prm]
    x0, u = Tn(x, dtype), Tn(us, dtype)
    xs = pkg.sim_rollout_states(params, case[1], x0, u, **kw)["xs"]
    x_obs = (xs + Tn(noise, dtype)).contiguous()
    gkw = dict(kw)
    if w is not None:
        gkw["weights"] = [float(v) for v in w]
    if om is not None:
        gkw["tick_weights"] = Tn(om, dtype)
    return x0, u, x_obs, xs, params, kw, gkw


def tick_matrices(pkg, case, x0, u, xs, params, kw, as_numpy=True):
    """A [T, nx, nx, B] from the parent's one-tick calls at the checkpoints x_t = x0, xs[0], ..: sim_step_jacobian; with a
    parameter tensor, which that call does not take, sim_step_param_vjp on the unit cotangents (row r of A per call), as
    tests/test_gpu_sim_rollout.py does."""
    model, dt, nt, _ = case
    nx = sj.NX[model]
    A = []
    for t in range(nt):
        xt = x0 if t == 0 else xs[t - 1].contiguous()
        ut = u[t].contiguous()
        if isinstance(params, torch.Tensor):
            rows = []
            for r in range(nx):
                e = torch.zeros_like(xt)
                e[r] = 1.0
                rows.append(pkg.sim_step_param_vjp(params, dt, xt, ut, e, want="x", **kw)["x"])
            A.append(torch.stack(rows))
        else:
            A.append(pkg.sim_step_jacobian(params, dt, xt, ut, want="A", **kw)["A"])
    A = torch.stack(A)
    return N_(A) if as_numpy else A


def wrapped_residuals(model, x_obs, xs):
    """x_obs - xs with the pole angles' differences wrapped, numpy [T, nx, B]"""
    r = x_obs - xs
    nq = sj.NX[model] // 2
    r[:, 1:nq] -= 2 * np.pi * np.round(r[:, 1:nq] / (2 * np.pi))
    return r


_REF = {}


def ref_and_bound(pkg, case, dtype, nb=B):
    """the float64 recurrence and sums on the parent's per-tick matrices, and the elementwise bounds of test 1 -> two dicts
    with Phi_final, H, g, cost; computed once per (case, dtype)"""
    key = (case, dtype, nb)
    if key not in _REF:
        model, dt, nt, _ = case
        nx = sj.NX[model]
        x0, u, x_obs, xs, params, kw, _ = tensors(pkg, case, dtype, nb)
        _, _, _, _, _, w, om = inputs(case, nb)
        w = np.ones(nx) if w is None else w
        om = np.ones((nt, nb)) if om is None else N_(Tn(om, dtype))
        A = tick_matrices(pkg, case, x0, u, xs, params, kw)
        P, Pabs = gx.transitions(A), gx.transitions(np.abs(A))
        r = wrapped_residuals(model, N_(x_obs), N_(xs))
        cost, g, H = gx.normal_equations(P, r, w, om)
        n_sub, eps = max(len(sj.sub_steps(dt)), 1), _eps(dtype)
        f, c = 4 * (nx + 1) * nt * n_sub * eps, 4 * nx * nt * eps
        dx = 4 * nt * n_sub * eps * np.maximum(1.0, np.abs(N_(xs)))
        ra = np.abs(r)
        b_H = (2 * f + c) * np.einsum("tb,tqjb,q,tqkb->jkb", om, Pabs, w, Pabs)
        b_g = (f + c) * np.einsum("tb,tqjb,q,tqb->jb", om, Pabs, w, ra) + np.einsum("tb,tqjb,q,tqb->jb", om, Pabs, w, dx)
        b_c = c * 0.5 * np.einsum("tb,q,tqb,tqb->b", om, w, ra, ra) + np.einsum("tb,q,tqb,tqb->b", om, w, ra, dx)
        _REF[key] = (dict(Phi_final=P[-1], H=H, g=g, cost=cost), dict(Phi_final=f * Pabs[-1], H=b_H, g=b_g, cost=b_c))
    return _REF[key]


def worst_ratio(got, ref, bound):
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0))))


def lane_dist(got, ref):
    """per lane: max |got - ref| relative to the lane's max |ref|; a lane whose reference is all zero must be all zero"""
    ax = tuple(range(ref.ndim - 1))
    d, s = (np.abs(got - ref).max(axis=ax), np.abs(ref).max(axis=ax)) if ax else (np.abs(got - ref), np.abs(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))


def call(pkg, case, dtype, want=OUTS, nb=B):
    x0, u, x_obs, _, params, _, gkw = tensors(pkg, case, dtype, nb)
    return pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=want, **gkw)


# ---- 1. against the parent's one-tick calls -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_outputs_are_the_recurrence_on_the_parents_tick_matrices(pkg, case, dtype):
    got = call(pkg, case, dtype)
    ref, bound = ref_and_bound(pkg, case, dtype)
    ratios = {name: worst_ratio(N_(got[name]), ref[name], bound[name]) for name in ("Phi_final", "H", "g", "cost")}
    print("gn_x0 %s %s: worst |out - ref| / bound: %s" % (IDS[CASES.index(case)], dtype,
                                                           "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert all(torch.isfinite(got[name]).all() for name in OUTS)
    assert max(ratios.values()) <= 1.0
    assert (N_(got["H"]) != 0).any()


# ---- 2. forward against reverse -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_g_is_the_adjoints_state_gradient(pkg, case, dtype):
    model, dt, nt, _ = case
    x0, u, x_obs, xs, params, kw, gkw = tensors(pkg, case, dtype)
    nq = sj.NX[model] // 2
    r = x_obs - xs
    r[:, 1:nq] = r[:, 1:nq] - 2 * np.pi * torch.round(r[:, 1:nq] / (2 * np.pi))
    w = torch.tensor(gkw.get("weights", [1.0] * sj.NX[model]), dtype=dtype, device=DEV)
    om = gkw.get("tick_weights", torch.ones((nt, B), dtype=dtype, device=DEV))
    gbar = (-(om[:, None, :] * (w[None, :, None] * r))).contiguous()
    rev = pkg.sim_rollout_vjp(params, dt, x0, u, xs, gbar=gbar, want="x", **kw)["x"]
    fwd = call(pkg, case, dtype, want="g")["g"]
    _, bound = ref_and_bound(pkg, case, dtype)
    ratio = worst_ratio(N_(fwd), N_(rev), bound["g"])
    print("gn_x0 %s %s: forward g against the adjoint's g_x0, worst |difference| / bound %.3f" % (IDS[CASES.index(case)], dtype,
                                                                                                   ratio))
    assert ratio <= 1.0


# ---- 3. one tick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model,dt,kind", [("single", 0.0105, None), ("double", 0.0105, None), ("single", 0.02, None),
                                           ("double", 0.001, None), ("single", 0.0105, "per"), ("single", 0.0105, "shared")])
def test_one_tick_is_the_parents_step_jacobian(pkg, model, dt, kind, dtype):
    case = (model, dt, 1, kind)
    x0, u, _, _, params, kw, _ = tensors(pkg, case, dtype)
    got = pkg.sim_rollout_gauss_newton_x0(params, dt, x0, u, None, want=("Phi_final", "x_final"), **kw)
    one = pkg.sim_step_jacobian(params, dt, x0, u[0].contiguous(), want=("x_new", "A"), **kw)
    _, bound = ref_and_bound(pkg, case, dtype)
    ratio = worst_ratio(N_(got["Phi_final"]), N_(one["A"]), bound["Phi_final"])
    n_sub, eps = max(len(sj.sub_steps(dt)), 1), _eps(dtype)
    dx = (N_(got["x_final"]) - N_(one["x_new"])) / (4 * n_sub * eps * np.maximum(1.0, np.abs(N_(one["x_new"]))))
    print("T = 1 %s dt=%g %s %s: |Phi_final - A| / bound %.3f, |x_final - x_new| / bound %.3f, bitwise Phi_final: %s, bitwise "
          "x_final: %s" % (model, dt, kind, dtype, ratio, np.abs(dx).max(), torch.equal(got["Phi_final"], one["A"]),
                           torch.equal(got["x_final"], one["x_new"])))
    assert ratio <= 1.0 and np.abs(dx).max() <= 1.0
    # the same text (rk4_step_jac_m, step_jac_apply) in both kernels: bitwise in every case measured, and held to it
    assert torch.equal(got["Phi_final"], one["A"]) and torch.equal(got["x_final"], one["x_new"])


# ---- 4. fp64 against the oracle's reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp64_matches_the_oracles_reference(pkg, orc, case):
    model, dt, nt, _ = case
    x, us, _, f, prm, w, om = inputs(case)
    _, _, x_obs, _, _, _, _ = tensors(pkg, case, torch.float64)
    xs_ref, P_ref = gx.oracle_route_batch(orc, model, prm, dt, x, us, fext=f)
    _, g_ref, H_ref = gx.normal_equations(P_ref, gx.gn.residuals(orc, model, N_(x_obs), xs_ref), w, om)
    got = call(pkg, case, torch.float64)
    ex = np.abs(N_(got["x_final"]) - xs_ref[-1]).max()
    errs = [lane_dist(N_(got[n]), r).max() for n, r in (("Phi_final", P_ref[-1]), ("g", g_ref), ("H", H_ref))]
    print("fp64 %s against the oracle: |x_final - ref| %.2e (bound %.0e)  Phi_final %.2e  g %.2e  H %.2e of the lane's max "
          "(bound %.0e)" % (IDS[CASES.index(case)], ex, nt * 1e-12, *errs, nt * 1e-7))
    assert ex <= nt * 1e-12
    assert max(errs) <= nt * 1e-7


# ---- 5. fp32 against the parent's float chain ---------------------------------------------------------------------------
def _float_chain(pkg, case):
    """the recurrence and the sums in float torch on the float one-tick calls at the float trajectory's checkpoints"""
    model, dt, nt, _ = case
    x0, u, x_obs, xs, params, kw, gkw = tensors(pkg, case, torch.float32)
    A = tick_matrices(pkg, case, x0, u, xs, params, kw, as_numpy=False)
    nx, nq = sj.NX[model], sj.NX[model] // 2
    w = torch.tensor(gkw.get("weights", [1.0] * nx), dtype=torch.float32, device=DEV)
    om = gkw.get("tick_weights", torch.ones((nt, B), dtype=torch.float32, device=DEV))
    P = torch.eye(nx, dtype=torch.float32, device=DEV)[:, :, None].repeat(1, 1, B)
    cost = torch.zeros(B, dtype=torch.float32, device=DEV)
    g = torch.zeros((nx, B), dtype=torch.float32, device=DEV)
    H = torch.zeros((nx, nx, B), dtype=torch.float32, device=DEV)
    for t in range(nt):
        P = torch.einsum("rcb,cjb->rjb", A[t], P)
        r = x_obs[t] - xs[t]
        r[1:nq] = r[1:nq] - 2 * np.pi * torch.round(r[1:nq] / (2 * np.pi))
        wr = w[:, None] * r
        cost = cost + 0.5 * om[t] * (wr * r).sum(dim=0)
        g = g - om[t] * torch.einsum("qjb,qb->jb", P, wr)
        H = H + om[t] * torch.einsum("qjb,q,qkb->jkb", P, w, P)
    return dict(cost=cost, g=g, H=H, Phi_final=P)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_within_four_times_the_parents_float_chain(pkg, case):
    x0, u, x_obs, _, params, kw, gkw = tensors(pkg, case, torch.float32)
    kw64 = dict(gkw)
    for name in ("fext", "tick_weights"):
        if name in kw64:
            kw64[name] = kw64[name].double()
    p64 = params.double() if isinstance(params, torch.Tensor) else params
    ref = pkg.sim_rollout_gauss_newton_x0(p64, case[1], x0.double(), u.double(), x_obs.double(), want=OUTS, **kw64)
    got = call(pkg, case, torch.float32)
    chain = _float_chain(pkg, case)
    ok = True
    for name in ("Phi_final", "g", "H", "cost"):
        ek, ec = lane_dist(N_(got[name]), N_(ref[name])), lane_dist(N_(chain[name]), N_(ref[name]))
        km, k99, cm, c99 = np.median(ek), np.percentile(ek, 99), np.median(ec), np.percentile(ec, 99)
        print("fp32 %s %s from the fp64 kernel: one call median %.2e p99 %.2e | parent's chain median %.2e p99 %.2e (bound 4 x; "
              "ratios %.2f %.2f)" % (IDS[CASES.index(case)], name, km, k99, cm, c99, km / cm if cm else 0.0,
                                     k99 / c99 if c99 else 0.0))
        ok = ok and km <= 4 * cm and k99 <= 4 * c99
    assert ok


# ---- 6. bitwise and structural ------------------------------------------------------------------------------------------
STRUCT = [c for c in CASES if c[1] == 0.0105]
STRUCT_IDS = ["%s-%g-%d-%s" % c for c in STRUCT]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_outputs_do_not_depend_on_each_other_and_the_inputs_are_read_only(pkg, case, dtype):
    x0, u, x_obs, _, params, _, gkw = tensors(pkg, case, dtype)
    held = [x0, u, x_obs] + ([params] if isinstance(params, torch.Tensor) else []) + \
           [gkw[k] for k in ("fext", "tick_weights") if k in gkw]
    kept = [t.clone() for t in held]
    every = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    again = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    nx = sj.NX[case[0]]
    for name in OUTS:
        assert torch.isfinite(every[name]).all(), name
        assert torch.equal(every[name], again[name]), name
        alone = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=name, **gkw)
        assert torch.equal(alone[name], every[name]), name
    pair = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=("H", "x_final"), **gkw)
    assert torch.equal(pair["H"], every["H"]) and torch.equal(pair["x_final"], every["x_final"])
    free = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, None, want=("Phi_final", "x_final"),
                                           **{k: v for k, v in gkw.items() if k not in ("weights", "tick_weights")})
    assert torch.equal(free["Phi_final"], every["Phi_final"]) and torch.equal(free["x_final"], every["x_final"])
    assert every["H"].shape == (nx, nx, B) and every["Phi_final"].shape == (nx, nx, B) and every["g"].shape == (nx, B)
    assert torch.equal(every["H"], every["H"].transpose(0, 1))
    for a, b in zip(kept, held):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_tick_weights(pkg, case, dtype):
    x0, u, x_obs, _, params, _, gkw = tensors(pkg, case, dtype)
    nt, cut = case[2], 3
    plain = {k: v for k, v in gkw.items() if k != "tick_weights"}
    fit = ("cost", "g", "H")
    # ones are None
    none = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=fit, **plain)
    ones = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=fit,
                                           tick_weights=torch.ones((nt, B), dtype=dtype, device=DEV), **plain)
    for name in fit:
        assert torch.equal(none[name], ones[name]), name
    # zero from tick `cut` on: the sums of a `cut`-tick call
    om = gkw["tick_weights"].clone() if "tick_weights" in gkw else torch.ones((nt, B), dtype=dtype, device=DEV)
    om[cut:] = 0.0
    long_ = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=fit, tick_weights=om, **plain)
    short = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u[:cut].contiguous(), x_obs[:cut].contiguous(), want=fit,
                                            tick_weights=om[:cut].contiguous(), **plain)
    for name in fit:
        assert torch.equal(long_[name], short[name]), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("nb,kind", [(B, None), (B, "dyn"), (B, "tw"), (B, "w"), (1, None)])
def test_dt_zero(pkg, model, dtype, nb, kind):
    case = (model, 0.0, 3, kind)
    nx = sj.NX[model]
    x0, u, x_obs, _, params, _, gkw = tensors(pkg, case, dtype, nb)
    got = pkg.sim_rollout_gauss_newton_x0(params, 0.0, x0, u, x_obs, want=OUTS, **gkw)
    assert torch.equal(got["x_final"], x0)
    eye = torch.eye(nx, dtype=dtype, device=DEV)[:, :, None].expand(nx, nx, nb)
    assert torch.equal(got["Phi_final"], eye)
    w = torch.tensor(gkw.get("weights", [1.0] * nx), dtype=dtype, device=DEV)
    om = gkw.get("tick_weights", torch.ones((3, nb), dtype=dtype, device=DEV))
    want_H = torch.zeros((nx, nx, nb), dtype=dtype, device=DEV)
    for t in range(3):
        for j in range(nx):
            want_H[j, j] = want_H[j, j] + om[t] * w[j]
    assert torch.equal(got["H"], want_H)                       # H == sum om_t W, bitwise
    nq = nx // 2
    want_g = torch.zeros((nx, nb), dtype=dtype, device=DEV)
    mag = torch.zeros((nx, nb), dtype=dtype, device=DEV)
    for t in range(3):
        r = x_obs[t] - x0
        r[1:nq] = r[1:nq] - 2 * np.pi * torch.round(r[1:nq] / (2 * np.pi))
        want_g = want_g - om[t] * (w[:, None] * r)
        mag = mag + (om[t] * (w[:, None] * r)).abs()
    ratio = ((got["g"] - want_g).abs() / (8 * _eps(dtype) * mag)).max().item()
    print("dt = 0 %s %s B=%d %s: g against -sum om W r, worst |difference| / (8 eps sum |om W r|) %.3f" % (model, dtype, nb, kind,
                                                                                                          ratio))
    # two roundings a term on either side and the sums' own: 8 eps of the terms' magnitudes, elementwise; 0 where all are 0
    assert torch.equal(got["g"][mag == 0], want_g[mag == 0]) and not (ratio > 1.0)


def _t_sum(dt, nt, dtype):
    """the sub-steps' lengths of the window added up in the kernel's order and type"""
    npt = np.float32 if dtype == torch.float32 else np.float64
    total = npt(0.0)
    hs = sj.sub_steps(dt)
    for _ in range(nt):
        for i, h in enumerate(hs):
            total = npt(total + (npt(h) if i + 1 == len(hs) else npt(0.001)))
    return float(total)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in CASES if c[3] in (None, "dyn", "per")], ids=lambda c: "%s-%g-%d-%s" % c)
def test_closed_form_columns_are_exact(pkg, case, dtype):
    """6-state model: columns 0 (the cart's position) and 3 (its velocity) never enter the dynamics, so Phi_final[:, 0] = e_0 and
    Phi_final[:, 3] = e_3 + t_sum e_0 with t_sum the window's length as the kernel adds it up.  4-state model: the position enters
    through the bumpers alone, so column 0 is e_0 on the lanes that stay off them."""
    model, dt, nt, _ = case
    nx = sj.NX[model]
    x0, u, x_obs, xs, params, _, gkw = tensors(pkg, case, dtype)
    P = pkg.sim_rollout_gauss_newton_x0(params, dt, x0, u, x_obs, want="Phi_final", **gkw)["Phi_final"]
    e = torch.eye(nx, dtype=dtype, device=DEV)
    if model == "double":
        t_sum = _t_sum(dt, nt, dtype)
        assert torch.equal(P[:, 0], e[:, 0, None].expand(nx, B))
        want3 = e[:, 3, None].expand(nx, B).clone()
        want3[0] = t_sum
        print("closed form %s %s: t_sum %.17g, kernel's %.17g" % (IDS[CASES.index(case)], dtype, t_sum, P[0, 3, 0].item()))
        assert torch.equal(P[:, 3], want3)
    else:
        x_s = params[7] if isinstance(params, torch.Tensor) else torch.full((B,), sj.BUMPER_X, dtype=dtype, device=DEV)
        reach = torch.maximum(x0[0].abs(), xs[:, 0].abs().max(dim=0).values)
        off = reach < 0.95 * x_s
        assert 20 <= int(off.sum()) < B
        assert torch.equal(P[:, 0][:, off], e[:, 0, None].expand(nx, int(off.sum())))
        if dt > 0:
            assert (P[2, 0][~off] != 0).any()   # and not everywhere: the bumper's spring


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
def test_a_nan_pole_angle_stays_in_its_lane(pkg, model, dtype):
    case, lane = (model, 0.0105, 5, "dyn"), 37
    x0, u, x_obs, _, params, _, gkw = tensors(pkg, case, dtype)
    clean = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    bad = x0.clone()
    bad[1, lane] = float("nan")
    got = pkg.sim_rollout_gauss_newton_x0(params, case[1], bad, u, x_obs, want=OUTS, **gkw)
    others = [b for b in range(B) if b != lane]
    for name in OUTS:
        assert not torch.isfinite(got[name][..., lane]).all(), name
        assert torch.equal(got[name][..., others], clean[name][..., others]), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_a_single_problem_is_lane_0_of_the_batch(pkg, case, dtype):
    x0, u, x_obs, _, params, _, gkw = tensors(pkg, case, dtype)
    one_kw = dict(gkw)
    for name in ("fext", "tick_weights"):
        if name in one_kw:
            one_kw[name] = gkw[name][:, :1].contiguous()
    p1 = params[:, :1].contiguous() if isinstance(params, torch.Tensor) else params
    x1, u1, o1 = (t[..., :1].contiguous() for t in (x0, u, x_obs))
    every = pkg.sim_rollout_gauss_newton_x0(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    one = pkg.sim_rollout_gauss_newton_x0(p1, case[1], x1, u1, o1, want=OUTS, **one_kw)
    for name in OUTS:
        assert one[name].shape == every[name].shape[:-1] + (1,), name
        assert torch.equal(one[name][..., 0], every[name][..., 0]), name


# ---- 7. estimation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gx.EST_CASES))
def test_sim_estimate_state_recovers_every_plants_state(pkg, name):
    """130 plants, one noise-free recorded window of 8 ticks each (the parent's rollout under random controls); from the truth
    +- (0.1 m, 0.1 rad, 0.2 m/s, 0.2 rad/s) every lane recovers the window's first state to 1e-9 within 8 undamped iterations,
    and with damping 1e-3 within 16 (section 5h's reasoning for the damped count); the arrival cost alone returns the prior; a
    lane whose recording holds a NaN keeps its guess with ok = 0 and no other lane notices.  The CPU twin
    (tests/test_sim_rollout_gn_x0_ref.py) is at 4e-15 / 8e-14 / 1.1e-13 after four iterations."""
    model, w = gx.EST_CASES[name]
    nx = sj.NX[model]
    truth, start, usn = gx.estimation_draws(model, B)
    x_true, guess, u = Tn(truth), Tn(start), Tn(usn)
    prm = [float(v) for v in sj.DYN[model]]
    rec = pkg.sim_rollout_states(prm, gx.EST_DT, x_true, u, model=model, want=("xs", "x_final"))
    x_obs = rec["xs"]
    kw = dict(model=model, weights=w)
    for it in (1, 2, 3, 4):
        res = pkg.sim_estimate_state(prm, gx.EST_DT, guess, u, x_obs, iterations=it, **kw)
        print("estimate (%s) undamped, %d iterations: worst |x0 - truth| %.2e, worst cost %.2e"
              % (name, it, np.abs(N_(res["x0"]) - truth).max(), res["cost"].max().item()))
    errs = {}
    for label, damping, its in (("undamped", 0.0, 8), ("damping 1e-3", 1e-3, 16)):
        res = pkg.sim_estimate_state(prm, gx.EST_DT, guess, u, x_obs, iterations=its, damping=damping, **kw)
        errs[label] = np.abs(N_(res["x0"]) - truth).max()
        e_now = np.abs(N_(res["x_final"]) - N_(rec["x_final"])).max()
        print("estimate (%s) %s, %d iterations: worst |x0 - truth| %.2e (bound 1e-9), current state %.2e, ok %d of %d, worst cost "
              "%.2e" % (name, label, its, errs[label], e_now, int(res["ok"].sum()), B, res["cost"].max().item()))
        assert res["x0"].shape == (nx, B) and res["x_final"].shape == (nx, B) and res["cost"].shape == (B,)
        assert res["H"].shape == (nx, nx, B) and res["ok"].shape == (B,) and res["ok"].dtype == torch.int32
        assert (res["ok"] == 1).all()
        if damping == 0.0:
            clean = res
    assert torch.equal(guess, Tn(start))                            # the starting guess is not changed
    assert max(errs.values()) <= 1e-9
    # H and x_final are those of the estimate
    at = pkg.sim_rollout_gauss_newton_x0(prm, gx.EST_DT, clean["x0"], u, x_obs, want=("H", "x_final"), **kw)
    assert torch.equal(at["H"], clean["H"]) and torch.equal(at["x_final"], clean["x_final"])
    # the arrival cost alone: one step lands on the prior, H is Pi
    prior = Tn(truth + 0.01)
    for info in (torch.ones((nx, B), dtype=torch.float64, device=DEV),
                 torch.eye(nx, dtype=torch.float64, device=DEV)[:, :, None].repeat(1, 1, B)):
        res = pkg.sim_estimate_state(prm, gx.EST_DT, guess, u, x_obs, iterations=1, prior=prior, prior_info=info,
                                     tick_weights=torch.zeros((gx.EST_T, B), dtype=torch.float64, device=DEV), **kw)
        ulps = ((res["x0"] - prior).abs() / (np.finfo(np.float64).eps * prior.abs().max(dim=0).values)).max().item()
        print("estimate (%s) arrival cost alone, prior_info %s: |x0 - prior| %.1f ulp of the lane's largest entry"
              % (name, tuple(info.shape), ulps))
        assert ulps <= 4 and (res["ok"] == 1).all()
        assert torch.equal(res["H"], torch.eye(nx, dtype=torch.float64, device=DEV)[:, :, None].expand(nx, nx, B))
    # a NaN in one lane's recording
    lane = 77
    bad = x_obs.clone()
    bad[3, 0, lane] = float("nan")
    got = pkg.sim_estimate_state(prm, gx.EST_DT, guess, u, bad, iterations=8, **kw)
    others = [b for b in range(B) if b != lane]
    assert got["ok"][lane] == 0 and (got["ok"][others] == 1).all()
    assert torch.equal(got["x0"][:, lane], guess[:, lane])
    assert torch.equal(got["x0"][:, others], clean["x0"][:, others])


def test_sim_identify_is_where_it_was(pkg):
    """sim_identify shares its accept / reject loop with sim_estimate_state: the loop written out here as the parent had it
    gives the same parameters, bit for bit, undamped and damped."""
    from helpers import sim_rollout_gn_ref as gn
    batch = __import__("importlib").import_module(pkg.__name__ + ".batch")
    model, idx, w = gn.IDENT_CASES["b"]
    true, start, x0n, usn = gn.identification_draws(model, idx, B)
    x0, u, p_true, p0 = Tn(x0n), Tn(usn), Tn(true), Tn(start)
    x_obs = pkg.sim_rollout_states(p_true, gn.IDENT_DT, x0, u, model=model)["xs"]

    def evaluate(q):
        return pkg.sim_rollout_gauss_newton(q, gn.IDENT_DT, x0, u, x_obs, weights=w, model=model)

    for damping, its in ((0.0, 4), (1e-3, 6)):
        p = p0.clone()
        cur = evaluate(p)
        live = torch.isfinite(cur["cost"])
        mu = torch.full((B,), float(damping), dtype=torch.float64, device=DEV)
        for _ in range(its):
            H, g = cur["H"], cur["g"]
            Hs = [[H[cj, ci] * (1.0 + mu) if ci == cj else H[cj, ci] for ci in idx] for cj in idx]
            delta, pd = batch._cholesky_solve_lanes(Hs, [g[c] for c in idx])
            for d in delta:
                pd = pd & torch.isfinite(d)
            live = live & pd
            trial = p.clone()
            for c, d in zip(idx, delta):
                trial[c] = torch.where(live, p[c] - d, p[c])
            new = evaluate(trial)
            if damping > 0.0:
                take = live & (new["cost"] < cur["cost"])
                mu = torch.where(take, mu * 0.1, mu * 10.0)
            else:
                take = live & torch.isfinite(new["cost"])
                live = take
            p = torch.where(take, trial, p)
            cur = {n: torch.where(take, new[n], cur[n]) for n in ("cost", "g", "H")}
        res = pkg.sim_identify(p0, gn.IDENT_DT, x0, u, x_obs, idx, iterations=its, damping=damping, weights=w, model=model)
        assert torch.equal(res["params"], p) and torch.equal(res["cost"], cur["cost"])
        assert torch.equal(res["ok"], live.to(torch.int32))


# ---- 8. the moving horizon --------------------------------------------------------------------------------------------------
def test_window_estimator_tracks_the_plants(pkg):
    """24 ticks of the parent's rollout at B = 64, noise-free positions, a window of 8, two iterations a tick: from the tick
    the window is full the returned current state is within ten times what the CPU twin reaches on the same draws
    (helpers: WINDOW_TWIN_WORST, pinned by tests/test_sim_rollout_gn_x0_ref.py); and at one tick the result is bitwise a direct
    sim_estimate_state call on the same window and guess."""
    model, w = "single", gx.EST_CASES["b"][1]
    nb, ticks, T, its = gx.WINDOW_B, gx.WINDOW_TICKS, gx.WINDOW_T, gx.WINDOW_ITERATIONS
    truth, guess, usn = gx.window_draws(model)
    prm = [float(v) for v in sj.DYN[model]]
    u = Tn(usn)
    xs = pkg.sim_rollout_states(prm, gx.EST_DT, Tn(truth), u, model=model)["xs"]
    est = pkg.WindowEstimator(prm, gx.EST_DT, nb, T, state=Tn(guess), model=model, weights=w)
    worst, direct_checked = 0.0, False
    for t in range(ticks):
        y = xs[t].clone()
        y[2:] = 0.0                                    # the velocities are not measured: whatever finite number
        est.push(u[t].contiguous(), y)
        if t == 13:
            g0, uw, yw, ww = (a.clone() for a in est.held())
            direct = pkg.sim_estimate_state(prm, gx.EST_DT, g0, uw, yw, iterations=its, weights=w, tick_weights=ww, model=model)
        now = est.estimate(iterations=its)
        assert now.shape == (sj.NX[model], nb)
        if t == 13:
            assert torch.equal(now, direct["x_final"]) and uw.shape == (T, nb)
            direct_checked = True
        if t >= T - 1:
            d = N_(now) - N_(xs[t])
            d[1] -= 2 * np.pi * np.round(d[1] / (2 * np.pi))
            worst = max(worst, np.abs(d).max())
    print("window estimator: %d lanes, %d ticks, window %d, %d iterations a tick: worst |current state - truth| from the tick the "
          "window is full %.2e (the CPU twin %.2e, bound 10 x)" % (nb, ticks, T, its, worst, gx.WINDOW_TWIN_WORST))
    assert direct_checked
    assert worst <= 10 * gx.WINDOW_TWIN_WORST
