"""The rollout's forward mode in the parameters with the Gauss-Newton normal equations of a window on the GPU
(cpmpc_sim_rollout_gn_batch; sim_rollout_gauss_newton, sim_identify) against the parent's one-tick calls, against the rollout's
adjoint, and against the numpy reference of tests/helpers/sim_rollout_gn_ref.py, which tests/test_sim_rollout_gn_ref.py pins.

Shapes: B = 130 -- two full waves and a 2-lane tail -- and B = 1; (dt, T) = (0.0105, 5), (0.02, 3), (0.001, 8), (0, 3): 11 / 20 /
1 / 0 sub-steps a tick; both models, both dtypes; the states of sim_jac_ref.states; the case kinds of test_gpu_sim_rollout.py
(shared forces, [4, B] forces, per-problem parameters DYN (1 +- 20 %)) and two of this call's own: "w", positions-only state
weights (1, 1, 0, 0), and "tw", random per-sample weights in [0, 2].  The recording x_obs is the parent's sim_rollout_states
trajectory plus uniform +-0.1, which keeps the residuals far above rounding.

1. Against the float64 recurrence S_{t+1} = A_t S_t + P_t on the parent's sim_step_jacobian A_t and sim_step_param_jacobian P_t
   at the parent's checkpoints, elementwise.  S_final within f Sabs, f = 4 (NX + 1) T max(n_sub, 1) eps and Sabs the recurrence on
   absolute values (section 5g's bound: each of at most T levels is an NX-term contraction plus one addition; max(n_sub, 1)
   covers a last-digit difference per sub-step between the carried tangents and the separately compiled kernels' A and P; 4 is
   the project's margin).  H, g, cost within the first-order propagation of that through their sums, with c = 4 NX T eps for the
   sums themselves and dx = 4 T max(n_sub, 1) eps max(1, |x|) for the kernel's own states against the parent's:
       H:    (2 f + c) sum om Sabs^T W Sabs
       g:    (f + c) sum om Sabs^T W |r|  +  sum om Sabs^T W dx
       cost: c 1/2 sum om |r|^T W |r|    +  sum om |r|^T W dx
2. Forward against reverse: g equals sim_rollout_vjp(gbar[t] = -om_t W r_t)["p"] within g's bound of 1.
3. T = 1: S_final against sim_step_param_jacobian's P within 1's bound; whether it is bitwise is printed.
4. fp64 against the oracle's reference: x_final within T 1e-12, S_final, g, H within T 1e-7 of the lane's largest reference entry.
5. fp32: per lane the distance of each output from the fp64 kernel's at the same float-rounded inputs, relative to the lane's
   largest entry; median and 99th percentile at most 4 x those of the parent's float chain (the same recurrence and sums
   composed by hand in float torch from the float one-tick calls).
6. bitwise and structural properties.  7. identification (sim_identify), fp64.
Every test prints its figures before it asserts; DESIGN.md section 5h is where they are recorded."""
import numpy as np
import pytest

from helpers import sim_jac_ref as sj
from helpers import sim_param_ref as sp
from helpers import sim_rollout_gn_ref as gn

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
OUTS = ("cost", "g", "H", "S_final", "x_final")


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1
    assert callable(pkg.sim_rollout_gauss_newton)   # imports the batch module; fails on a tree without the call


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
    """A [T, nx, nx, B], P [T, nx, np, B] from the parent's one-tick calls at the checkpoints x_t = x0, xs[0], ..  P:
    sim_step_param_jacobian.  A: sim_step_jacobian; with a parameter tensor, which that call does not take, sim_step_param_vjp
    on the unit cotangents (row r of A per call), as tests/test_gpu_sim_rollout.py does."""
    model, dt, nt, _ = case
    nx = sj.NX[model]
    A, P = [], []
    for t in range(nt):
        xt = x0 if t == 0 else xs[t - 1].contiguous()
        ut = u[t].contiguous()
        P.append(pkg.sim_step_param_jacobian(params, dt, xt, ut, want="P", **kw)["P"])
        if isinstance(params, torch.Tensor):
            rows = []
            for r in range(nx):
                e = torch.zeros_like(xt)
                e[r] = 1.0
                rows.append(pkg.sim_step_param_vjp(params, dt, xt, ut, e, want="x", **kw)["x"])
            A.append(torch.stack(rows))
        else:
            A.append(pkg.sim_step_jacobian(params, dt, xt, ut, want="A", **kw)["A"])
    A, P = torch.stack(A), torch.stack(P)
    return (N_(A), N_(P)) if as_numpy else (A, P)


def wrapped_residuals(model, x_obs, xs):
    """x_obs - xs with the pole angles' differences wrapped, numpy [T, nx, B]"""
    r = x_obs - xs
    nq = sj.NX[model] // 2
    r[:, 1:nq] -= 2 * np.pi * np.round(r[:, 1:nq] / (2 * np.pi))
    return r


_REF = {}


def ref_and_bound(pkg, case, dtype, nb=B):
    """the float64 recurrence and sums on the parent's per-tick matrices, and the elementwise bounds of test 1 -> two dicts
    with S_final, H, g, cost; computed once per (case, dtype)"""
    key = (case, dtype, nb)
    if key not in _REF:
        model, dt, nt, _ = case
        nx = sj.NX[model]
        x0, u, x_obs, xs, params, kw, _ = tensors(pkg, case, dtype, nb)
        _, _, _, _, _, w, om = inputs(case, nb)
        w = np.ones(nx) if w is None else w
        om = np.ones((nt, nb)) if om is None else N_(Tn(om, dtype))
        A, P = tick_matrices(pkg, case, x0, u, xs, params, kw)
        S, Sabs = gn.sensitivities(A, P), gn.sensitivities(np.abs(A), np.abs(P))
        r = wrapped_residuals(model, N_(x_obs), N_(xs))
        cost, g, H = gn.normal_equations(S, r, w, om)
        n_sub, eps = max(len(sj.sub_steps(dt)), 1), _eps(dtype)
        f, c = 4 * (nx + 1) * nt * n_sub * eps, 4 * nx * nt * eps
        dx = 4 * nt * n_sub * eps * np.maximum(1.0, np.abs(N_(xs)))
        ra = np.abs(r)
        b_H = (2 * f + c) * np.einsum("tb,tqjb,q,tqkb->jkb", om, Sabs, w, Sabs)
        b_g = (f + c) * np.einsum("tb,tqjb,q,tqb->jb", om, Sabs, w, ra) + np.einsum("tb,tqjb,q,tqb->jb", om, Sabs, w, dx)
        b_c = c * 0.5 * np.einsum("tb,q,tqb,tqb->b", om, w, ra, ra) + np.einsum("tb,q,tqb,tqb->b", om, w, ra, dx)
        _REF[key] = (dict(S_final=S[-1], H=H, g=g, cost=cost), dict(S_final=f * Sabs[-1], H=b_H, g=b_g, cost=b_c))
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
    return pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=want, **gkw)


# ---- 1. against the parent's one-tick calls -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_outputs_are_the_recurrence_on_the_parents_tick_matrices(pkg, case, dtype):
    got = call(pkg, case, dtype)
    ref, bound = ref_and_bound(pkg, case, dtype)
    ratios = {name: worst_ratio(N_(got[name]), ref[name], bound[name]) for name in ("S_final", "H", "g", "cost")}
    print("gn %s %s: worst |out - ref| / bound: %s" % (IDS[CASES.index(case)], dtype,
                                                        "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert all(torch.isfinite(got[name]).all() for name in OUTS)
    assert max(ratios.values()) <= 1.0
    if case[1] > 0:
        assert (N_(got["S_final"]) != 0).any() and (N_(got["H"]) != 0).any()


# ---- 2. forward against reverse -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_g_is_the_adjoints_parameter_gradient(pkg, case, dtype):
    model, dt, nt, _ = case
    x0, u, x_obs, xs, params, kw, gkw = tensors(pkg, case, dtype)
    nq = sj.NX[model] // 2
    r = x_obs - xs
    r[:, 1:nq] = r[:, 1:nq] - 2 * np.pi * torch.round(r[:, 1:nq] / (2 * np.pi))
    w = torch.tensor(gkw.get("weights", [1.0] * sj.NX[model]), dtype=dtype, device=DEV)
    om = gkw.get("tick_weights", torch.ones((nt, B), dtype=dtype, device=DEV))
    gbar = (-(om[:, None, :] * (w[None, :, None] * r))).contiguous()
    rev = pkg.sim_rollout_vjp(params, dt, x0, u, xs, gbar=gbar, want="p", **kw)["p"]
    fwd = call(pkg, case, dtype, want="g")["g"]
    _, bound = ref_and_bound(pkg, case, dtype)
    ratio = worst_ratio(N_(fwd), N_(rev), bound["g"])
    print("gn %s %s: forward g against the adjoint's g_p, worst |difference| / bound %.3f" % (IDS[CASES.index(case)], dtype, ratio))
    assert ratio <= 1.0


# ---- 3. one tick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [None, "dyn"])
@pytest.mark.parametrize("model", ["single", "double"])
def test_one_tick_is_the_parents_param_jacobian(pkg, model, kind, dtype):
    case = (model, 0.0105, 1, kind)
    x0, u, _, _, params, kw, _ = tensors(pkg, case, dtype)
    got = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, None, want=("S_final", "x_final"), **kw)
    one = pkg.sim_step_param_jacobian(params, case[1], x0, u[0].contiguous(), **kw)
    _, bound = ref_and_bound(pkg, case, dtype)
    ratio = worst_ratio(N_(got["S_final"]), N_(one["P"]), bound["S_final"])
    print("T = 1 %s %s %s: |S_final - P| / bound %.3f, bitwise S_final: %s, bitwise x_final: %s" % (
        model, kind, dtype, ratio, torch.equal(got["S_final"], one["P"]), torch.equal(got["x_final"], one["x_new"])))
    assert ratio <= 1.0


# ---- 4. fp64 against the oracle's reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp64_matches_the_oracles_reference(pkg, orc, case):
    model, dt, nt, _ = case
    x, us, _, f, prm, w, om = inputs(case)
    _, _, x_obs, _, _, _, _ = tensors(pkg, case, torch.float64)
    xs_ref, S_ref = gn.oracle_route_batch(orc, model, prm, dt, x, us, fext=f)
    _, g_ref, H_ref = gn.normal_equations(S_ref, gn.residuals(orc, model, N_(x_obs), xs_ref), w, om)
    got = call(pkg, case, torch.float64)
    ex = np.abs(N_(got["x_final"]) - xs_ref[-1]).max()
    errs = [lane_dist(N_(got[n]), r).max() for n, r in (("S_final", S_ref[-1]), ("g", g_ref), ("H", H_ref))]
    print("fp64 %s against the oracle: |x_final - ref| %.2e (bound %.0e)  S_final %.2e  g %.2e  H %.2e of the lane's max (bound %.0e)"
          % (IDS[CASES.index(case)], ex, nt * 1e-12, *errs, nt * 1e-7))
    assert ex <= nt * 1e-12
    assert max(errs) <= nt * 1e-7


# ---- 5. fp32 against the parent's float chain ---------------------------------------------------------------------------
def _float_chain(pkg, case):
    """the recurrence and the sums in float torch on the float one-tick calls at the float trajectory's checkpoints"""
    model, dt, nt, _ = case
    x0, u, x_obs, xs, params, kw, gkw = tensors(pkg, case, torch.float32)
    A, P = tick_matrices(pkg, case, x0, u, xs, params, kw, as_numpy=False)
    nx, nq = sj.NX[model], sj.NX[model] // 2
    w = torch.tensor(gkw.get("weights", [1.0] * nx), dtype=torch.float32, device=DEV)
    om = gkw.get("tick_weights", torch.ones((nt, B), dtype=torch.float32, device=DEV))
    S = torch.zeros_like(P[0])
    cost = torch.zeros(B, dtype=torch.float32, device=DEV)
    g = torch.zeros((P.shape[2], B), dtype=torch.float32, device=DEV)
    H = torch.zeros((P.shape[2], P.shape[2], B), dtype=torch.float32, device=DEV)
    for t in range(nt):
        S = torch.einsum("rcb,cjb->rjb", A[t], S) + P[t]
        r = x_obs[t] - xs[t]
        r[1:nq] = r[1:nq] - 2 * np.pi * torch.round(r[1:nq] / (2 * np.pi))
        wr = w[:, None] * r
        cost = cost + 0.5 * om[t] * (wr * r).sum(dim=0)
        g = g - om[t] * torch.einsum("qjb,qb->jb", S, wr)
        H = H + om[t] * torch.einsum("qjb,q,qkb->jkb", S, w, S)
    return dict(cost=cost, g=g, H=H, S_final=S)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_within_four_times_the_parents_float_chain(pkg, case):
    x0, u, x_obs, _, params, kw, gkw = tensors(pkg, case, torch.float32)
    kw64 = dict(gkw)
    for name in ("fext", "tick_weights"):
        if name in kw64:
            kw64[name] = kw64[name].double()
    p64 = params.double() if isinstance(params, torch.Tensor) else params
    ref = pkg.sim_rollout_gauss_newton(p64, case[1], x0.double(), u.double(), x_obs.double(), want=OUTS, **kw64)
    got = call(pkg, case, torch.float32)
    chain = _float_chain(pkg, case)
    ok = True
    for name in ("S_final", "g", "H", "cost"):
        ek, ec = lane_dist(N_(got[name]), N_(ref[name])), lane_dist(N_(chain[name]), N_(ref[name]))
        km, k99, cm, c99 = np.median(ek), np.percentile(ek, 99), np.median(ec), np.percentile(ec, 99)
        print("fp32 %s %s from the fp64 kernel: one call median %.2e p99 %.2e | parent's chain median %.2e p99 %.2e (bound 4 x)"
              % (IDS[CASES.index(case)], name, km, k99, cm, c99))
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
    every = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    again = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    for name in OUTS:
        assert torch.isfinite(every[name]).all(), name
        assert torch.equal(every[name], again[name]), name
        alone = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=name, **gkw)
        assert torch.equal(alone[name], every[name]), name
    pair = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=("H", "x_final"), **gkw)
    assert torch.equal(pair["H"], every["H"]) and torch.equal(pair["x_final"], every["x_final"])
    assert every["H"].shape == (sp.NP[case[0]], sp.NP[case[0]], B) and every["S_final"].shape == (sj.NX[case[0]], sp.NP[case[0]], B)
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
    none = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=fit, **plain)
    ones = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=fit,
                                        tick_weights=torch.ones((nt, B), dtype=dtype, device=DEV), **plain)
    for name in fit:
        assert torch.equal(none[name], ones[name]), name
    # zero from tick `cut` on: the sums of a `cut`-tick call
    om = gkw["tick_weights"].clone() if "tick_weights" in gkw else torch.ones((nt, B), dtype=dtype, device=DEV)
    om[cut:] = 0.0
    long_ = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=fit, tick_weights=om, **plain)
    short = pkg.sim_rollout_gauss_newton(params, case[1], x0, u[:cut].contiguous(), x_obs[:cut].contiguous(), want=fit,
                                         tick_weights=om[:cut].contiguous(), **plain)
    for name in fit:
        assert torch.equal(long_[name], short[name]), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("nb,kind", [(B, None), (B, "dyn"), (1, None)])
def test_dt_zero(pkg, model, dtype, nb, kind):
    case = (model, 0.0, 3, kind)
    x0, u, x_obs, _, params, _, gkw = tensors(pkg, case, dtype, nb)
    got = pkg.sim_rollout_gauss_newton(params, 0.0, x0, u, x_obs, want=OUTS, **gkw)
    assert torch.equal(got["x_final"], x0)
    for name in ("S_final", "H", "g"):
        assert (got[name] == 0).all(), name
    nq = sj.NX[model] // 2
    want = torch.zeros(nb, dtype=dtype, device=DEV)
    for t in range(3):
        r = x_obs[t] - x0
        r[1:nq] = r[1:nq] - 2 * np.pi * torch.round(r[1:nq] / (2 * np.pi))
        want = want + 0.5 * (r * r).sum(dim=0)
    err = ((got["cost"] - want).abs() / want).max().item()
    print("dt = 0 %s %s B=%d %s: cost against the weighted residual of x0, worst relative difference %.2e (bound %.1e)"
          % (model, dtype, nb, kind, err, 4 * sj.NX[model] * 3 * _eps(dtype)))
    assert (want > 0).all() and err <= 4 * sj.NX[model] * 3 * _eps(dtype)   # the sums' own term c of test 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [None, "dyn", "per"])
def test_bumper_columns_vanish_off_the_bumpers(pkg, kind, dtype):
    case = ("single", 0.0105, 5, kind)
    x0, u, x_obs, xs, params, _, gkw = tensors(pkg, case, dtype)
    got = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    x_s = params[sp.COL_XS] if isinstance(params, torch.Tensor) else torch.full((B,), sj.BUMPER_X, dtype=dtype, device=DEV)
    reach = torch.maximum(x0[0].abs(), xs[:, 0].abs().max(dim=0).values)
    off = reach < 0.95 * x_s
    print("bumpers %s %s: %d of %d lanes stay off the bumpers" % (kind, dtype, int(off.sum()), B))
    assert 20 <= int(off.sum()) < B
    for c in (sp.COL_XS, sp.COL_KS):
        assert (got["S_final"][:, c][:, off] == 0).all() and (got["g"][c][off] == 0).all()
        assert (got["H"][c][:, off] == 0).all() and (got["H"][:, c][:, off] == 0).all()
    assert (got["S_final"][:, sp.COL_KS][:, ~off] != 0).any()   # and not everywhere


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
def test_a_nan_pole_angle_stays_in_its_lane(pkg, model, dtype):
    case, lane = (model, 0.0105, 5, "dyn"), 37
    x0, u, x_obs, _, params, _, gkw = tensors(pkg, case, dtype)
    clean = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    bad = x0.clone()
    bad[1, lane] = float("nan")
    got = pkg.sim_rollout_gauss_newton(params, case[1], bad, u, x_obs, want=OUTS, **gkw)
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
    every = pkg.sim_rollout_gauss_newton(params, case[1], x0, u, x_obs, want=OUTS, **gkw)
    one = pkg.sim_rollout_gauss_newton(p1, case[1], x1, u1, o1, want=OUTS, **one_kw)
    for name in OUTS:
        assert one[name].shape == every[name].shape[:-1] + (1,), name
        assert torch.equal(one[name][..., 0], every[name][..., 0]), name


# ---- 7. identification ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gn.IDENT_CASES))
def test_sim_identify_recovers_every_plants_parameters(pkg, name):
    """130 plants, each with its own three parameters within +-10 % of DYN, one recorded window of 8 ticks each (the parent's
    rollout under the true parameters); from the nominal set every lane recovers its parameters to 1e-9 relative within 8
    iterations undamped, and with damping 1e-3 within 16; a lane whose recording holds a NaN keeps its parameters with ok = 0
    and no other lane notices.  The CPU twin (tests/test_sim_rollout_gn_ref.py) reaches 2e-13 / 2.6e-11 / 4e-13 in four
    iterations.

    Why 16 for the damped run: the error along H's weakest direction shrinks by mu / (lambda_min + mu) a step, lambda_min of
    the diagonally scaled H being 3 / cond >= 1.2e-4 (cond <= 2.4e4, case b), so from mu = 1e-3 at a tenth per accepted step
    it takes five accepted steps until mu << lambda_min and two more of Gauss-Newton's own; and a step whose cost rises is
    not taken, which spends that iteration and a factor 10 in mu that an accepted step has to win back -- two iterations a
    rejection.  Measured with 8 iterations, worst lane: (a) 6.5e-14, (b) 2.5e-5 (two rejections at the start), (c) 2.3e-14;
    the figure after 8 is printed beside the one after 16."""
    model, idx, w = gn.IDENT_CASES[name]
    true, start, x0n, usn = gn.identification_draws(model, idx, B)
    x0, u, p_true, p0 = Tn(x0n), Tn(usn), Tn(true), Tn(start)
    x_obs = pkg.sim_rollout_states(p_true, gn.IDENT_DT, x0, u, model=model)["xs"]
    kw = dict(model=model, weights=w)
    for it in (1, 2, 3, 4):
        res = pkg.sim_identify(p0, gn.IDENT_DT, x0, u, x_obs, idx, iterations=it, **kw)
        print("identify (%s) undamped, %d iterations: worst relative parameter error %.2e, worst cost %.2e"
              % (name, it, np.abs(N_(res["params"])[idx] / true[idx] - 1.0).max(), res["cost"].max().item()))
    res = pkg.sim_identify(p0, gn.IDENT_DT, x0, u, x_obs, idx, iterations=8, damping=1e-3, **kw)
    print("identify (%s) damping 1e-3, 8 iterations: worst relative parameter error %.2e (not asserted)"
          % (name, np.abs(N_(res["params"])[idx] / true[idx] - 1.0).max()))
    errs = {}
    for label, damping, its in (("undamped", 0.0, 8), ("damping 1e-3", 1e-3, 16)):
        res = pkg.sim_identify(p0, gn.IDENT_DT, x0, u, x_obs, idx, iterations=its, damping=damping, **kw)
        est = N_(res["params"])
        errs[label] = np.abs(est[idx] / true[idx] - 1.0).max()
        rest = [j for j in range(sp.NP[model]) if j not in idx]
        print("identify (%s) %s, %d iterations: worst relative parameter error %.2e (bound 1e-9), ok %d of %d, worst cost %.2e"
              % (name, label, its, errs[label], int(res["ok"].sum()), B, res["cost"].max().item()))
        assert res["params"].shape == (sp.NP[model], B) and res["cost"].shape == (B,) and res["ok"].shape == (B,)
        assert np.array_equal(est[rest], start[rest])          # the other parameters stay as given
        assert (res["ok"] == 1).all()
        if damping == 0.0:
            clean = res
    assert torch.equal(p0, Tn(start))                            # the starting point is not changed
    assert max(errs.values()) <= 1e-9
    lane = 77
    bad = x_obs.clone()
    bad[3, 0, lane] = float("nan")
    got = pkg.sim_identify(p0, gn.IDENT_DT, x0, u, bad, idx, iterations=8, **kw)
    others = [b for b in range(B) if b != lane]
    assert got["ok"][lane] == 0 and (got["ok"][others] == 1).all()
    assert torch.equal(got["params"][:, lane], p0[:, lane])
    assert torch.equal(got["params"][:, others], clean["params"][:, others])
