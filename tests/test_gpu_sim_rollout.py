"""The plant rollout over T ticks and its adjoint on the GPU (cpmpc_sim_rollout_batch, cpmpc_sim_rollout_vjp_batch;
sim_rollout_states, sim_rollout_vjp, sim_rollout, BatchSimulator.rollout / rollout_differentiable) against the parent's
one-tick calls and against the numpy reference of tests/helpers/sim_rollout_ref.py, which tests/test_sim_rollout_ref.py pins.

Shapes: B = 130 -- two full waves and a 2-lane tail -- and B = 1; (dt, T) = (0.0105, 5), (0.02, 3), (0.001, 8), (0, 3): 11 / 20 /
1 / 0 sub-steps a tick; both models, both dtypes; the states of sim_jac_ref.states (a block of lanes wraps inside the step;
for the 4-state model a block sits beyond the bumpers); one case with shared forces, one with [4, B] forces, one per model
with per-problem parameters DYN (1 +- 20 %).

1. forward: xs[t] is BITWISE what t + 1 BatchSimulator.step calls leave, in both dtypes -- the tick body is the same code.
2. VJP: against the recurrence run in float64 numpy on the parent's per-tick A_t, Bu_t, P_t at the checkpoints, elementwise
   |g - g_ref| <= 4 (NX + 1) T max(n_sub, 1) eps S, S the same recurrence on absolute values: each of at most T levels is an
   NX-term contraction plus one addition; max(n_sub, 1) covers a last-digit difference between the in-register Phi and the
   separately compiled kernel's A per sub-step; 4 is the project's margin (tests/test_gpu_sim_jac.py).
3. fp64 against the oracle's reference: gradients within T 1e-7 of the lane's max |ref| (the suite's per-step bound for P and
   for finite differences, accumulated to first order), xs within T 1e-12.
4. fp32: per lane the distance of each gradient from the fp64 kernel's at the same float-rounded inputs, relative to the
   lane's max; median and 99th percentile at most 4 x those of the parent's float chain (T sim_step_param_vjp calls composed
   by hand in reverse order).
5. bitwise and structural properties; 6. autograd.
Every test prints its figures before it asserts; DESIGN.md section 5g is where they are recorded."""
import numpy as np
import pytest

from helpers import sim_jac_ref as sj
from helpers import sim_param_ref as sp
from helpers import sim_rollout_ref as sr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = 130
DT_T = ((0.0105, 5), (0.02, 3), (0.001, 8), (0.0, 3))
# (model, dt, T, kind): kind None, "shared" forces, "per"-problem forces, "dyn" per-problem parameters
CASES = [(m, dt, nt, None) for m in ("single", "double") for dt, nt in DT_T] + \
        [("single", 0.0105, 5, "shared"), ("single", 0.0105, 5, "per"), ("single", 0.0105, 5, "dyn"), ("double", 0.0105, 5, "dyn")]
IDS = ["%s-%g-%d-%s" % c for c in CASES]
DTYPES = [torch.float64, torch.float32]
SHARED_F = ((1.5, 0.0), (-2.0, 1.0))


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1
    assert callable(pkg.sim_rollout_states)   # imports the batch module


def Tn(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _eps(dtype):
    return float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)


_IN = {}


def inputs(case, nb=B):
    """numpy inputs of a case, made once and left unchanged: x0 [nx, nb], us [T, nb], gbar [T, nx, nb], gbar_final [nx, nb],
    forces (None, 4 shared numbers or [4, nb]) and parameters (np numbers or [np, nb])."""
    key = (case, nb)
    if key not in _IN:
        model, dt, nt, kind = case
        x, _ = sj.states(model, nb)
        rng = np.random.default_rng(41)
        us = rng.uniform(-20.0, 20.0, (nt, nb))
        gb = rng.uniform(-1.0, 1.0, (nt, sj.NX[model], nb))
        gf = rng.uniform(-1.0, 1.0, (sj.NX[model], nb))
        f = None
        if kind == "shared":
            f = np.array([SHARED_F[0][0], SHARED_F[0][1], SHARED_F[1][0], SHARED_F[1][1]])
        elif kind == "per":
            f = np.random.default_rng(21).uniform(-3.0, 3.0, (4, nb))
        prm = np.array(sj.DYN[model])
        if kind == "dyn":
            prm = np.tile(prm[:, None], (1, nb)) * np.random.default_rng(43).uniform(0.8, 1.2, (len(prm), nb))
        _IN[key] = (x, us, gb, gf, f, prm)
        for a in _IN[key]:
            if a is not None:
                a.setflags(write=False)
    return _IN[key]


def tensors(case, dtype, nb=B):
    """-> x0, u, gbar, gbar_final tensors, params (list or tensor) and the force keywords of the package's calls"""
    x, us, gb, gf, f, prm = inputs(case, nb)
    kw = dict(model=case[0])
    if case[3] == "shared":
        kw.update(f_base=SHARED_F[0], f_mass=SHARED_F[1])
    elif case[3] == "per":
        kw.update(fext=Tn(f, dtype))
    params = Tn(prm, dtype) if prm.ndim == 2 else [float(v) for v in prm]
    return Tn(x, dtype), Tn(us, dtype), Tn(gb, dtype), Tn(gf, dtype), params, kw


def _sim_kw(kw):
    return {k: v for k, v in kw.items() if k != "model"}


def chain_states(pkg, case, dtype, x0, u, params, kw):
    """[T, nx, B]: the state after each of T BatchSimulator.step calls on a twin (the parent's plant step)"""
    twin = pkg.BatchSimulator(x0.shape[1], dtype=dtype, device=0, model=case[0])
    twin.set_state(x0)
    out = []
    for t in range(case[2]):
        twin.step(params, case[1], u[t].contiguous(), **_sim_kw(kw))
        out.append(twin.get_state().clone())
    return torch.stack(out)


def tick_matrices(pkg, case, x0, u, xs, params, kw):
    """A [T, nx, nx, B], Bu [T, nx, B], P [T, nx, np, B] in float64 numpy from the parent's one-tick calls at the checkpoints
    x_t = x0, xs[0], ..  P: sim_step_param_jacobian.  A, Bu: sim_step_jacobian; with a parameter tensor, which that call does
    not take, sim_step_param_vjp on the unit cotangents (row r of A and entry r of Bu per call)."""
    model, dt, nt, _ = case
    nx = sj.NX[model]
    A, Bu, P = [], [], []
    for t in range(nt):
        xt = x0 if t == 0 else xs[t - 1].contiguous()
        ut = u[t].contiguous()
        P.append(N_(pkg.sim_step_param_jacobian(params, dt, xt, ut, want="P", **kw)["P"]))
        if isinstance(params, torch.Tensor):
            At, Bt = np.zeros((nx, nx, xt.shape[1])), np.zeros((nx, xt.shape[1]))
            for r in range(nx):
                e = torch.zeros_like(xt)
                e[r] = 1.0
                v = pkg.sim_step_param_vjp(params, dt, xt, ut, e, want=("x", "u"), **kw)
                At[r], Bt[r] = N_(v["x"]), N_(v["u"])
        else:
            j = pkg.sim_step_jacobian(params, dt, xt, ut, want=("A", "Bu"), **kw)
            At, Bt = N_(j["A"]), N_(j["Bu"])
        A.append(At)
        Bu.append(Bt)
    return np.stack(A), np.stack(Bu), np.stack(P)


def ref_and_bound(pkg, case, dtype, x0, u, xs, params, kw, gb, gf):
    """the float64 recurrence on the parent's per-tick matrices and the elementwise bound of test 2 -> (refs, bounds)"""
    A, Bu, P = tick_matrices(pkg, case, x0, u, xs, params, kw)
    g = None if gb is None else N_(gb)
    f = None if gf is None else N_(gf)
    ref = sr.recurrence(A, Bu, P, g, f)
    S = sr.recurrence(np.abs(A), np.abs(Bu), np.abs(P), None if g is None else np.abs(g), None if f is None else np.abs(f))
    factor = 4 * (sj.NX[case[0]] + 1) * case[2] * max(len(sj.sub_steps(case[1])), 1) * _eps(dtype)
    return ref, [factor * s for s in S]


def worst_ratio(got, ref, bound):
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0))))


def lane_dist(got, ref):
    """per lane: max |got - ref| relative to the lane's max |ref|; a lane whose reference is all zero must be all zero"""
    ax = tuple(range(ref.ndim - 1))
    d, s = np.abs(got - ref).max(axis=ax), np.abs(ref).max(axis=ax)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))


# ---- 1. forward against the parent's plant step -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_is_the_chained_plant_step_bitwise(pkg, case, dtype):
    x0, u, _, _, params, kw = tensors(case, dtype)
    keep = x0.clone()
    both = pkg.sim_rollout_states(params, case[1], x0, u, want=("xs", "x_final"), **kw)
    chain = chain_states(pkg, case, dtype, x0, u, params, kw)
    print("forward %s %s: worst |xs - chained step| %.3e (bitwise asked)" % (IDS[CASES.index(case)], dtype,
                                                                              (both["xs"] - chain).abs().max().item()))
    assert torch.isfinite(both["xs"]).all()
    assert torch.equal(both["xs"], chain)
    assert torch.equal(both["x_final"], both["xs"][-1])
    assert torch.equal(pkg.sim_rollout_states(params, case[1], x0, u, want="xs", **kw)["xs"], both["xs"])
    assert torch.equal(pkg.sim_rollout_states(params, case[1], x0, u, want="x_final", **kw)["x_final"], both["x_final"])
    assert torch.equal(x0, keep)
    if case[1] == 0.0:
        for t in range(case[2]):
            assert torch.equal(both["xs"][t], x0)
    else:
        nq = sj.NX[case[0]] // 2
        assert ((both["xs"][0][1:nq, :2] - x0[1:nq, :2]).abs() > 3.0).all(), "lanes 0 and 1 did not wrap inside the first tick"


# ---- 2. the VJP against the parent's per-tick matrices ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_vjp_is_the_recurrence_on_the_parents_tick_matrices(pkg, case, dtype):
    x0, u, gb, gf, params, kw = tensors(case, dtype)
    xs = pkg.sim_rollout_states(params, case[1], x0, u, **kw)["xs"]
    worst = {}
    for name, g, f in (("gbar", gb, None), ("gbar_final", None, gf), ("both", gb, gf)):
        got = pkg.sim_rollout_vjp(params, case[1], x0, u, xs, gbar=g, gbar_final=f, **kw)
        ref, bound = ref_and_bound(pkg, case, dtype, x0, u, xs, params, kw, g, f)
        worst[name] = [worst_ratio(N_(got[w]), r, b) for w, r, b in zip(("x", "u", "p"), ref, bound)]
    print("vjp %s %s: worst |g - g_ref| / bound, g_x0 / g_u / g_p: %s" % (
        IDS[CASES.index(case)], dtype, "  ".join("%s %.3f %.3f %.3f" % (k, *v) for k, v in worst.items())))
    assert max(max(v) for v in worst.values()) <= 1.0


# ---- 3. fp64 against the oracle's reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp64_matches_the_oracles_reference(pkg, orc, case):
    model, dt, nt, _ = case
    x, us, gb, _, f, prm = inputs(case)
    x0, u, gbt, _, params, kw = tensors(case, torch.float64)
    xs_ref, *g_ref = sr.adjoint_batch(orc, model, prm, dt, x, us, gbar=gb, fext=f)
    xs = pkg.sim_rollout_states(params, dt, x0, u, **kw)["xs"]
    got = pkg.sim_rollout_vjp(params, dt, x0, u, xs, gbar=gbt, **kw)
    ex = np.abs(N_(xs) - xs_ref).max()
    errs = [lane_dist(N_(got[w]), r).max() for w, r in zip(("x", "u", "p"), g_ref)]
    print("fp64 %s against the oracle: |xs - ref| %.2e (bound %.0e)  g_x0 %.2e  g_u %.2e  g_p %.2e of the lane's max (bound %.0e)"
          % (IDS[CASES.index(case)], ex, nt * 1e-12, *errs, nt * 1e-7))
    assert ex <= nt * 1e-12
    assert max(errs) <= nt * 1e-7


# ---- 4. fp32 against the parent's float chain ---------------------------------------------------------------------------
def _float_chain(pkg, case, x0, u, gb, params, kw):
    """T sim_step_param_vjp calls in reverse order at the checkpoints of T chained BatchSimulator.step calls, in float"""
    model, dt, nt, _ = case
    xs = chain_states(pkg, case, torch.float32, x0, u, params, kw)
    lam = torch.zeros_like(x0)
    g_u = torch.zeros_like(u)
    g_p = None
    for t in range(nt - 1, -1, -1):
        lam = lam + gb[t]
        v = pkg.sim_step_param_vjp(params, dt, x0 if t == 0 else xs[t - 1].contiguous(), u[t].contiguous(), lam.contiguous(), **kw)
        g_u[t] = v["u"]
        g_p = v["p"] if g_p is None else g_p + v["p"]
        lam = v["x"]
    return lam, g_u, g_p


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_within_four_times_the_parents_float_chain(pkg, case):
    x0, u, gb, _, params, kw = tensors(case, torch.float32)
    x64, u64, g64 = x0.double(), u.double(), gb.double()
    p64, kw64 = (params.double() if isinstance(params, torch.Tensor) else params), dict(kw)
    if "fext" in kw64:
        kw64["fext"] = kw["fext"].double()
    xs64 = pkg.sim_rollout_states(p64, case[1], x64, u64, **kw64)["xs"]
    ref = pkg.sim_rollout_vjp(p64, case[1], x64, u64, xs64, gbar=g64, **kw64)
    xs32 = pkg.sim_rollout_states(params, case[1], x0, u, **kw)["xs"]
    got = pkg.sim_rollout_vjp(params, case[1], x0, u, xs32, gbar=gb, **kw)
    chain = dict(zip(("x", "u", "p"), _float_chain(pkg, case, x0, u, gb, params, kw)))
    ok = True
    for w in ("x", "u", "p"):
        ek, ec = lane_dist(N_(got[w]), N_(ref[w])), lane_dist(N_(chain[w]), N_(ref[w]))
        km, k99, cm, c99 = np.median(ek), np.percentile(ek, 99), np.median(ec), np.percentile(ec, 99)
        print("fp32 %s g_%s from the fp64 kernel: rollout median %.2e p99 %.2e | parent's chain median %.2e p99 %.2e (bound 4 x)"
              % (IDS[CASES.index(case)], w, km, k99, cm, c99))
        ok = ok and km <= 4 * cm and k99 <= 4 * c99
    assert ok


# ---- 5. bitwise and structural ------------------------------------------------------------------------------------------
STRUCT = [c for c in CASES if c[1] in (0.0105,)]
STRUCT_IDS = ["%s-%g-%d-%s" % c for c in STRUCT]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_outputs_do_not_depend_on_each_other_and_the_inputs_are_read_only(pkg, case, dtype):
    x0, u, gb, gf, params, kw = tensors(case, dtype)
    xs = pkg.sim_rollout_states(params, case[1], x0, u, **kw)["xs"]
    kept = [t.clone() for t in (x0, u, gb, gf, xs)] + ([params.clone()] if isinstance(params, torch.Tensor) else [])
    every = pkg.sim_rollout_vjp(params, case[1], x0, u, xs, gbar=gb, gbar_final=gf, **kw)
    again = pkg.sim_rollout_vjp(params, case[1], x0, u, xs, gbar=gb, gbar_final=gf, **kw)
    for w in ("x", "u", "p"):
        assert torch.isfinite(every[w]).all(), w
        assert torch.equal(every[w], again[w]), w
        alone = pkg.sim_rollout_vjp(params, case[1], x0, u, xs, gbar=gb, gbar_final=gf, want=w, **kw)
        assert torch.equal(alone[w], every[w]), w
    pair = pkg.sim_rollout_vjp(params, case[1], x0, u, xs, gbar=gb, gbar_final=gf, want=("x", "u"), **kw)
    assert torch.equal(pair["x"], every["x"]) and torch.equal(pair["u"], every["u"])
    now = [x0, u, gb, gf, xs] + ([params] if isinstance(params, torch.Tensor) else [])
    for a, b in zip(kept, now):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("nb,kind", [(B, None), (B, "dyn"), (1, None)])
def test_dt_zero_is_the_identity(pkg, model, dtype, nb, kind):
    case = (model, 0.0, 3, kind)
    x0, u, gb, gf, params, kw = tensors(case, dtype, nb)
    res = pkg.sim_rollout_states(params, 0.0, x0, u, want=("xs", "x_final"), **kw)
    for t in range(3):
        assert torch.equal(res["xs"][t], x0)
    assert torch.equal(res["x_final"], x0)
    g = pkg.sim_rollout_vjp(params, 0.0, x0, u, res["xs"], gbar=gb, gbar_final=gf, **kw)
    assert torch.equal(g["x"], ((gb[2] + gf) + gb[1]) + gb[0])   # the cotangents added in the kernel's order, not multiplied
    assert (g["u"] == 0).all() and (g["p"] == 0).all()
    only = pkg.sim_rollout_vjp(params, 0.0, x0, u, res["xs"], gbar=gb, **kw)
    assert torch.equal(only["x"], (gb[2] + gb[1]) + gb[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [None, "dyn"])
@pytest.mark.parametrize("model", ["single", "double"])
def test_one_tick_is_the_parents_one_step_vjp(pkg, model, kind, dtype):
    case = (model, 0.0105, 1, kind)
    x0, u, _, gf, params, kw = tensors(case, dtype)
    got = pkg.sim_rollout_vjp(params, case[1], x0, u, None, gbar_final=gf, **kw)
    one = pkg.sim_step_param_vjp(params, case[1], x0, u[0].contiguous(), gf, **kw)
    _, bound = ref_and_bound(pkg, case, dtype, x0, u, None, params, kw, None, gf)
    ratios = [worst_ratio(N_(got["x"]), N_(one["x"]), bound[0]), worst_ratio(N_(got["u"])[0], N_(one["u"]), bound[1][0]),
              worst_ratio(N_(got["p"]), N_(one["p"]), bound[2])]
    print("T = 1 %s %s %s: |rollout vjp - sim_step_param_vjp| / bound, gx / gu / gp: %.3f %.3f %.3f" % (model, kind, dtype, *ratios))
    assert max(ratios) <= 1.0
    with_xs = pkg.sim_rollout_vjp(params, case[1], x0, u, pkg.sim_rollout_states(params, case[1], x0, u, **kw)["xs"],
                                  gbar_final=gf, **kw)
    for w in ("x", "u", "p"):
        assert torch.equal(with_xs[w], got[w]), w   # row T-1 of xs is never loaded


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
def test_a_nan_pole_angle_stays_in_its_lane(pkg, model, dtype):
    case, lane = (model, 0.0105, 5, "dyn"), 37
    x0, u, gb, gf, params, kw = tensors(case, dtype)
    clean_xs = pkg.sim_rollout_states(params, case[1], x0, u, **kw)["xs"]
    clean = pkg.sim_rollout_vjp(params, case[1], x0, u, clean_xs, gbar=gb, gbar_final=gf, **kw)
    bad = x0.clone()
    bad[1, lane] = float("nan")
    xs = pkg.sim_rollout_states(params, case[1], bad, u, **kw)["xs"]
    got = pkg.sim_rollout_vjp(params, case[1], bad, u, xs, gbar=gb, gbar_final=gf, **kw)
    others = [b for b in range(B) if b != lane]
    assert not torch.isfinite(xs[..., lane]).all()
    assert torch.equal(xs[..., others], clean_xs[..., others])
    for w in ("x", "u", "p"):
        assert not torch.isfinite(got[w][..., lane]).all(), w
        assert torch.equal(got[w][..., others], clean[w][..., others]), w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_a_single_problem_is_lane_0_of_the_batch(pkg, case, dtype):
    x0, u, gb, gf, params, kw = tensors(case, dtype)
    one_kw = dict(kw)
    if "fext" in kw:
        one_kw["fext"] = kw["fext"][:, :1].contiguous()
    p1 = params[:, :1].contiguous() if isinstance(params, torch.Tensor) else params
    x1, u1, gb1, gf1 = (t[..., :1].contiguous() for t in (x0, u, gb, gf))
    xs = pkg.sim_rollout_states(params, case[1], x0, u, **kw)["xs"]
    xs1 = pkg.sim_rollout_states(p1, case[1], x1, u1, **one_kw)["xs"]
    assert xs1.shape == (case[2], sj.NX[case[0]], 1) and torch.equal(xs1[..., 0], xs[..., 0])
    g = pkg.sim_rollout_vjp(params, case[1], x0, u, xs, gbar=gb, gbar_final=gf, **kw)
    g1 = pkg.sim_rollout_vjp(p1, case[1], x1, u1, xs1, gbar=gb1, gbar_final=gf1, **one_kw)
    assert g1["x"].shape == (sj.NX[case[0]], 1) and g1["u"].shape == (case[2], 1) and g1["p"].shape == (sp.NP[case[0]], 1)
    for w in ("x", "u", "p"):
        assert torch.equal(g1[w][..., 0], g[w][..., 0]), w


# ---- 6. autograd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in STRUCT if c[3] in (None, "dyn")], ids=[i for i, c in zip(STRUCT_IDS, STRUCT)
                                                                                   if c[3] in (None, "dyn")])
def test_autograd_is_one_vjp_call_and_agrees_with_the_chained_steps(pkg, case, dtype):
    x0, u, gb, _, params, kw = tensors(case, dtype)
    per_problem = isinstance(params, torch.Tensor)
    xs = pkg.sim_rollout_states(params, case[1], x0, u, **kw)["xs"]
    direct = pkg.sim_rollout_vjp(params, case[1], x0, u, xs, gbar=gb, **kw)

    def leaves():
        a, b = x0.clone().requires_grad_(True), u.clone().requires_grad_(True)
        p = params.clone().requires_grad_(True) if per_problem else params
        return a, b, p

    a, b, p = leaves()
    out = pkg.sim_rollout(p, case[1], a, b, **kw)
    assert torch.equal(out.detach(), xs)
    out.backward(gb)
    assert torch.equal(a.grad, direct["x"]) and torch.equal(b.grad, direct["u"])
    if per_problem:
        assert torch.equal(p.grad, direct["p"])

    a2, b2, p2 = leaves()
    x, loss = a2, 0.0
    for t in range(case[2]):
        x = pkg.sim_step(p2, case[1], x, b2[t], **kw)
        loss = loss + (gb[t] * x).sum()
    loss.backward()
    ref, bound = ref_and_bound(pkg, case, dtype, x0, u, xs, params, kw, gb, None)
    ratios = [worst_ratio(N_(a2.grad), N_(direct["x"]), bound[0]), worst_ratio(N_(b2.grad), N_(direct["u"]), bound[1])]
    if per_problem:
        ratios.append(worst_ratio(N_(p2.grad), N_(direct["p"]), bound[2]))
    print("autograd %s %s: |chained sim_step gradients - rollout's| / bound: %s" % (IDS[CASES.index(case)], dtype,
                                                                                   " ".join("%.3f" % r for r in ratios)))
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
def test_batch_simulator_rollout(pkg, model, dtype):
    case = (model, 0.0105, 5, "dyn")
    x0, u, gb, _, params, kw = tensors(case, dtype)
    chain = chain_states(pkg, case, dtype, x0, u, params, kw)
    sim = pkg.BatchSimulator(B, dtype=dtype, device=0, model=model)
    sim.set_state(x0)
    xs = sim.rollout(params, case[1], u)
    assert torch.equal(xs, chain) and torch.equal(sim.get_state(), chain[-1])
    sim.step(params, case[1], u[0].contiguous())          # the state is the simulator's own: a step does not reach into xs
    assert torch.equal(xs, chain)
    dif = pkg.BatchSimulator(B, dtype=dtype, device=0, model=model)
    dif.set_state(x0)
    uu = u.clone().requires_grad_(True)
    ys = dif.rollout_differentiable(params, case[1], uu)
    assert torch.equal(ys.detach(), chain) and torch.equal(dif.get_state().detach(), chain[-1])
    ys.backward(gb)
    want = pkg.sim_rollout_vjp(params, case[1], x0, u, chain, gbar=gb, want="u", **kw)["u"]
    assert torch.equal(uu.grad, want)
