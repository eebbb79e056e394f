"""On the GPU: the LQR gains along a plant trajectory and the plant under an affine feedback law, one launch each
(cpmpc_sim_lqr_batch, cpmpc_sim_rollout_fb_batch; sim_lqr, sim_rollout_feedback, BatchSimulator.rollout_feedback,
ClosedLoop.tick_hold) against the numpy reference of tests/helpers/sim_lqr_ref.py, which tests/test_sim_lqr_ref.py pins and whose
inputs it shows to be admissible.

1. fp64 against the reference (the textbook Riccati recursion on the oracle's Phi and gamma; the feedback rollout through the
   oracle's step): K, P0, and the feedback rollout's xs and us within T 1e-7 of the lane's largest reference entry, the siblings'
   bound for derived quantities; with K = None xs within T 1e-12.
2. fp32 against the float64 reference ON THE FLOAT INPUTS, the siblings' rule.  For K and P0: gap = the distance of the
   reference's float32-algebra run from its float64 run (worst lane, relative to the lane's largest entry); the kernel may be
   8 x gap away plus the siblings' state bound 4 T max(n_sub, 1) eps max(1, |x|), |x| the lane's largest state along its
   trajectory: that part covers what a float Phi and gamma add (the reference's float32 run takes both from float64), and the
   tick Jacobian's rounding grows with the velocities that enter it.  Measured: the kernel's K is within 2.8e-7 (2.4 eps) of the
   float64 recursion run on the float Phi and gamma that sim_step_jacobian returns for the same tick, so everything beyond that
   is the float tick Jacobian's: at T = 1, dt = 0.0105 the 6-state model's worst lane (angle rates 4.5 rad/s beside the +-pi cut)
   has gamma 4.1e-6 and K 7.9e-6 from the reference, 1.15 x what the bound would be WITHOUT the max(1, |x|) factor (|x| = 4.9
   there) and 0.29 x with it, the worst of all cases; every other case stays below 0.7 x without it.  For the feedback rollout there is no covariance-like
   algebra: the state bound e = 4 max(n_sub, 1) eps max(1, |x|) a tick is carried through the law once per tick by |K|_1:
       E_0 = 0,   du_t = |K_t|_1 E_t + (nx + 2) eps (|u_nom_t| + sum_i |K_t,i d_i|),   E_{t+1} = E_t + e + g_t du_t,
   g_t = 1.25 x the largest |gamma| entry of the nominal tick (the plant's parameters are within 10 % of the nominal's); us[t] is
   held to du_t and xs[t] to E_{t+1}.
3. bitwise and structural properties.  4. dt = 0.  5. tracking, the CPU test's condition.  6. ClosedLoop.tick_hold."""
import numpy as np
import pytest

from helpers import batch_position as bp
from helpers import sim_jac_ref as sj
from helpers import sim_lqr_ref as lq

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = lq.B
CASES, IDS, FB_CASES, FB_IDS = lq.CASES, lq.IDS, lq.FB_CASES, lq.FB_IDS
DTYPES = [torch.float64, torch.float32]
FB_OUTS = ("xs", "x_final", "us")


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1
    assert callable(pkg.sim_lqr) and callable(pkg.sim_rollout_feedback)   # fails on a tree without the calls


def Tn(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _eps(dtype):
    return float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)


def lane_dist(got, ref):
    """per lane: max |got - ref| relative to the lane's max |ref|; a lane whose reference is all zero must be all zero"""
    ax = tuple(range(ref.ndim - 1))
    d, s = np.abs(got - ref).max(axis=ax), np.abs(ref).max(axis=ax)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))


def state_diff(model, got, ref):
    """|got - ref| of states [..., nx, B], the pole angles' differences to the nearest turn"""
    d = got - ref
    nq = sj.NX[model] // 2
    d[..., 1:nq, :] -= 2 * np.pi * np.round(d[..., 1:nq, :] / (2 * np.pi))
    return np.abs(d)


def same_bits(a, b, name="output", idx=None):
    msg = bp.first_difference(a, b, 1, idx, name)
    assert msg is None, msg


def _plant_kw(case, f, dtype, held=None):
    kw = dict(model=case[0])
    if case[3] == "shared":
        kw.update(f_base=lq.SHARED_F[0], f_mass=lq.SHARED_F[1])
    elif f is not None:
        kw.update(fext=Tn(f, dtype))
        if held is not None:
            held["f"] = N_(kw["fext"])
    return kw


def _params(prm, dtype, held=None):
    if prm.ndim == 2:
        t = Tn(prm, dtype)
        if held is not None:
            held["prm"] = N_(t)
        return t
    return [float(v) for v in prm]


_LQR = {}


def lqr_tensors(pkg, orc, case, dtype, nb=B):
    """-> the arguments of sim_lqr: (params, dt, state, u, xs, q, r), its keywords, and the case's arrays as the tensors hold them.
    xs is the GPU's own rollout, as a caller has it.  Made once per (case, dtype) and left unchanged."""
    key = (case, dtype, nb)
    if key not in _LQR:
        i = lq.inputs(orc, case, nb)
        held = dict(i)
        kw = _plant_kw(case, i["f"], dtype, held)
        params = _params(i["prm"], dtype, held)
        x0, u = Tn(i["x0"], dtype), Tn(i["us"], dtype)
        held.update(x0=N_(x0), us=N_(u))
        if i["PT"] is not None:
            kw["terminal"] = Tn(i["PT"], dtype)
            held["PT"] = N_(kw["terminal"])
        xs = pkg.sim_rollout_states(params, case[1], x0, u, **{k: v for k, v in kw.items() if k != "terminal"})["xs"]
        _LQR[key] = ((params, case[1], x0, u, xs, [float(v) for v in i["q"]], float(i["r"])), kw, held)
    return _LQR[key]


def call_lqr(pkg, orc, case, dtype, want=("K", "P0"), **over):
    args, kw, _ = lqr_tensors(pkg, orc, case, dtype)
    return pkg.sim_lqr(*args, want=want, **dict(kw, **over))


_FBT = {}


def fb_tensors(orc, case, dtype, nb=B):
    """-> the arguments of sim_rollout_feedback: (params, dt, state, u_nom, K, x0_nom, xs_nom), its keywords, the arrays held"""
    key = (case, dtype, nb)
    if key not in _FBT:
        i = lq.fb_inputs(orc, case, nb)
        held = dict(i)
        kw = _plant_kw(case, i["f"], dtype, held)
        kw["u_limit"] = float(i["u_limit"])
        params = _params(i["prm"], dtype, held)
        t = {n: None if i[n] is None else Tn(i[n], dtype) for n in ("x0", "u_nom", "K", "x0_nom", "xs_nom")}
        held.update({n: None if v is None else N_(v) for n, v in t.items()})
        _FBT[key] = ((params, case[1], t["x0"], t["u_nom"], t["K"], t["x0_nom"], t["xs_nom"]), kw, held)
    return _FBT[key]


def call_fb(orc, pkg, case, dtype, want=FB_OUTS, **over):
    args, kw, _ = fb_tensors(orc, case, dtype)
    return pkg.sim_rollout_feedback(*args, want=want, **dict(kw, **over))


# ---- 1. fp64 against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lqr_fp64_matches_the_reference(pkg, orc, case):
    nt = case[2]
    ref = lq.reference(orc, case)
    got = {n: N_(v) for n, v in call_lqr(pkg, orc, case, torch.float64).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    errs = dict(K=lane_dist(got["K"], ref["K"]).max(), P0=lane_dist(got["P0"], ref["P0"]).max())
    print("lqr fp64 %s against the reference, worst lane of its largest entry: %s (bound %.0e)" % (
        IDS[CASES.index(case)], "  ".join("%s %.2e" % kv for kv in errs.items()), nt * 1e-7))
    assert max(errs.values()) <= nt * 1e-7


@pytest.mark.parametrize("case", FB_CASES, ids=FB_IDS)
def test_feedback_rollout_fp64_matches_the_reference(pkg, orc, case):
    model, dt, nt, kind = case
    xs_ref, us_ref = lq.fb_reference(orc, case)
    got = {n: N_(v) for n, v in call_fb(orc, pkg, case, torch.float64).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    dx = state_diff(model, got["xs"], xs_ref)
    ex = (dx.max(axis=(0, 1)) / np.abs(xs_ref).max(axis=(0, 1))).max()
    eu = lane_dist(got["us"], us_ref).max()
    print("feedback rollout fp64 %s against the reference, worst lane of its largest entry: xs %.2e us %.2e (bound %.0e); "
          "|xs - ref| %.2e%s" % (FB_IDS[FB_CASES.index(case)], ex, eu, nt * 1e-7, dx.max(),
                                 " (bound %.0e: no feedback)" % (nt * 1e-12) if kind == "noK" else ""))
    if kind == "noK":
        assert dx.max() <= nt * 1e-12
    assert max(ex, eu) <= nt * 1e-7
    assert np.array_equal(got["xs"][-1], got["x_final"])
    if kind == "clamp":
        assert np.abs(got["us"]).max() == lq.FB_LIMIT and 0.1 <= (np.abs(got["us"]) == lq.FB_LIMIT).mean() <= 0.9


# ---- 2. fp32 against the float64 reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lqr_fp32_within_eight_times_the_float32_algebras_gap(pkg, orc, case):
    model, dt, nt, kind = case
    _, _, held = lqr_tensors(pkg, orc, case, torch.float32)
    ref = lq.reference(orc, case, arrays=held)
    r32 = lq.reference(orc, case, arrays=held, dtype=np.float32)
    got = {n: N_(v) for n, v in call_lqr(pkg, orc, case, torch.float32).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    # the siblings' state bound 4 T max(n_sub, 1) eps max(1, |x|), |x| the lane's largest state along its trajectory
    x_max = np.maximum(np.abs(held["x0"]).max(axis=0), np.abs(ref["xs"]).max(axis=(0, 1)))
    state = 4 * nt * max(len(sj.sub_steps(dt)), 1) * _eps(torch.float32) * np.maximum(1.0, x_max)
    ok = True
    for name in ("K", "P0"):
        gap = lane_dist(r32[name], ref[name]).max()
        bound = 8 * gap + state                              # per lane, relative to the lane's largest entry
        err = lane_dist(got[name], ref[name])
        worst = int(err.argmax())
        print("lqr fp32 %s %s: float32-algebra gap %.2e, kernel's error %.2e, error / bound %.3f (lane %d, max |x| there %.2f; "
              "%d lanes beyond the bound)" % (IDS[CASES.index(case)], name, gap, err.max(), (err / bound).max(), worst,
                                              max(np.abs(held["x0"][:, worst]).max(), np.abs(ref["xs"][:, :, worst]).max()),
                                              int((err > bound).sum())))
        ok = ok and bool((err <= bound).all())
    assert ok


@pytest.mark.parametrize("case", FB_CASES, ids=FB_IDS)
def test_feedback_rollout_fp32_within_the_state_bound_carried_through_the_law(pkg, orc, case):
    model, dt, nt, kind = case
    nx = sj.NX[model]
    _, _, held = fb_tensors(orc, case, torch.float32)
    xs_ref, us_ref = lq.fb_reference(orc, case, arrays=held)
    got = {n: N_(v) for n, v in call_fb(orc, pkg, case, torch.float32).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    eps = _eps(torch.float32)
    x_at = np.concatenate([held["x0"][None], xs_ref[:-1]])                      # the state at each tick's start
    e = 4 * max(len(sj.sub_steps(dt)), 1) * eps * np.maximum(1.0, np.abs(np.concatenate([x_at, xs_ref[-1:]])).max(axis=(0, 1)))
    E, worst_x, worst_u = np.zeros(B), 0.0, 0.0
    for t in range(nt):
        du = np.zeros(B)
        if held["K"] is not None:
            n_at = held["x0_nom"] if t == 0 else held["xs_nom"][t - 1]
            d = lq.wrap_nearest(model, x_at[t] - n_at)
            du = np.abs(held["K"][t]).sum(axis=0) * E + (nx + 2) * eps * (np.abs(held["u_nom"][t]) + np.abs(held["K"][t] * d).sum(axis=0))
        du = du + eps * np.abs(us_ref[t])                                       # the control as a float
        worst_u = max(worst_u, (np.abs(got["us"][t] - us_ref[t]) / du).max() if (du > 0).all() else float((got["us"][t] != us_ref[t]).any()))
        E = E + e + 1.25 * held["gam_max"][t] * du
        worst_x = max(worst_x, (state_diff(model, got["xs"][t], xs_ref[t]).max(axis=0) / E).max())
    print("feedback rollout fp32 %s: worst error / bound: xs %.3f us %.3f" % (FB_IDS[FB_CASES.index(case)], worst_x, worst_u))
    assert worst_x <= 1.0 and worst_u <= 1.0


# ---- 3. bitwise and structural --------------------------------------------------------------------------------------------
STRUCT = [c for c in CASES if c[1] == 0.0105 and c[2] == 5 and c[3] in (None, "dyn", "PT")]
STRUCT_IDS = ["%s-%g-%d-%s" % c for c in STRUCT]
FB_STRUCT = [c for c in FB_CASES if c[1] == 0.0105 and c[2] == 5 and c[3] in ("clamp", "mismatch")]
FB_STRUCT_IDS = ["%s-%g-%d-%s" % c for c in FB_STRUCT]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_lqr_outputs_do_not_depend_on_each_other_and_the_inputs_are_read_only(pkg, orc, case, dtype):
    args, kw, _ = lqr_tensors(pkg, orc, case, dtype)
    tensors = [a for a in args if isinstance(a, torch.Tensor)] + [v for v in kw.values() if isinstance(v, torch.Tensor)]
    before = [a.clone() for a in tensors]
    both = call_lqr(pkg, orc, case, dtype)
    for name in ("K", "P0"):
        same_bits(both[name], call_lqr(pkg, orc, case, dtype, want=name)[name], name + " alone")
    P = both["P0"]
    assert torch.equal(P, P.transpose(0, 1))                                  # exactly symmetric
    for a, b in zip(tensors, before):
        assert torch.equal(a, b)
    if "terminal" in kw:   # only PT's lower triangle is read: garbage above the diagonal changes nothing
        junk = kw["terminal"].clone()
        iu = np.triu_indices(junk.shape[0], 1)
        junk[iu[0], iu[1]] = float("nan")
        got = call_lqr(pkg, orc, case, dtype, terminal=junk)
        for name in ("K", "P0"):
            same_bits(both[name], got[name], name + " with NaNs above PT's diagonal")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", FB_STRUCT, ids=FB_STRUCT_IDS)
def test_feedback_rollout_outputs_do_not_depend_on_each_other(pkg, orc, case, dtype):
    every = call_fb(orc, pkg, case, dtype)
    for name in FB_OUTS:
        same_bits(every[name], call_fb(orc, pkg, case, dtype, want=name)[name], name + " alone")
    same_bits(every["xs"][-1], every["x_final"], "xs[-1]")


def _lqr_arranged(pkg, orc, case, dtype, idx):
    (params, dt, x0, u, xs, q, r), kw, _ = lqr_tensors(pkg, orc, case, dtype)
    kw = {k: bp.take(v, idx) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    prm = bp.take(params, idx) if isinstance(params, torch.Tensor) else params
    return pkg.sim_lqr(prm, dt, bp.take(x0, idx), bp.take(u, idx), bp.take(xs, idx), q, r, **kw)


def _fb_arranged(pkg, orc, case, dtype, idx):
    (params, dt, *ts), kw, _ = fb_tensors(orc, case, dtype)
    kw = {k: bp.take(v, idx) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    prm = bp.take(params, idx) if isinstance(params, torch.Tensor) else params
    return pkg.sim_rollout_feedback(prm, dt, *[bp.take(t, idx) for t in ts], want=FB_OUTS, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which,case", [("lqr", c) for c in STRUCT] + [("fb", c) for c in FB_STRUCT],
                         ids=["lqr-" + i for i in STRUCT_IDS] + ["fb-" + i for i in FB_STRUCT_IDS])
def test_a_lanes_bits_do_not_depend_on_its_place_in_the_batch(pkg, orc, which, case, dtype):
    """the same lanes reversed, and as prefixes that end alone, below, on and above a wave boundary"""
    natural = call_lqr(pkg, orc, case, dtype) if which == "lqr" else call_fb(orc, pkg, case, dtype)
    arranged = _lqr_arranged if which == "lqr" else _fb_arranged
    rev = bp.permutations(B, 7)["reverse"]
    got = arranged(pkg, orc, case, dtype, rev)
    for name in natural:
        same_bits(natural[name], bp.put_back(got[name], rev), name + " reversed", rev)
    for nb in (1, 63, 64, 65):
        idx = np.arange(nb, dtype=np.int64)
        got = arranged(pkg, orc, case, dtype, idx)
        for name in natural:
            same_bits(bp.take(natural[name], idx), got[name], "%s of the first %d" % (name, nb))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in FB_CASES if c[3] in ("noK", "per", "mismatch") or c[1] == 0.0],
                         ids=lambda c: "%s-%g-%d-%s" % c)
def test_without_gains_and_clamp_it_is_the_plain_rollout(pkg, orc, case, dtype):
    (params, dt, x0, u_nom, _, _, _), kw, _ = fb_tensors(orc, case, dtype)
    plant = {k: v for k, v in kw.items() if k != "u_limit"}
    roll = pkg.sim_rollout_states(params, dt, x0, u_nom, want=("xs", "x_final"), **plant)
    got = pkg.sim_rollout_feedback(params, dt, x0, u_nom, None, None, None, want=FB_OUTS, **plant)   # u_limit: infinity
    same_bits(roll["xs"], got["xs"], "xs")
    same_bits(roll["x_final"], got["x_final"], "x_final")
    same_bits(u_nom, got["us"], "us")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT + [c for c in CASES if c[2] in (1, 8, 12)], ids=lambda c: "%s-%g-%d-%s" % c)
def test_from_the_nominal_start_it_reproduces_the_nominal_rollout(pkg, orc, case, dtype):
    """x0 == x0_nom and the nominal's own plant: d is exactly 0 at every tick, whatever the (finite) gains and the clamp"""
    (params, dt, x0, u, xs, q, r), kw, _ = lqr_tensors(pkg, orc, case, dtype)
    plant = {k: v for k, v in kw.items() if k != "terminal"}
    K = call_lqr(pkg, orc, case, dtype, want="K")["K"]
    assert torch.isfinite(K).all() and (u != 0).all()
    got = pkg.sim_rollout_feedback(params, dt, x0, u, K, x0, xs, u_limit=300.0, want=FB_OUTS, **plant)
    same_bits(xs, got["xs"], "xs")
    same_bits(xs[-1], got["x_final"], "x_final")
    same_bits(u, got["us"], "us")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,t1", [(c, t1) for c in STRUCT for t1 in (2,)] + [(c, 5) for c in CASES if c[2] == 12],
                         ids=lambda v: "%s-%g-%d-%s" % v if isinstance(v, tuple) else str(v))
def test_a_window_is_its_tail_chained_into_its_head(pkg, orc, case, t1, dtype):
    (params, dt, x0, u, xs, q, r), kw, _ = lqr_tensors(pkg, orc, case, dtype)
    whole = call_lqr(pkg, orc, case, dtype)
    plant = {k: v for k, v in kw.items() if k != "terminal"}
    tail = pkg.sim_lqr(params, dt, xs[t1 - 1].contiguous(), u[t1:].contiguous(), xs[t1:].contiguous(), q, r, **kw)
    head = pkg.sim_lqr(params, dt, x0, u[:t1].contiguous(), xs[:t1].contiguous(), q, r, terminal=tail["P0"], **plant)
    same_bits(whole["P0"], head["P0"], "P0")
    same_bits(whole["K"][:t1], head["K"], "K of the head")
    same_bits(whole["K"][t1:], tail["K"], "K of the tail")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT[:2], ids=STRUCT_IDS[:2])
def test_a_poisoned_lane_stays_in_its_lane(pkg, orc, case, dtype):
    (params, dt, x0, u, xs, q, r), kw, _ = lqr_tensors(pkg, orc, case, dtype)
    clean = call_lqr(pkg, orc, case, dtype)
    lane = 70
    others = np.array([b for b in range(B) if b != lane], dtype=np.int64)
    bad = u.clone()
    bad[1, lane] = float("nan")
    got = pkg.sim_lqr(params, dt, x0, bad, xs, q, r, **kw)
    for name in ("K", "P0"):
        same_bits(bp.take(clean[name], others), bp.take(got[name], others), name)
    assert torch.isnan(got["P0"][:, :, lane]).any() and torch.isnan(got["K"][:, :, lane]).any()
    # and the feedback rollout under the poisoned gains
    fb_clean = pkg.sim_rollout_feedback(params, dt, x0, u, clean["K"], x0, xs, want=FB_OUTS, model=case[0])
    fb_bad = pkg.sim_rollout_feedback(params, dt, x0, u, got["K"], x0, xs, want=FB_OUTS, model=case[0])
    for name in FB_OUTS:
        same_bits(bp.take(fb_clean[name], others), bp.take(fb_bad[name], others), name)
    assert torch.isnan(fb_bad["us"][:, lane]).any() and torch.isnan(fb_bad["x_final"][:, lane]).any()


# ---- 4. dt = 0 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("tensor_terminal", [False, True])
def test_dt_zero_is_the_closed_form(pkg, orc, model, tensor_terminal, dtype):
    case = (model, 0.0, 3, None)
    (params, dt, x0, u, xs, q, r), kw, _ = lqr_tensors(pkg, orc, case, dtype)
    nt, nx = case[2], sj.NX[model]
    PT = Tn(lq.terminal_costs(model, B), dtype) if tensor_terminal else None
    got = pkg.sim_lqr(params, dt, x0, u, xs, q, r, terminal=PT, **kw)
    assert (got["K"] == 0).all()
    want = (N_(PT) if tensor_terminal else np.tile(np.diag(q)[:, :, None], (1, 1, B))) + nt * np.diag(q)[:, :, None]
    d = np.abs(N_(got["P0"]) - want) / np.maximum(np.abs(want), 1e-300)
    print("lqr dt = 0 %s %s: worst |P0 - (P_T + T diag(q))| relative %.2e (bound %.2e)" % (model, dtype, d.max(), nt * _eps(dtype)))
    assert (d <= nt * _eps(dtype)).all()
    off = ~np.eye(nx, dtype=bool)
    assert np.array_equal(N_(got["P0"])[off], (N_(PT) if tensor_terminal else np.zeros((nx, nx, B)))[off])
    assert got["K"].shape == (nt, nx, B)


# ---- 5. tracking ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
def test_tracking_beats_the_open_loop(pkg, model, dtype):
    """60 ticks of 10 ms near the upright, the start moved by 1e-2: on every lane the closed loop ends within 0.25 of the open
    loop's distance from the nominal end state (tests/test_sim_lqr_ref.py's condition), with the handle's 300 N clamp idle."""
    x_nom, u_nom, x0, qf = lq.tracking_draws(model, B)
    prm, dt = sj.DYN[model], lq.TRACK_DT
    x_nom, u_nom, x0 = Tn(x_nom, dtype), Tn(u_nom, dtype), Tn(x0, dtype)
    xs_nom = pkg.sim_rollout_states(prm, dt, x_nom, u_nom, model=model)["xs"]
    K = pkg.sim_lqr(prm, dt, x_nom, u_nom, xs_nom, list(lq.Q[model]), lq.R, terminal=qf, model=model, want="K")["K"]
    open_ = pkg.sim_rollout_states(prm, dt, x0, u_nom, model=model, want="x_final")["x_final"]
    sim = pkg.BatchSimulator(B, dtype=dtype, device=0, model=model)
    sim.set_state(x0)
    xs, us = sim.rollout_feedback(prm, dt, u_nom, K, x_nom, xs_nom, u_limit=300.0)
    same_bits(xs[-1], sim.get_state(), "the simulator's state")
    d_open = lq.deviation(model, N_(open_), N_(xs_nom[-1]))
    d_fb = lq.deviation(model, N_(xs[-1]), N_(xs_nom[-1]))
    print("tracking %s %s over %d ticks: worst closed / open ratio %.3f, open-loop growth at least %.1f x, max |u| %.2f" % (
        model, dtype, lq.TRACK_T, (d_fb / d_open).max(), (d_open / lq.TRACK_DELTA).min(), float(us.abs().max())))
    assert (d_open >= lq.TRACK_GROWTH * lq.TRACK_DELTA).all()
    assert (d_fb <= lq.TRACK_RATIO * d_open).all()
    assert float(us.abs().max()) < 300.0


# ---- 6. ClosedLoop.tick_hold ------------------------------------------------------------------------------------------------
HOLD_B = 256


def _hold_states(seed=11):
    rng = np.random.default_rng(seed)
    return Tn(np.stack([rng.uniform(-0.3, 0.3, HOLD_B), rng.uniform(-np.pi, np.pi, HOLD_B), rng.uniform(-0.5, 0.5, HOLD_B),
                        rng.uniform(-1.0, 1.0, HOLD_B)]))


def test_tick_hold_of_one_tick_is_tick(pkg):
    dyn, q = sj.DYN["single"], list(lq.Q["single"])
    loops = [pkg.ClosedLoop(pkg.default_params(), HOLD_B, dtype=torch.float64, device=0) for _ in range(2)]
    for cl in loops:
        cl.set_state(_hold_states())
    for t in range(3):
        loops[0].tick(dyn)
        loops[1].tick_hold(dyn, 1, q, lq.R)
        same_bits(loops[0].state(), loops[1].state(), "the plants' states at tick %d" % t)
        same_bits(loops[0].controls(), loops[1].controls(), "the plan at tick %d" % t)
        same_bits(loops[0].opts[0].get_solution(HOLD_B), loops[1].opts[0].get_solution(HOLD_B), "the warm start at tick %d" % t)
    assert loops[0].ticks == loops[1].ticks == 3
    for cl in loops:
        cl.close()


def test_tick_hold_is_the_public_calls_in_order(pkg):
    m, dt = 4, 0.01
    dyn, q = sj.DYN["single"], list(lq.Q["single"])
    plant = [v * s for v, s in zip(dyn, (1.1, 0.9, 1.05, 1.0, 1.2, 1.0, 0.8, 1.0, 1.0))]     # the plants differ from the model
    qf = [10.0 * v for v in q]
    cl = pkg.ClosedLoop(pkg.default_params(), HOLD_B, dtype=torch.float64, device=0)
    twin = pkg.ClosedLoop(pkg.default_params(), HOLD_B, dtype=torch.float64, device=0)
    for c in (cl, twin):
        c.set_state(_hold_states())
    o, s = twin.opts[0], twin.sims[0]
    for t in range(2):
        cl.tick_hold(dyn, m, q, lq.R, dt=dt, plant_dyn=plant, terminal=qf)
        # by hand on the twin's solver and plant
        x0 = s.get_state()
        r = o.step(x0, dyn, 0.0, want_predicted=False)
        u_nom = r.u[:m].clone()
        xs_nom = pkg.sim_rollout_states(dyn, dt, x0, u_nom)["xs"]
        K = pkg.sim_lqr(dyn, dt, x0, u_nom, xs_nom, q, lq.R, terminal=qf, want="K")["K"]
        xs, us = s.rollout_feedback(plant, dt, u_nom, K, x0, xs_nom, u_limit=cl.u_limit)
        z = o.get_solution(HOLD_B)
        zu = z[o.dim - o.N:].clone()
        z[o.dim - o.N:] = torch.cat([zu[m - 1:], zu[-1:].expand(m - 1, HOLD_B)])
        o.set_previous_solution(z)
        same_bits(cl.state(), s.get_state(), "the plants' states after hold %d" % t)
        same_bits(cl.controls(), r.u, "the plan of hold %d" % t)
        warm = cl.opts[0].get_solution(HOLD_B)
        same_bits(warm, z, "the warm start after hold %d" % t)
        # the next step's u_prev is the warm start's first control: the plan's u_{m-1}; its guess starts from u_m
        same_bits(warm[o.dim - o.N], r.u[m - 1], "u_prev of the next step")
        same_bits(warm[o.dim - o.N + 1], r.u[m], "the next step's first guess")
        assert not torch.equal(us, u_nom)                                       # the feedback did act: the plants are not the model
    assert cl.ticks == 2 * m and torch.isfinite(cl.state()).all()
    for bad in (0, cl.opts[0].N + 1):
        with pytest.raises(ValueError):
            cl.tick_hold(dyn, bad, q, lq.R)
    for c in (cl, twin):
        c.close()


def test_tick_hold_in_two_ranges_is_one_range(pkg):
    """per-problem plants and a tensor terminal cost, split over two column ranges with a stream each: the same bits"""
    m, q = 3, list(lq.Q["single"])
    dyn = sj.DYN["single"]
    plant = Tn(np.array(dyn)[:, None] * np.random.default_rng(5).uniform(0.9, 1.1, (len(dyn), HOLD_B)))
    PT = Tn(lq.terminal_costs("single", HOLD_B))
    loops = [pkg.ClosedLoop(pkg.default_params(), HOLD_B, dtype=torch.float64, device=0, ranges=n) for n in (1, 2)]
    for cl in loops:
        cl.set_state(_hold_states())
    for t in range(2):
        for cl in loops:
            cl.tick_hold(dyn, m, q, lq.R, plant_dyn=plant, terminal=PT)
        same_bits(loops[0].state(), loops[1].state(), "the plants' states after hold %d" % t)
        same_bits(loops[0].controls(), loops[1].controls(), "the plan of hold %d" % t)
    for cl in loops:
        cl.close()


def test_tick_hold_is_refused_by_feedback_loops(pkg):
    cl = pkg.ClosedLoop(pkg.default_params(), 64, dtype=torch.float64, device=0, feedback=True)
    with pytest.raises(ValueError, match="feedback=True"):
        cl.tick_hold(sj.DYN["single"], 2, list(lq.Q["single"]), lq.R)
    cl.close()
