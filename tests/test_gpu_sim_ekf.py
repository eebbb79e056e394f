"""On the GPU: the extended Kalman filter over a window in one launch (cpmpc_sim_ekf_batch; sim_ekf, StateFilter,
WindowEstimator(prior_cov=...)) against the numpy reference of tests/helpers/sim_ekf_ref.py, which tests/test_sim_ekf_ref.py
pins and whose inputs it shows to be admissible.

1. fp64 against the reference (the joint update in the Joseph form on the oracle's x- and A): where nothing is measured the
   states within T 1e-12; P, the filtered states and nis within T 1e-7 of the lane's largest reference entry -- the bounds of
   tests/test_gpu_sim_rollout_gn_x0.py's test 4.
2. fp32 against the float64 reference ON THE FLOAT INPUTS.  The bound is made per case on the CPU: gap = the distance of the
   reference's float32-algebra run from its float64 run (worst lane, relative to the lane's largest entry); the kernel may be
   8 x gap away (another summation order, the sequential form) plus the siblings' state bound 4 T max(n_sub, 1) eps max(1, |x|),
   which covers what a float x- and A add: the reference's float32 run takes both from float64.  For nis that state bound
   counts through the innovations, times |d nis / d x-| = |2 S^-1 nu| (ten to a few hundred here: nu ~ 0.02, s ~ 2e-4).
3. bitwise and structural properties.  4. dt = 0: the closed form of the CPU test.  5. StateFilter against its CPU twin.
6. WindowEstimator(prior_cov=...) against its CPU twin, the dt = 0 full-information identity, and prior_cov=None as before."""
import numpy as np
import pytest

from helpers import batch_position as bp
from helpers import sim_ekf_ref as ek
from helpers import sim_jac_ref as sj
from helpers import sim_rollout_gn_x0_ref as gx
from helpers import sim_rollout_ref as sr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = ek.B
CASES, IDS = ek.CASES, ek.IDS
DTYPES = [torch.float64, torch.float32]
OUTS = ("x_final", "P_final", "xs", "nis")


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1
    assert callable(pkg.sim_ekf)   # imports the batch module; fails on a tree without the call


def Tn(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _eps(dtype):
    return float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)


def tensors(orc, case, dtype, nb=B):
    """-> the positional arguments of sim_ekf after dt (state, cov, u, y, weights), its keywords, the parameters, and the
    case's arrays as the tensors hold them (what the float64 reference of the fp32 test runs on)"""
    i = ek.inputs(orc, case, nb)
    kw = dict(model=case[0], process_noise=[float(v) for v in i["q"]])
    held = dict(i)
    if case[3] == "shared":
        kw.update(f_base=ek.SHARED_F[0], f_mass=ek.SHARED_F[1])
    elif case[3] == "per":
        kw.update(fext=Tn(i["f"], dtype))
        held["f"] = N_(kw["fext"])
    if i["om"] is not None:
        kw["tick_weights"] = Tn(i["om"], dtype)
        held["om"] = N_(kw["tick_weights"])
    params = Tn(i["prm"], dtype) if i["prm"].ndim == 2 else [float(v) for v in i["prm"]]
    if i["prm"].ndim == 2:
        held["prm"] = N_(params)
    x0, P0, u, y = Tn(i["x0"], dtype), Tn(i["P0"], dtype), Tn(i["us"], dtype), Tn(i["ys"], dtype)
    held.update(x0=N_(x0), P0=N_(P0), us=N_(u), ys=N_(y))
    return (x0, P0, u, y, [float(v) for v in i["w"]]), kw, params, held


def call(pkg, orc, case, dtype, want=OUTS, nb=B, **over):
    args, kw, params, _ = tensors(orc, case, dtype, nb)
    kw.update(over)
    return pkg.sim_ekf(params, case[1], *args, want=want, **kw)


def lane_dist(got, ref):
    """per lane: max |got - ref| relative to the lane's max |ref|; a lane whose reference is all zero must be all zero"""
    ax = tuple(range(ref.ndim - 1))
    d, s = (np.abs(got - ref).max(axis=ax), np.abs(ref).max(axis=ax)) if ax else (np.abs(got - ref), np.abs(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))


def same_bits(a, b, name="output", idx=None):
    msg = bp.first_difference(a, b, 1, idx, name)
    assert msg is None, msg


# ---- 1. fp64 against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp64_matches_the_reference(pkg, orc, case):
    model, dt, nt, kind = case
    ref = ek.reference(orc, case)
    got = {n: N_(v) for n, v in call(pkg, orc, case, torch.float64).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    errs = dict(x_final=lane_dist(got["x_final"], ref["x_final"]).max(), xs=lane_dist(got["xs"], ref["xs"]).max(),
                P_final=lane_dist(got["P_final"], ref["P_final"]).max(), nis=lane_dist(got["nis"], ref["nis"]).max())
    ex = np.abs(got["xs"] - ref["xs"]).max()
    print("ekf fp64 %s against the reference, worst lane of its largest entry: %s (bound %.0e); |xs - ref| %.2e%s" % (
        IDS[CASES.index(case)], "  ".join("%s %.2e" % kv for kv in errs.items()), nt * 1e-7, ex,
        " (bound %.0e: nothing is measured)" % (nt * 1e-12) if kind == "w0" else ""))
    if kind == "w0":
        assert ex <= nt * 1e-12 and (got["nis"] == 0).all()
    assert max(errs.values()) <= nt * 1e-7


# ---- 2. fp32 against the float64 reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_within_eight_times_the_float32_algebras_gap(pkg, orc, case):
    model, dt, nt, kind = case
    _, _, _, held = tensors(orc, case, torch.float32)
    ref = ek.reference(orc, case, arrays=held)
    r32 = ek.reference(orc, case, arrays=held, dtype=np.float32)
    got = {n: N_(v) for n, v in call(pkg, orc, case, torch.float32).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    n_sub, eps = max(len(sj.sub_steps(dt)), 1), _eps(torch.float32)
    state = 4 * nt * n_sub * eps           # the siblings' state bound, relative to max(1, |x|)
    ok = True
    for name in ("x_final", "xs", "P_final", "nis"):
        gap = lane_dist(r32[name], ref[name]).max()
        if name in ("x_final", "xs"):
            ax = tuple(range(ref[name].ndim - 1))
            scale = np.maximum(1.0, np.abs(ref[name])).max(axis=ax) / np.abs(ref[name]).max(axis=ax)
            bound = 8 * gap + state * scale                  # per lane, relative to the lane's largest entry
        elif name == "nis":
            # nis reads the predicted states through the innovations: d nis / d x- = -2 S^-1 nu, so the state bound reaches it
            # as state * sum_t |2 S^-1 nu| . max(1, |x-|) (the reference's nis_dx), here relative to the lane's nis
            reach = np.divide(ref["nis_dx"], np.abs(ref["nis"]), out=np.zeros(B), where=ref["nis"] != 0)
            bound = 8 * gap + state * (1.0 + reach)
        else:
            bound = 8 * gap + state
        err = lane_dist(got[name], ref[name])
        print("ekf fp32 %s %s: float32-algebra gap %.2e, kernel's error %.2e, error / bound %.3f" % (
            IDS[CASES.index(case)], name, gap, err.max(), (err / bound).max() if np.all(bound > 0) else float(err.max() > 0)))
        ok = ok and bool((err <= bound).all())
    assert ok


# ---- 3. bitwise and structural --------------------------------------------------------------------------------------------
STRUCT = [c for c in CASES if c[1] == 0.0105 and c[2] == 5 and c[3] in (None, "dyn", "tw")]
STRUCT_IDS = ["%s-%g-%d-%s" % c for c in STRUCT]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_outputs_do_not_depend_on_each_other_and_the_inputs_are_read_only(pkg, orc, case, dtype):
    args, kw, params, _ = tensors(orc, case, dtype)
    before = [a.clone() for a in args[:4]]
    every = call(pkg, orc, case, dtype)
    again = call(pkg, orc, case, dtype)
    for name in OUTS:
        same_bits(every[name], again[name], name)
        same_bits(every[name], call(pkg, orc, case, dtype, want=name)[name], name + " alone")
    pair = call(pkg, orc, case, dtype, want=("P_final", "nis"))
    same_bits(every["P_final"], pair["P_final"], "P_final of a pair")
    same_bits(every["nis"], pair["nis"], "nis of a pair")
    P = every["P_final"]
    assert torch.equal(P, P.transpose(0, 1))                                  # exactly symmetric
    same_bits(every["xs"][-1], every["x_final"], "xs[-1]")
    for a, b in zip(args[:4], before):
        assert torch.equal(a, b)
    # only P0's lower triangle is read: garbage above the diagonal changes nothing
    x0, P0, u, y, w = args
    junk = P0.clone()
    iu = np.triu_indices(P0.shape[0], 1)
    junk[iu[0], iu[1]] = float("nan")
    got = pkg.sim_ekf(params, case[1], x0, junk, u, y, w, want=OUTS, **kw)
    for name in OUTS:
        same_bits(every[name], got[name], name + " with NaNs above P0's diagonal")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_nothing_measured_is_the_plain_rollout(pkg, orc, case, dtype):
    """weights 0, or every tick weight 0: x_final and xs are sim_rollout_states', bit for bit"""
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, P0, u, y, w = args
    plant = {k: v for k, v in kw.items() if k in ("model", "fext", "f_base", "f_mass")}
    roll = pkg.sim_rollout_states(params, case[1], x0, u, want=("xs", "x_final"), **plant)
    zero_w = pkg.sim_ekf(params, case[1], x0, P0, u, None, [0.0] * len(w), want=OUTS, **dict(kw, tick_weights=None))
    zero_t = pkg.sim_ekf(params, case[1], x0, P0, u, y, w, want=OUTS, **dict(kw, tick_weights=torch.zeros_like(u)))
    for name, got in (("weights 0", zero_w), ("tick weights 0", zero_t)):
        same_bits(roll["xs"], got["xs"], "xs, " + name)
        same_bits(roll["x_final"], got["x_final"], "x_final, " + name)
        assert (got["nis"] == 0).all()
    same_bits(zero_w["P_final"], zero_t["P_final"], "P_final")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model,dt,nt", [("single", 0.0105, 5), ("double", 0.0105, 5), ("double", 0.001, 8), ("single", 0.0, 3)])
def test_pure_prediction_of_the_identity_is_phi_phi_transposed(pkg, orc, model, dt, nt, dtype):
    """weights 0, q = 0, P0 = I: P_final = Phi Phi^T with sim_rollout_gauss_newton_x0's Phi_final, within 5j's eps-propagation
    bound: each factor carries f = 4 (NX + 1) T max(n_sub, 1) eps of the product of the ticks' |A|, the product NX T eps more."""
    case = (model, dt, nt, None)
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, _, u, _, _ = args
    nx = sj.NX[model]
    eye = torch.eye(nx, dtype=dtype, device=DEV)[:, :, None].repeat(1, 1, B).contiguous()
    got = pkg.sim_ekf(params, dt, x0, eye, u, None, [0.0] * nx, process_noise=None, model=model, want="P_final")["P_final"]
    Phi = N_(pkg.sim_rollout_gauss_newton_x0(params, dt, x0, u, None, model=model, want="Phi_final")["Phi_final"])
    xs = pkg.sim_rollout_states(params, dt, x0, u, model=model)["xs"]
    hat = np.tile(np.eye(nx)[:, :, None], (1, 1, B))
    for t in range(nt):
        xt = x0 if t == 0 else xs[t - 1].contiguous()
        A = N_(pkg.sim_step_jacobian(params, dt, xt, u[t].contiguous(), model=model, want="A")["A"])
        hat = np.einsum("rcb,cjb->rjb", np.abs(A), hat)
    n_sub, eps = max(len(sj.sub_steps(dt)), 1), _eps(dtype)
    bound = (2 * 4 * (nx + 1) * nt * n_sub * eps + 4 * nx * nt * eps) * np.einsum("jqb,kqb->jkb", hat, hat)
    d = np.abs(N_(got) - np.einsum("jqb,kqb->jkb", Phi, Phi))
    print("ekf %s dt=%g T=%d %s: |P_final - Phi Phi^T| / bound %.3f" % (model, dt, nt, dtype, (d[bound > 0] / bound[bound > 0]).max()))
    assert (d <= bound).all()
    if dt == 0.0:
        assert torch.equal(got, eye)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in CASES if c[2] == 2 or (c[2] == 5 and c[3] == "tw")],
                         ids=lambda c: "%s-%g-%d-%s" % c)
def test_two_ticks_are_two_chained_one_tick_calls(pkg, orc, case, dtype):
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, P0, u, y, w = args
    whole = pkg.sim_ekf(params, case[1], x0, P0, u[:2].contiguous(), y[:2].contiguous(), w,
                        **dict(kw, tick_weights=kw["tick_weights"][:2].contiguous() if "tick_weights" in kw else None))
    x, P = x0, P0
    for t in range(2):
        tw = kw["tick_weights"][t:t + 1].contiguous() if "tick_weights" in kw else None
        step = pkg.sim_ekf(params, case[1], x, P, u[t:t + 1].contiguous(), y[t:t + 1].contiguous(), w,
                           **dict(kw, tick_weights=tw))
        x, P = step["x_final"], step["P_final"]
    same_bits(whole["x_final"], x, "x_final")
    same_bits(whole["P_final"], P, "P_final")


def _arranged(pkg, orc, case, dtype, idx):
    """the case's call on the lanes idx (a permutation or a prefix), every output"""
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, P0, u, y, w = args
    kw = dict(kw)
    for name in ("fext", "tick_weights"):
        if name in kw:
            kw[name] = bp.take(kw[name], idx)
    prm = bp.take(params, idx) if isinstance(params, torch.Tensor) else params
    return pkg.sim_ekf(prm, case[1], bp.take(x0, idx), bp.take(P0, idx), bp.take(u, idx), bp.take(y, idx), w, want=OUTS, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_a_lanes_bits_do_not_depend_on_its_place_in_the_batch(pkg, orc, case, dtype):
    """the same lanes reversed, and as prefixes that end alone, below, on and above a wave boundary"""
    natural = call(pkg, orc, case, dtype)
    rev = bp.permutations(B, 7)["reverse"]
    got = _arranged(pkg, orc, case, dtype, rev)
    for name in OUTS:
        same_bits(natural[name], bp.put_back(got[name], rev), name + " reversed", rev)
    for nb in (1, 63, 64, 65):
        idx = np.arange(nb, dtype=np.int64)
        got = _arranged(pkg, orc, case, dtype, idx)
        for name in OUTS:
            same_bits(bp.take(natural[name], idx), got[name], "%s of the first %d" % (name, nb))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT[:2], ids=STRUCT_IDS[:2])
def test_a_nan_measurement_stays_in_its_lane(pkg, orc, case, dtype):
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, P0, u, y, w = args
    clean = call(pkg, orc, case, dtype)
    bad = y.clone()
    lane = 70
    bad[1, 0, lane] = float("nan")
    got = pkg.sim_ekf(params, case[1], x0, P0, u, bad, w, want=OUTS, **kw)
    others = np.array([b for b in range(B) if b != lane], dtype=np.int64)
    for name in OUTS:
        same_bits(bp.take(clean[name], others), bp.take(got[name], others), name)
    assert torch.isnan(got["x_final"][:, lane]).any() and torch.isnan(got["nis"][lane])


# ---- 4. dt = 0 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("weighted", [False, True])
def test_constant_state_closed_form(pkg, model, weighted, dtype):
    """dt = 0, diagonal P0, q = 0: every state is a scalar filter, P_ii = 1 / (1 / P0_ii + sum_t rho_t) and the matching mean.
    Each of the T updates rounds a handful of times, so both are held to 8 (T + 1) eps of the sums' magnitudes: P_ii's own, and
    for the mean P_ii (|x0_i| / P0_ii + sum_t rho_t |y_t,i|).  A pole angle is wrapped after every tick's update, and the wrap
    sends a negative angle through + 2 pi - 2 pi: one rounding at the size of 2 pi, eps pi, whatever the angle's own size --
    T eps pi more for those, absolutely."""
    nx, nt, nb = sj.NX[model], 6, 65
    rng = np.random.default_rng(3)
    x0 = Tn(rng.uniform(-0.5, 0.5, (nx, nb)), dtype)
    p0 = Tn(rng.uniform(0.5, 2.0, (nx, nb)) * ek.prior_covariance(model)[:, None], dtype)
    ys = (x0[None] + Tn(rng.uniform(-0.05, 0.05, (nt, nx, nb)), dtype)).contiguous()
    w = ek.weights(model)
    w[-1] = 25.0
    om = Tn(rng.uniform(0.0, 2.0, (nt, nb)), dtype) if weighted else None
    P0 = torch.diag_embed(p0.t()).permute(1, 2, 0).contiguous()
    got = pkg.sim_ekf(sj.DYN[model], 0.0, x0, P0, Tn(rng.uniform(-20, 20, (nt, nb)), dtype), ys, [float(v) for v in w],
                      tick_weights=om, model=model)
    P, x = N_(got["P_final"]), N_(got["x_final"])
    off = P.copy()
    off[np.arange(nx), np.arange(nx)] = 0.0
    assert (off == 0).all()
    tol, worst_p, worst_x = 8 * (nt + 1) * _eps(dtype), 0.0, 0.0
    wrap = np.array([nt * _eps(dtype) * np.pi if 1 <= i < nx // 2 else 0.0 for i in range(nx)])
    for b in range(nb):
        o = None if om is None else N_(om)[:, b]
        mean, var = ek.constant_state(N_(x0)[:, b], N_(p0)[:, b], N_(ys)[:, :, b], w, o)
        mag, _ = ek.constant_state(np.abs(N_(x0)[:, b]), N_(p0)[:, b], np.abs(N_(ys)[:, :, b]), w, o)
        worst_p = max(worst_p, (np.abs(np.diag(P[:, :, b]) - var) / (tol * var)).max())
        worst_x = max(worst_x, (np.abs(x[:, b] - mean) / (tol * mag + wrap)).max())
    print("ekf %s dt = 0 %s weighted=%s: worst distance from the closed form / bound: P %.3f, x %.3f" % (
        model, dtype, weighted, worst_p, worst_x))
    assert worst_p <= 1.0 and worst_x <= 1.0


# ---- 5. StateFilter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b", "c"])
def test_state_filter_follows_its_twin(pkg, orc, name):
    """12 ticks, 64 lanes, fp64, positions only with encoder noise: after every push the state is the reference filter's, as
    test 1 holds a window to it (T 1e-7 of the lane's largest entry), and push returns what .state holds."""
    model, _ = gx.EST_CASES[name]
    nx, nb, ticks = sj.NX[model], ek.FILTER_B, ek.FILTER_TICKS
    truth, guess, us = ek.twin_draws(model)
    xs = sr.rollout_batch(orc, model, sj.DYN[model], gx.EST_DT, truth, us)
    ys = xs + np.random.default_rng(37).uniform(-2 * ek.SIGMA, 2 * ek.SIGMA, xs.shape)
    w, q, p0 = ek.weights(model), ek.process_noise(model), ek.prior_covariance(model)
    P0 = np.zeros((nx, nx, nb))
    P0[np.arange(nx), np.arange(nx)] = p0[:, None]
    ref = ek.run_batch(orc, model, sj.DYN[model], gx.EST_DT, guess, P0, us, ys, w, q)
    flt = pkg.StateFilter(sj.DYN[model], gx.EST_DT, nb, Tn(np.tile(p0[:, None], (1, nb))), [float(v) for v in w],
                          [float(v) for v in q], state=Tn(guess), model=model)
    worst = 0.0
    for t in range(ticks):
        out = flt.push(Tn(us[t]), Tn(ys[t]))
        assert out is flt.state and tuple(out.shape) == (nx, nb)
        worst = max(worst, lane_dist(N_(out), ref["xs"][t]).max(), lane_dist(N_(flt.cov), ref["Ps"][t]).max())
    nq = nx // 2
    err0 = np.abs(np.array([gx.wrap_state_diff(model, d) for d in (guess - truth).T])).max(axis=0)
    err = np.abs(np.array([gx.wrap_state_diff(model, d) for d in (N_(flt.state) - xs[-1]).T])).max(axis=0)
    print("StateFilter %s: worst lane from the twin over %d ticks %.2e of its largest entry (bound %.0e); worst |state - truth| "
          "at the start %s, after %s" % (model, ticks, worst, ticks * 1e-7, np.round(err0, 3), np.round(err, 3)))
    assert worst <= ticks * 1e-7
    # the measured positions end nearer the truth than the guess began (0.1): the encoders' +- 0.02 and a tick's drift under
    # a velocity error of 0.2 (0.002) are all that can be left in them
    assert err[:nq].max() < err0[:nq].min() and flt.nis is not None and torch.isfinite(flt.nis).all()


# ---- 6. WindowEstimator with the rolling prior ------------------------------------------------------------------------------
def test_window_estimator_with_the_rolling_prior_follows_its_twin(pkg, orc):
    """fp64, 64 lanes, 12 ticks, window 4, positions only, noise-free, two iterations a tick: the current state is the CPU
    twin's within ten times gx.WINDOW_TWIN_WORST, the bound the plain estimator's test holds it to (there against the truth,
    which the twin reaches; with a prior around a perturbed guess neither does, so here the twin itself is the yardstick)."""
    model, w = gx.EST_CASES["b"]
    nb, ticks, T = ek.WINDOW_B, ek.WINDOW_TICKS, ek.WINDOW_T
    truth, guess, us = ek.twin_draws(model, nb, ticks)
    xs = sr.rollout_batch(orc, model, sj.DYN[model], gx.EST_DT, truth, us)
    p0, q = ek.prior_covariance(model), ek.process_noise(model)
    wv = [v / ek.SIGMA ** 2 for v in w]
    est = pkg.WindowEstimator(sj.DYN[model], gx.EST_DT, nb, T, state=Tn(guess), model=model, weights=wv,
                              prior_cov=Tn(np.tile(p0[:, None], (1, nb))), process_noise=[float(v) for v in q])
    got = np.zeros((ticks,) + truth.shape)
    for t in range(ticks):
        est.push(Tn(us[t]), Tn(xs[t]))
        got[t] = N_(est.estimate(iterations=ek.WINDOW_ITERATIONS))
    worst = 0.0
    for b in range(nb):
        twin = ek.window_prior_estimates(orc, model, sj.DYN[model], gx.EST_DT, guess[:, b], us[:, b], xs[:, :, b], T, wv,
                                         ek.WINDOW_ITERATIONS, prior_cov=np.diag(p0), q=q)
        worst = max(worst, np.abs(np.array([gx.wrap_state_diff(model, d) for d in got[:, :, b] - twin])).max())
    print("WindowEstimator(prior_cov): worst |current state - twin's| over %d lanes and %d ticks %.2e (bound %.1e)" % (
        nb, ticks, worst, 10 * gx.WINDOW_TWIN_WORST))
    assert worst <= 10 * gx.WINDOW_TWIN_WORST


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_estimator_full_information_identity_at_dt_zero(pkg, dtype):
    """dt = 0, window 3, 8 ticks, every state measured, one iteration (the fit is linear): with prior_cov the estimate is the
    closed form over ALL samples pushed so far, without it the mean of the last 3.  Held to 8 (ticks + nx) eps of the magnitudes
    that enter (the guess, the prior mean and the samples, all O(1): their largest, and at least 1)."""
    model, window, ticks, nb = "single", 3, 8, 64
    nx = sj.NX[model]
    rng = np.random.default_rng(5)
    guess = rng.uniform(-0.5, 0.5, (nx, nb))
    ys = guess[None] + rng.uniform(-0.05, 0.05, (ticks, nx, nb))
    us = rng.uniform(-20, 20, (ticks, nb))
    w = [1.0 / ek.SIGMA ** 2] * nx
    p0 = ek.prior_covariance(model)
    kw = dict(state=Tn(guess, dtype), dtype=dtype, model=model, weights=w)
    rolling = pkg.WindowEstimator(sj.DYN[model], 0.0, nb, window, prior_cov=Tn(np.tile(p0[:, None], (1, nb)), dtype), **kw)
    plain = pkg.WindowEstimator(sj.DYN[model], 0.0, nb, window, **kw)
    tol = 8 * (ticks + nx) * _eps(dtype) * max(1.0, np.abs(ys).max())
    worst = 0.0
    for t in range(ticks):
        for e in (rolling, plain):
            e.push(Tn(us[t], dtype), Tn(ys[t], dtype))
        a, b = N_(rolling.estimate(iterations=1)), N_(plain.estimate(iterations=1))
        held = N_(Tn(ys[:t + 1], dtype))
        for lane in range(nb):
            full, _ = ek.constant_state(N_(kw["state"])[:, lane], N_(Tn(p0, dtype)), held[:, :, lane], w)
            worst = max(worst, np.abs(a[:, lane] - full).max(), np.abs(b[:, lane] - held[max(0, t + 1 - window):, :, lane].mean(axis=0)).max())
    print("WindowEstimator dt = 0 %s: worst distance from the closed forms %.2e (bound %.2e)" % (dtype, worst, tol))
    assert worst <= tol


def test_window_estimator_without_prior_cov_is_as_before(pkg, orc):
    model, w = gx.EST_CASES["b"]
    nb, ticks, T = 64, 6, 4
    truth, guess, us = ek.twin_draws(model, nb, ticks)
    xs = sr.rollout_batch(orc, model, sj.DYN[model], gx.EST_DT, truth, us)
    a = pkg.WindowEstimator(sj.DYN[model], gx.EST_DT, nb, T, state=Tn(guess), model=model, weights=w)
    b = pkg.WindowEstimator(sj.DYN[model], gx.EST_DT, nb, T, state=Tn(guess), model=model, weights=w, prior_cov=None,
                            process_noise=None)
    for t in range(ticks):
        for e in (a, b):
            e.push(Tn(us[t]), Tn(xs[t]))
        ra, rb = a.estimate(want_result=True), b.estimate(want_result=True)
        same_bits(ra[0], rb[0], "the current state at tick %d" % t)
        for name in ("x0", "cost", "H"):
            same_bits(ra[1][name], rb[1][name], name)
    assert b.prior_mean is None and b.prior_cov is None
