"""On the GPU: the Rauch-Tung-Striebel smoother over a window in two launches (cpmpc_sim_rts_batch; sim_rts,
WindowEstimator.smooth) against the numpy reference of tests/helpers/sim_rts_ref.py, which tests/test_sim_rts_ref.py pins and
whose inputs it shows to be admissible.  The cases are sim_ekf_ref.CASES as they are, B = 130.

1. fp64 against the reference (np.linalg.solve on the unscaled P-, on the oracle's x- and A): xs_smooth, Ps_smooth, x0_smooth,
   P0_smooth within T 1e-7 of the lane's largest reference entry -- the bound of tests/test_gpu_sim_ekf.py -- and ok all ones.
2. fp32 against the float64 reference ON THE FLOAT INPUTS.  The bound is made per case on the CPU: gap = the distance of the
   reference's float32-algebra run (filter and smoother) from its float64 run (worst lane, relative to the lane's largest entry);
   the kernel may be 8 x gap away, plus the siblings' state bound e = 4 T max(n_sub, 1) eps, relative to max(1, |x|) for the
   states and to the entry's own scale sqrt(P_ii P_jj) for the covariances, carried through the backward recursion entry by
   entry by the reach the helper returns: entry (t, i) of xs_smooth may be e reach_x[t, i] further away, entry (t, i, j) of
   Ps_smooth e reach_P[t, i, j].  tests/test_sim_rts_ref.py holds the covariances' bound below 1e-2 of the lane's largest
   entry at each index (1e-1 where ticks go unmeasured) on 16 lanes, and this test on all 130, so a P0_smooth of zeros or of
   the wrong sign cannot pass.
3. bitwise and structural properties.  4. dt = 0: the closed form of the CPU test, and x0_smooth against sim_estimate_state with
   the prior.  5. WindowEstimator.smooth()."""
import numpy as np
import pytest

from helpers import batch_position as bp
from helpers import sim_ekf_ref as ek
from helpers import sim_jac_ref as sj
from helpers import sim_rts_ref as rt

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = ek.B
CASES, IDS = ek.CASES, ek.IDS
DTYPES = [torch.float64, torch.float32]
FILTER = ("x_final", "P_final", "xs", "nis")
SMOOTH = ("xs_smooth", "Ps_smooth", "x0_smooth", "P0_smooth")
OUTS = SMOOTH + ("ok",) + FILTER


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    assert callable(pkg.sim_rts)   # imports the batch module; fails on a tree without the call
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1


def Tn(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _eps(dtype):
    return float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)


_TENSORS = {}


def tensors(orc, case, dtype, nb=B):
    """-> the positional arguments of sim_rts after dt (state, cov, u, y, weights), its keywords, the parameters, and the
    case's arrays as the tensors hold them (what the float64 reference of the fp32 test runs on).  Made once; nobody writes."""
    key = (case, dtype, nb)
    if key in _TENSORS:
        return _TENSORS[key]
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
    _TENSORS[key] = ((x0, P0, u, y, [float(v) for v in i["w"]]), kw, params, held)
    return _TENSORS[key]


def call(pkg, orc, case, dtype, want=OUTS, nb=B, **over):
    args, kw, params, _ = tensors(orc, case, dtype, nb)
    return pkg.sim_rts(params, case[1], *args, want=want, **dict(kw, **over))


def lane_scale(ref):
    return np.abs(ref).max(axis=tuple(range(ref.ndim - 1)))


def lane_dist(got, ref):
    """per lane: max |got - ref| relative to the lane's max |ref|; a lane whose reference is all zero must be all zero"""
    ax = tuple(range(ref.ndim - 1))
    d, s = np.abs(got - ref).max(axis=ax), np.abs(ref).max(axis=ax)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))


def same_bits(a, b, name="output", idx=None):
    msg = bp.first_difference(a, b, 1, idx, name)
    assert msg is None, msg


def lower_symmetric(P0):
    """the symmetric matrix the calls read from P0 [nx, nx, B]: its lower triangle mirrored"""
    low = torch.tril(P0.permute(2, 0, 1))
    return (low + torch.tril(low, -1).transpose(1, 2)).permute(1, 2, 0).contiguous()


# ---- 1. fp64 against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp64_matches_the_reference(pkg, orc, case):
    nt = case[2]
    ref = rt.reference(orc, case)
    res = call(pkg, orc, case, torch.float64)
    got = {n: N_(res[n]) for n in SMOOTH}
    assert all(np.isfinite(v).all() for v in got.values())
    errs = {n: lane_dist(got[n], ref[n]).max() for n in SMOOTH}
    moved = ref["x0_smooth"] - ek.inputs(orc, case)["x0"]
    moved = np.abs(moved - 2 * np.pi * np.round(moved / (2 * np.pi))).max()          # a pole angle may have gone round
    print("rts fp64 %s against the reference, worst lane of its largest entry: %s (bound %.0e); x0_smooth is up to %.1e "
          "from x0; ok %d / %d" % (IDS[CASES.index(case)], "  ".join("%s %.2e" % kv for kv in errs.items()),
                                                      nt * 1e-7, moved, int(res["ok"].sum()), B))
    assert (ref["ok"] == 1).all() and (res["ok"] == 1).all()
    assert max(errs.values()) <= nt * 1e-7


# ---- 2. fp32 against the float64 reference --------------------------------------------------------------------------------
def _limit(kind):
    """what the covariances' bound may be of the lane's largest entry: 1e-2, and 1e-1 where ticks go unmeasured ("w0", and the
    lanes of "tw" whose tick weights are mostly exact zeros): there P^s - P- is an exact zero and the reach, which adds the
    errors of P^s and P- as if independent, overstates (tests/test_sim_rts_ref.py)"""
    return 1e-1 if kind in ("w0", "tw") else 1e-2


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_within_eight_times_the_float32_algebras_gap(pkg, orc, case):
    model, dt, nt, kind = case
    _, _, _, held = tensors(orc, case, torch.float32)
    ref = rt.reference(orc, case, arrays=held, key="f32")
    r32 = rt.reference(orc, case, arrays=held, key="f32", dtype=np.float32)
    res = call(pkg, orc, case, torch.float32)
    got = {n: N_(res[n]) for n in SMOOTH}
    assert all(np.isfinite(v).all() for v in got.values()) and (res["ok"] == 1).all()
    n_sub, eps = max(len(sj.sub_steps(dt)), 1), _eps(torch.float32)
    state = 4 * nt * n_sub * eps
    reach = dict(xs_smooth=ref["reach_x"], x0_smooth=ref["reach_x"][0], Ps_smooth=ref["reach_P"], P0_smooth=ref["reach_P"][0])
    ok = True
    for name in SMOOTH:
        gap = lane_dist(r32[name], ref[name]).max()
        bound = 8 * gap * lane_scale(ref[name]) + state * reach[name]         # per entry, absolute
        err = np.abs(got[name] - ref[name])
        print("rts fp32 %s %s: float32-algebra gap %.2e, kernel's error %.2e of the lane's largest entry, error / bound %.3f; "
              "the bound is at most %.2e of the lane's largest entry" % (
                  IDS[CASES.index(case)], name, gap, lane_dist(got[name], ref[name]).max(), (err / bound).max(),
                  (bound / lane_scale(ref[name])).max()))
        ok = ok and bool((err <= bound).all())
        if name in ("Ps_smooth", "P0_smooth"):                # the bound tells a right covariance from a wrong one, on every lane
            assert (bound / lane_scale(ref[name])).max() <= _limit(kind), name
    assert ok


# ---- 3. bitwise and structural --------------------------------------------------------------------------------------------
STRUCT = [c for c in CASES if c[1] == 0.0105 and c[2] == 5 and c[3] in (None, "dyn", "tw")]
STRUCT_IDS = ["%s-%g-%d-%s" % c for c in STRUCT]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_outputs_are_the_filters_and_do_not_depend_on_each_other(pkg, orc, case, dtype):
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, P0, u, y, w = args
    before = [a.clone() for a in args[:4]]
    every = call(pkg, orc, case, dtype)
    again = call(pkg, orc, case, dtype)
    flt = pkg.sim_ekf(params, case[1], *args, want=FILTER, **kw)
    for name in FILTER:
        same_bits(flt[name], every[name], name + " against sim_ekf")
    for name in OUTS:
        same_bits(every[name], again[name], name + " of a second call")
        same_bits(every[name], call(pkg, orc, case, dtype, want=name)[name], name + " alone")
    pair = call(pkg, orc, case, dtype, want=("Ps_smooth", "nis"))
    same_bits(every["Ps_smooth"], pair["Ps_smooth"], "Ps_smooth of a pair")
    same_bits(every["nis"], pair["nis"], "nis of a pair")
    same_bits(every["xs_smooth"][-1], every["x_final"], "xs_smooth[T]")
    same_bits(every["Ps_smooth"][-1], every["P_final"], "Ps_smooth[T]")
    same_bits(every["xs_smooth"][0], every["x0_smooth"], "xs_smooth[0]")
    same_bits(every["Ps_smooth"][0], every["P0_smooth"], "Ps_smooth[0]")
    Ps = every["Ps_smooth"]
    assert torch.equal(Ps, Ps.transpose(1, 2))                                # exactly symmetric
    assert every["ok"].dtype == torch.int32 and (every["ok"] == 1).all()
    assert not torch.equal(every["xs_smooth"][1:-1], every["xs"][:-1])        # smoothing acts
    # a caller's workspace, larger than needed and full of NaNs, against the allocated one
    rows = pkg.capi.load().cpmpc_sim_rts_work_rows(0 if case[0] == "single" else 1, case[2])
    work = torch.full((rows + 3, B), float("nan"), dtype=dtype, device=DEV)
    mine = call(pkg, orc, case, dtype, work=work)
    for name in OUTS:
        same_bits(every[name], mine[name], name + " with a caller's workspace")
    assert torch.isnan(work[rows:]).all() and not torch.isnan(work[:rows]).any()      # its rows, and no more, are written
    with pytest.raises(ValueError):
        call(pkg, orc, case, dtype, work=work[:rows - 1])
    for a, b in zip(args[:4], before):
        assert torch.equal(a, b)
    # only P0's lower triangle is read: garbage above the diagonal changes nothing
    junk = P0.clone()
    iu = np.triu_indices(P0.shape[0], 1)
    junk[iu[0], iu[1]] = float("nan")
    got = pkg.sim_rts(params, case[1], x0, junk, u, y, w, want=OUTS, **kw)
    for name in OUTS:
        same_bits(every[name], got[name], name + " with NaNs above P0's diagonal")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_nothing_measured_leaves_the_filtered_values(pkg, orc, case, dtype):
    """weights 0, or every tick weight 0: P^s - P- and x^s - x- are exact zeros, so every smoothed value is the filtered one"""
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, P0, u, y, w = args
    nt = case[2]
    zero_w = pkg.sim_rts(params, case[1], x0, P0, u, None, [0.0] * len(w), want=OUTS, **dict(kw, tick_weights=None))
    zero_t = pkg.sim_rts(params, case[1], x0, P0, u, y, w, want=OUTS, **dict(kw, tick_weights=torch.zeros_like(u)))
    # the filtered covariances of every index: the filter a tick at a time (bitwise the window's, tests/test_gpu_sim_ekf.py)
    covs, x, P = [lower_symmetric(P0)], x0, P0
    for t in range(nt):
        step = pkg.sim_ekf(params, case[1], x, P, u[t:t + 1].contiguous(), None, [0.0] * len(w), **dict(kw, tick_weights=None))
        x, P = step["x_final"], step["P_final"]
        covs.append(P)
    covs = torch.stack(covs)
    for name, got in (("weights 0", zero_w), ("tick weights 0", zero_t)):
        assert torch.equal(got["xs_smooth"][1:], got["xs"]), name
        assert torch.equal(got["xs_smooth"][0], x0) and torch.equal(got["x0_smooth"], x0), name
        assert torch.equal(got["Ps_smooth"], covs) and torch.equal(got["P0_smooth"], covs[0]), name
        assert (got["ok"] == 1).all() and (got["nis"] == 0).all(), name


def _arranged(pkg, orc, case, dtype, idx):
    """the case's call on the lanes idx (a permutation or a prefix), every output"""
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, P0, u, y, w = args
    kw = dict(kw)
    for name in ("fext", "tick_weights"):
        if name in kw:
            kw[name] = bp.take(kw[name], idx)
    prm = bp.take(params, idx) if isinstance(params, torch.Tensor) else params
    return pkg.sim_rts(prm, case[1], bp.take(x0, idx), bp.take(P0, idx), bp.take(u, idx), bp.take(y, idx), w, want=OUTS, **kw)


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
    got = pkg.sim_rts(params, case[1], x0, P0, u, bad, w, want=OUTS, **kw)
    others = np.array([b for b in range(B) if b != lane], dtype=np.int64)
    for name in OUTS:
        same_bits(bp.take(clean[name], others), bp.take(got[name], others), name)
    assert torch.isnan(got["xs_smooth"][:, :, lane]).any() and int(got["ok"][lane]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT[:2], ids=STRUCT_IDS[:2])
def test_a_known_start_falls_back_to_the_filtered_values(pkg, orc, case, dtype):
    """P0 = 0 on some lanes: the first tick's P- = diag(q) is not positive definite, that tick takes G = 0 -- ok is 0 there and
    index 0, the index behind the failing tick, is smoothed = filtered; the later indices are finite, the other lanes untouched"""
    args, kw, params, _ = tensors(orc, case, dtype)
    x0, P0, u, y, w = args
    clean = call(pkg, orc, case, dtype)
    lanes = np.array([0, 5, 63, 64, 129], dtype=np.int64)
    known = P0.clone()
    known[:, :, lanes] = 0.0
    got = pkg.sim_rts(params, case[1], x0, known, u, y, w, want=OUTS, **kw)
    others = np.array([b for b in range(B) if b not in lanes], dtype=np.int64)
    for name in OUTS:
        same_bits(bp.take(clean[name], others), bp.take(got[name], others), name)
    sel = bp.take
    assert (sel(got["ok"], lanes) == 0).all() and (sel(got["ok"], others) == 1).all()
    assert torch.equal(sel(got["xs_smooth"][0], lanes), sel(x0, lanes)) and torch.equal(sel(got["x0_smooth"], lanes), sel(x0, lanes))
    assert (sel(got["Ps_smooth"][0], lanes) == 0).all() and (sel(got["P0_smooth"], lanes) == 0).all()
    assert torch.isfinite(sel(got["xs_smooth"], lanes)).all() and torch.isfinite(sel(got["Ps_smooth"], lanes)).all()
    assert not torch.equal(sel(got["xs_smooth"][1:-1], lanes), sel(got["xs"][:-1], lanes))       # the later ticks do smooth


# ---- 4. dt = 0 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("weighted", [False, True])
def test_constant_state_closed_form_at_every_index(pkg, model, weighted, dtype):
    """dt = 0, diagonal P0, q = 0: the smoothed state at EVERY index is the closed form's mean and variances, with the bounds of
    tests/test_sim_rts_ref.py: 8 (T + 1) eps of the sums -- for a variance of index t the largest term that enters, the
    filtered variance of that index (P0_ii at index 0) -- plus T eps pi on the pole angles, compared modulo 2 pi.  x0_smooth is also sim_estimate_state's x0 with prior = x0, prior_info = P0^-1 (one
    Gauss-Newton step of a linear fit), within the same bound."""
    nx, nt, nb = sj.NX[model], 6, 65
    rng = np.random.default_rng(3)
    x0 = Tn(rng.uniform(-0.5, 0.5, (nx, nb)), dtype)
    p0 = Tn(rng.uniform(0.5, 2.0, (nx, nb)) * ek.prior_covariance(model)[:, None], dtype)
    ys = (x0[None] + Tn(rng.uniform(-0.05, 0.05, (nt, nx, nb)), dtype)).contiguous()
    w = ek.weights(model)
    w[-1] = 25.0
    om = Tn(rng.uniform(0.0, 2.0, (nt, nb)), dtype) if weighted else None
    P0 = torch.diag_embed(p0.t()).permute(1, 2, 0).contiguous()
    u = Tn(rng.uniform(-20, 20, (nt, nb)), dtype)
    wl = [float(v) for v in w]
    got = pkg.sim_rts(sj.DYN[model], 0.0, x0, P0, u, ys, wl, tick_weights=om, model=model, want=("xs_smooth", "Ps_smooth", "ok"))
    est = pkg.sim_estimate_state(sj.DYN[model], 0.0, x0, u, ys, iterations=1, weights=wl, tick_weights=om, prior=x0,
                                 prior_info=(1.0 / p0).contiguous(), model=model)
    xs, Ps, fit = N_(got["xs_smooth"]), N_(got["Ps_smooth"]), N_(est["x0"])
    assert (got["ok"] == 1).all()
    tol = 8 * (nt + 1) * _eps(dtype)
    wrap = np.array([nt * _eps(dtype) * np.pi if 1 <= i < nx // 2 else 0.0 for i in range(nx)])
    worst_p = worst_x = worst_off = worst_fit = 0.0
    for b in range(nb):
        o = None if om is None else N_(om)[:, b]
        mean, var = ek.constant_state(N_(x0)[:, b], N_(p0)[:, b], N_(ys)[:, :, b], w, o)
        mag, _ = ek.constant_state(np.abs(N_(x0)[:, b]), N_(p0)[:, b], np.abs(N_(ys)[:, :, b]), w, o)
        filtered = rt.filtered_variances(N_(p0)[:, b], w, o, nt)                  # [T+1, nx]: index 0 is P0_ii

        def angle_diff(d):
            d = d.copy()
            d[1:nx // 2] -= 2 * np.pi * np.round(d[1:nx // 2] / (2 * np.pi))
            return np.abs(d)

        for t in range(nt + 1):
            P = Ps[t, :, :, b]
            worst_p = max(worst_p, (np.abs(np.diag(P) - var) / (tol * filtered[t])).max())
            worst_off = max(worst_off, np.abs(P - np.diag(np.diag(P))).max() / (tol * filtered[t].max()))
            worst_x = max(worst_x, (angle_diff(xs[t, :, b] - mean) / (tol * mag + wrap)).max())
        worst_fit = max(worst_fit, (angle_diff(xs[0, :, b] - fit[:, b]) / (tol * mag + wrap)).max())
    print("rts %s dt = 0 %s weighted=%s: worst distance from the closed form / bound: P %.3f (off the diagonal %.3f), x %.3f; "
          "x0_smooth from sim_estimate_state's x0 / bound %.3f" % (model, dtype, weighted, worst_p, worst_off, worst_x, worst_fit))
    assert worst_p <= 1.0 and worst_off <= 1.0 and worst_x <= 1.0 and worst_fit <= 1.0


# ---- 5. WindowEstimator.smooth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_window_estimator_smooth_is_sim_rts_on_what_it_holds(pkg, orc, dtype):
    """window 4, 7 ticks pushed (so the rolling prior has moved three times): smooth() is a direct sim_rts call on held() from
    the prior, bit for bit, leaves the estimator's tensors alone, and raises without prior_cov"""
    case = ("single", 0.0105, 5, None)
    model, dt = case[0], case[1]
    i = ek.inputs(orc, case)
    nx, window, ticks = sj.NX[model], 4, 7
    rng = np.random.default_rng(17)
    us = Tn(rng.uniform(-20, 20, (ticks, B)), dtype)
    ys = Tn(i["x0"][None] + rng.uniform(-0.05, 0.05, (ticks, nx, B)), dtype)
    w, q = [float(v) for v in ek.weights(model)], [float(v) for v in ek.process_noise(model)]
    est = pkg.WindowEstimator(sj.DYN[model], dt, B, window, state=Tn(i["x0"], dtype), dtype=dtype, model=model, weights=w,
                              prior_cov=Tn(i["P0"], dtype), process_noise=q)
    plain = pkg.WindowEstimator(sj.DYN[model], dt, B, window, state=Tn(i["x0"], dtype), dtype=dtype, model=model, weights=w)
    for t in range(ticks):
        tw = None if t != 5 else torch.zeros(B, dtype=dtype, device=DEV)
        for e in (est, plain):
            e.push(us[t], ys[t], tw)
    names = ("x0", "u", "y", "w", "prior_mean", "prior_cov")
    before = {n: getattr(est, n).clone() for n in names}
    ids = {n: getattr(est, n).data_ptr() for n in names}
    got = est.smooth(want=OUTS)
    _, u, y, tw = est.held()
    direct = pkg.sim_rts(sj.DYN[model], dt, est.prior_mean, est.prior_cov, u, y, w, process_noise=q, tick_weights=tw, model=model,
                         want=OUTS)
    for name in OUTS:
        same_bits(direct[name], got[name], name)
    assert tuple(got["xs_smooth"].shape) == (window + 1, nx, B) and (got["ok"] == 1).all()
    assert sorted(est.smooth().keys()) == ["P0_smooth", "x0_smooth", "xs_smooth"]
    for n in names:
        assert getattr(est, n).data_ptr() == ids[n] and torch.equal(getattr(est, n), before[n]), n
    assert est.count == window
    with pytest.raises(ValueError):
        plain.smooth()
