"""On the GPU: the two passes of an iterative LQR on the plant's tick map, one launch each, and the loop above them
(cpmpc_sim_ilqr_backward_batch, cpmpc_sim_ilqr_forward_batch; sim_ilqr_backward, sim_ilqr_forward, sim_ilqr, BatchSimulator.ilqr)
against the numpy reference of tests/helpers/sim_ilqr_ref.py, which tests/test_sim_ilqr_ref.py pins and whose inputs it shows to
be admissible.  B = 130, sim_lqr_ref's states: lanes at the +-pi cut and beyond the bumpers.

1. fp64 against the reference (the textbook Q_x, Q_u, Q_xx, Q_ux, Q_uu recursion on the oracle's Phi and gamma; the forward pass
   through the oracle's step): K, kff, P0, g0, dV, hmax, and the forward pass's xs and us, within T 1e-7 of the lane's largest
   reference entry; cost within T 1e-7 relative.  A lane whose unclamped control lies within 1e-9 of the limit is left out of the
   K comparison; at most 2 % of the lanes may be.
2. fp32 against the float64 reference ON THE FLOAT INPUTS, the siblings' rule.  Backward: gap = the distance of the reference's
   float32-algebra run from its float64 run (worst lane, relative to the lane's largest entry); the kernel may be 8 x gap away plus
   the state bound 4 T max(n_sub, 1) eps max(1, |x|).  A lane where the float run puts the control on the other side of the limit
   than the reference (a discrete decision) is left out, under the same 2 % cap.  Forward: the state bound carried through the law
   once per tick, as tests/test_gpu_sim_lqr.py carries it, with alpha kff in the control's rounding; the cost's bound follows
   from the states' and controls' by the cost's own derivative plus its summation's rounding.  Every ratio is printed.
3. identities and structure: at its own reference kff and dV are exactly 0 and K, P0 are sim_lqr's BIT FOR BIT (the two kernels
   share the Riccati step's text); without kff, K and limit the forward pass is sim_rollout_states bit for bit; from the nominal start with alpha = 0
   it reproduces the nominal xs, us and cost bit for bit; outputs do not depend on which others are requested; inputs are left
   unchanged; a lane's bits do not depend on its place in the batch; a lane with non-finite data stays in its lane.  (There is no
   gT beside PT, so a window is not chained from its tail: dV and hmax are sums and maxima over the whole window anyway.)
4. dt = 0, the closed form.
5. the loop on the CPU test's 32 lanes, T = 30, dt = 0.01, free and clamped: cost_history never increases; sim_ilqr is the public
   backward and forward calls issued in the loop's order, bit for bit, and there a rejected lane keeps its trajectory bit for bit;
   the controls returned, evaluated by the numpy plant and cost, are within 1e-8 relative of the reference loop's converged cost in
   fp64.  In fp32 the bound is 10 x the worst lane MEASURED on an MI355X against the same converged costs: FP32_SUBOPT below."""
import numpy as np
import pytest

from helpers import batch_position as bp
from helpers import sim_ilqr_ref as il
from helpers import sim_jac_ref as sj
from helpers import sim_lqr_ref as lq

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = il.B
CASES, IDS = il.CASES, il.IDS
DTYPES = [torch.float64, torch.float32]
BW_OUTS = ("K", "kff", "dV", "P0", "g0", "hmax")
FW_OUTS = ("xs", "x_final", "us", "cost")
# the worst lane's relative sub-optimality of the fp32 loop measured on an MI355X, (model, clamped) -> figure; the test allows 10 x
FP32_SUBOPT = {("single", False): 4.43e-7, ("single", True): 1.28e-7, ("double", False): 1.10e-6, ("double", True): 6.35e-6}


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1
    # fails on a tree without the calls
    assert callable(pkg.sim_ilqr_backward) and callable(pkg.sim_ilqr_forward) and callable(pkg.sim_ilqr)


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
    d = got - ref
    nq = sj.NX[model] // 2
    d[..., 1:nq, :] -= 2 * np.pi * np.round(d[..., 1:nq, :] / (2 * np.pi))
    return np.abs(d)


def same_bits(a, b, name="output", idx=None):
    msg = bp.first_difference(a, b, 1, idx, name)
    assert msg is None, msg


_T = {}


def tensors(pkg, orc, case, dtype):
    """-> the positional arguments of sim_ilqr_backward (params, dt, state, u, xs, x_ref, u_ref, q, r), its keywords, and the
    case's arrays as the tensors hold them.  xs is the GPU's own rollout.  Made once per (case, dtype) and left unchanged."""
    key = (case, dtype)
    if key not in _T:
        i = il.inputs(orc, case)
        held = dict(i)
        kw = dict(model=case[0], u_limit=float(i["u_limit"]))
        if i["f"] is not None:
            kw["fext"] = Tn(i["f"], dtype)
            held["f"] = N_(kw["fext"])
        if i["prm"].ndim == 2:
            params = Tn(i["prm"], dtype)
            held["prm"] = N_(params)
        else:
            params = [float(v) for v in i["prm"]]
        t = {n: Tn(i[n], dtype) for n in ("x0", "us", "x_ref", "u_ref")}
        held.update({n: N_(v) for n, v in t.items()})
        if i["PT"] is not None:
            kw["terminal"] = Tn(i["PT"], dtype)
            held["PT"] = N_(kw["terminal"])
        if i["mu"] is not None:
            kw["mu"] = Tn(i["mu"], dtype)
            held["mu"] = N_(kw["mu"])
        plant = {k: v for k, v in kw.items() if k in ("model", "fext")}
        xs = pkg.sim_rollout_states(params, case[1], t["x0"], t["us"], **plant)["xs"]
        _T[key] = ((params, case[1], t["x0"], t["us"], xs, t["x_ref"], t["u_ref"], [float(v) for v in i["q"]], float(i["r"])),
                   kw, held)
    return _T[key]


def call_bw(pkg, orc, case, dtype, want=BW_OUTS, **over):
    args, kw, _ = tensors(pkg, orc, case, dtype)
    return pkg.sim_ilqr_backward(*args, want=want, **dict(kw, **over))


_REF = {}


def ref_bw(orc, case, held=None, dtype=np.float64, tag="f64"):
    key = (case, tag, dtype)
    if key not in _REF:
        _REF[key] = il.reference(orc, case, arrays=held, dtype=dtype)
    return _REF[key]


def _alphas(nb):
    return np.random.default_rng(5).choice([1.0, 0.5, 0.25, 0.0], nb)


def fw_args(pkg, orc, case, dtype, ref):
    """the forward pass under the REFERENCE's kff and K (both sides then have the same law), a step per lane"""
    (params, dt, x0, u, xs, x_ref, u_ref, q, r), kw, held = tensors(pkg, orc, case, dtype)
    kw = {k: v for k, v in kw.items() if k != "mu"}
    kff, K, alpha = Tn(ref["kff"], dtype), Tn(ref["K"], dtype), Tn(_alphas(B), dtype)
    xs_nom = Tn(ref["xs"], dtype)
    return (params, dt, x0, u, kff, K, x0, xs_nom, x_ref, u_ref, q, r), dict(kw, alpha=alpha), \
        dict(held, kff=N_(kff), K=N_(K), alpha=N_(alpha), xs_nom=N_(xs_nom))


def ref_fw(orc, case, h):
    return il.forward_batch(orc, case[0], h["prm"], case[1], h["x0"], h["us"], h["kff"], h["K"], h["x0"], h["xs_nom"], h["alpha"],
                            h["x_ref"], h["u_ref"], h["q"], h["r"], h["PT"], h["u_limit"], h["f"])


# ---- 1. fp64 against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_fp64_matches_the_reference(pkg, orc, case):
    nt = case[2]
    ref = ref_bw(orc, case)
    got = {n: N_(v) for n, v in call_bw(pkg, orc, case, torch.float64).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    lim = il.inputs(orc, case)["u_limit"]
    near = (np.abs(np.abs(ref["un"]) - lim) <= 1e-9).any(axis=0)               # a tie at the limit: K is a discrete decision
    assert near.mean() <= 0.02
    errs = {n: lane_dist(got[n], ref[n]) for n in ("kff", "P0", "g0", "dV")}
    errs["K"] = lane_dist(got["K"], ref["K"])[~near]
    errs["hmax"] = np.abs(got["hmax"] - ref["hmax"]) / np.maximum(ref["hmax"], 1e-300)
    print("ilqr backward fp64 %s against the reference, worst lane of its largest entry: %s (bound %.0e; %d lanes out of K)" % (
        IDS[CASES.index(case)], "  ".join("%s %.2e" % (n, v.max()) for n, v in errs.items()), nt * 1e-7, near.sum()))
    assert max(v.max() for v in errs.values()) <= nt * 1e-7
    if case[3] == "limit":
        assert 0.1 <= (np.abs(got["K"]).max(axis=1) == 0).mean() <= 0.9      # the limit binds on some (lane, tick) pairs


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_fp64_matches_the_reference(pkg, orc, case):
    model, dt, nt, kind = case
    args, kw, h = fw_args(pkg, orc, case, torch.float64, ref_bw(orc, case))
    xs_ref, us_ref, J_ref = ref_fw(orc, case, h)
    got = {n: N_(v) for n, v in pkg.sim_ilqr_forward(*args, want=FW_OUTS, **kw).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    dx = state_diff(model, got["xs"], xs_ref)
    ex = (dx.max(axis=(0, 1)) / np.abs(xs_ref).max(axis=(0, 1))).max()
    eu = lane_dist(got["us"], us_ref).max()
    ej = (np.abs(got["cost"] - J_ref) / J_ref).max()
    print("ilqr forward fp64 %s against the reference: xs %.2e us %.2e of the lane's largest entry, cost %.2e relative (bound %.0e)"
          % (IDS[CASES.index(case)], ex, eu, ej, nt * 1e-7))
    assert max(ex, eu, ej) <= nt * 1e-7
    assert np.array_equal(got["xs"][-1], got["x_final"])
    if kind == "limit":
        assert np.abs(got["us"]).max() == il.LIMIT and (np.abs(got["us"]) == il.LIMIT).mean() >= 0.05


# ---- 2. fp32 against the float64 reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_fp32_within_eight_times_the_float32_algebras_gap(pkg, orc, case):
    model, dt, nt, kind = case
    _, _, held = tensors(pkg, orc, case, torch.float32)
    ref = ref_bw(orc, case, held, tag="f32in")
    r32 = ref_bw(orc, case, held, np.float32, tag="f32in")
    got = {n: N_(v) for n, v in call_bw(pkg, orc, case, torch.float32).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    x_max = np.maximum(np.abs(held["x0"]).max(axis=0), np.abs(ref["xs"]).max(axis=(0, 1)))
    state = 4 * nt * max(len(sj.sub_steps(dt)), 1) * _eps(torch.float32) * np.maximum(1.0, x_max)
    # the clamp's decision is discrete: a lane where the float run (the kernel's or the reference's own) decides otherwise than
    # the float64 reference at some tick is not comparable
    flipped = ((np.abs(got["K"]).max(axis=1) == 0) != (np.abs(ref["K"]).max(axis=1) == 0)).any(axis=0) | \
              ((np.abs(r32["K"]).max(axis=1) == 0) != (np.abs(ref["K"]).max(axis=1) == 0)).any(axis=0)
    if dt == 0.0:
        flipped[:] = False                                                     # K = 0 everywhere: nothing to decide
    assert flipped.mean() <= 0.02
    ok = True
    for name in ("K", "kff", "dV", "P0", "g0"):
        gap = lane_dist(r32[name], ref[name])[~flipped].max()
        bound = 8 * gap + state
        err = lane_dist(got[name], ref[name])
        err[flipped] = 0.0
        print("ilqr backward fp32 %s %s: float32-algebra gap %.2e, kernel's error %.2e, error / bound %.3f (lane %d; %d lanes beyond "
              "the bound, %d left out)" % (IDS[CASES.index(case)], name, gap, err.max(), (err / bound).max(), int((err / bound).argmax()),
                                           int((err > bound).sum()), int(flipped.sum())))
        ok = ok and bool((err <= bound).all())
    assert ok


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_fp32_within_the_state_bound_carried_through_the_law(pkg, orc, case):
    model, dt, nt, kind = case
    nx = sj.NX[model]
    _, _, held = tensors(pkg, orc, case, torch.float32)
    args, kw, h = fw_args(pkg, orc, case, torch.float32, ref_bw(orc, case, held, tag="f32in"))
    xs_ref, us_ref, J_ref = ref_fw(orc, case, h)
    got = {n: N_(v) for n, v in pkg.sim_ilqr_forward(*args, want=FW_OUTS, **kw).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    eps = _eps(torch.float32)
    x_at = np.concatenate([h["x0"][None], xs_ref[:-1]])
    e = 4 * max(len(sj.sub_steps(dt)), 1) * eps * np.maximum(1.0, np.abs(np.concatenate([x_at, xs_ref[-1:]])).max(axis=(0, 1)))
    gam_max = np.stack([np.abs(lq.trajectory(orc, model, il.sr._params(h["prm"], b), dt, h["x0"][:, b], us_ref[:, b],
                                             il.sr._lane(h["f"], b))[2]).max(axis=1) for b in range(B)], axis=1)
    q, r = np.asarray(h["q"]), h["r"]
    E, worst_x, worst_u, dJ = np.zeros(B), 0.0, 0.0, np.zeros(B)
    for t in range(nt):
        n_at = h["x0"] if t == 0 else h["xs_nom"][t - 1]
        d = lq.wrap_nearest(model, x_at[t] - n_at)
        du = np.abs(h["K"][t]).sum(axis=0) * E + (nx + 3) * eps * (np.abs(h["us"][t]) + np.abs(h["alpha"] * h["kff"][t]) +
                                                                   np.abs(h["K"][t] * d).sum(axis=0))
        du = du + eps * np.abs(us_ref[t])
        worst_u = max(worst_u, (np.abs(got["us"][t] - us_ref[t]) / du).max())
        et = lq.wrap_nearest(model, x_at[t] - h["x_ref"][t])
        dJ += 2 * (q[:, None] * np.abs(et)).sum(axis=0) * (E + eps * np.abs(et).max(axis=0)) + \
            2 * r * np.abs(us_ref[t] - h["u_ref"][t]) * (du + eps * np.abs(h["u_ref"][t]))
        E = E + e + 1.25 * gam_max[t] * du
        worst_x = max(worst_x, (state_diff(model, got["xs"][t], xs_ref[t]).max(axis=0) / E).max())
    eT = lq.wrap_nearest(model, xs_ref[-1] - h["x_ref"][nt])
    PT = np.stack([il._terminal(h["q"], h["PT"], b) for b in range(B)], axis=-1)
    dJ += 2 * np.abs(np.einsum("ijb,jb->ib", PT, eT)).sum(axis=0) * (E + eps * np.abs(eT).max(axis=0))
    dJ += (nt * (nx + 2) + nx * nx + 4) * eps * J_ref
    worst_j = (np.abs(got["cost"] - J_ref) / dJ).max()
    print("ilqr forward fp32 %s: worst error / bound: xs %.3f us %.3f cost %.3f (cost's relative error %.2e)" % (
        IDS[CASES.index(case)], worst_x, worst_u, worst_j, (np.abs(got["cost"] - J_ref) / J_ref).max()))
    assert worst_x <= 1.0 and worst_u <= 1.0 and worst_j <= 1.0


# ---- 3. identities and structure ------------------------------------------------------------------------------------------
STRUCT = [c for c in CASES if c[1] == 0.0105 and c[2] == 5 and c[3] in ("dyn", "PT", "mu", "limit")]
STRUCT_IDS = ["%s-%g-%d-%s" % c for c in STRUCT]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in CASES if c[3] in (None, "dyn", "PT", "per")], ids=lambda c: "%s-%g-%d-%s" % c)
def test_at_its_own_reference_it_is_sim_lqr(pkg, orc, case, dtype):
    (params, dt, x0, u, xs, _, _, q, r), kw, _ = tensors(pkg, orc, case, dtype)
    x_ref = torch.cat([x0[None], xs]).contiguous()
    got = pkg.sim_ilqr_backward(params, dt, x0, u, xs, x_ref, u, q, r, want=BW_OUTS, **kw)
    assert (got["kff"] == 0).all() and (got["dV"] == 0).all() and (got["g0"] == 0).all() and (got["hmax"] == 0).all()
    lqr = pkg.sim_lqr(params, dt, x0, u, xs, q, r, **{k: v for k, v in kw.items() if k != "u_limit"})
    same_bits(lqr["K"], got["K"], "K")
    same_bits(lqr["P0"], got["P0"], "P0")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in CASES if c[3] in (None, "dyn", "per")], ids=lambda c: "%s-%g-%d-%s" % c)
def test_without_feedforward_gains_and_limit_it_is_the_plain_rollout(pkg, orc, case, dtype):
    (params, dt, x0, u, xs, x_ref, u_ref, q, r), kw, _ = tensors(pkg, orc, case, dtype)
    plant = {k: v for k, v in kw.items() if k in ("model", "fext")}
    got = pkg.sim_ilqr_forward(params, dt, x0, u, None, None, None, None, x_ref, u_ref, q, r, want=FW_OUTS, **plant)
    same_bits(xs, got["xs"], "xs")
    same_bits(xs[-1], got["x_final"], "x_final")
    same_bits(u, got["us"], "us")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT + [c for c in CASES if c[2] in (1, 8, 12)], ids=lambda c: "%s-%g-%d-%s" % c)
def test_from_the_nominal_start_with_alpha_zero_it_reproduces_the_nominal(pkg, orc, case, dtype):
    (params, dt, x0, u, _, x_ref, u_ref, q, r), kw, _ = tensors(pkg, orc, case, dtype)
    fkw = {k: v for k, v in kw.items() if k != "mu"}
    nom = pkg.sim_ilqr_forward(params, dt, x0, u, None, None, None, None, x_ref, u_ref, q, r, want=("xs", "us", "cost"), **fkw)
    bw = pkg.sim_ilqr_backward(params, dt, x0, nom["us"], nom["xs"], x_ref, u_ref, q, r, want=("K", "kff"), **kw)
    assert torch.isfinite(bw["K"]).all() and torch.isfinite(bw["kff"]).all() and (bw["kff"] != 0).any()
    zero = torch.zeros(B, dtype=dtype, device=DEV)
    got = pkg.sim_ilqr_forward(params, dt, x0, nom["us"], bw["kff"], bw["K"], x0, nom["xs"], x_ref, u_ref, q, r, alpha=zero,
                               want=FW_OUTS, **fkw)
    same_bits(nom["xs"], got["xs"], "xs")
    same_bits(nom["us"], got["us"], "us")
    same_bits(nom["cost"], got["cost"], "cost")
    full = pkg.sim_ilqr_forward(params, dt, x0, nom["us"], bw["kff"], bw["K"], x0, nom["xs"], x_ref, u_ref, q, r, want="us", **fkw)
    assert not torch.equal(full["us"], nom["us"])                              # and alpha = 1 (None) does move


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_outputs_do_not_depend_on_each_other_and_the_inputs_are_read_only(pkg, orc, case, dtype):
    args, kw, _ = tensors(pkg, orc, case, dtype)
    fa, fkw, _ = fw_args(pkg, orc, case, dtype, ref_bw(orc, case))
    held = [a for a in args + fa if isinstance(a, torch.Tensor)] + [v for v in list(kw.values()) + list(fkw.values())
                                                                    if isinstance(v, torch.Tensor)]
    before = [a.clone() for a in held]
    every = call_bw(pkg, orc, case, dtype)
    for name in BW_OUTS:
        same_bits(every[name], call_bw(pkg, orc, case, dtype, want=name)[name], name + " alone")
    assert torch.equal(every["P0"], every["P0"].transpose(0, 1))             # exactly symmetric
    fw = pkg.sim_ilqr_forward(*fa, want=FW_OUTS, **fkw)
    for name in FW_OUTS:
        same_bits(fw[name], pkg.sim_ilqr_forward(*fa, want=name, **fkw)[name], name + " alone")
    same_bits(fw["xs"][-1], fw["x_final"], "xs[-1]")
    for a, b in zip(held, before):
        assert torch.equal(a, b)
    if "terminal" in kw:   # only PT's lower triangle is read
        junk = kw["terminal"].clone()
        iu = np.triu_indices(junk.shape[0], 1)
        junk[iu[0], iu[1]] = float("nan")
        got = call_bw(pkg, orc, case, dtype, terminal=junk)
        for name in BW_OUTS:
            same_bits(every[name], got[name], name + " with NaNs above PT's diagonal")
        same_bits(fw["cost"], pkg.sim_ilqr_forward(*fa, want="cost", **dict(fkw, terminal=junk))["cost"], "cost, NaNs above")


def _arranged(pkg, fn, args, kw, idx, want):
    take = lambda v: bp.take(v, idx) if isinstance(v, torch.Tensor) else v     # noqa: E731
    return fn(*[take(a) for a in args], want=want, **{k: take(v) for k, v in kw.items()})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_a_lanes_bits_do_not_depend_on_its_place_in_the_batch(pkg, orc, case, dtype):
    """the same lanes reversed, and as prefixes that end alone, below, on and above a wave boundary"""
    args, kw, _ = tensors(pkg, orc, case, dtype)
    fa, fkw, _ = fw_args(pkg, orc, case, dtype, ref_bw(orc, case))
    for fn, a, k, outs in ((pkg.sim_ilqr_backward, args, kw, BW_OUTS), (pkg.sim_ilqr_forward, fa, fkw, FW_OUTS)):
        natural = fn(*a, want=outs, **k)
        rev = bp.permutations(B, 7)["reverse"]
        got = _arranged(pkg, fn, a, k, rev, outs)
        for name in outs:
            same_bits(natural[name], bp.put_back(got[name], rev), name + " reversed", rev)
        for nb in (1, 63, 64, 65):
            idx = np.arange(nb, dtype=np.int64)
            got = _arranged(pkg, fn, a, k, idx, outs)
            for name in outs:
                same_bits(bp.take(natural[name], idx), got[name], "%s of the first %d" % (name, nb))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT[:1] + STRUCT[4:5], ids=STRUCT_IDS[:1] + STRUCT_IDS[4:5])
def test_a_poisoned_lane_stays_in_its_lane(pkg, orc, case, dtype):
    (params, dt, x0, u, xs, x_ref, u_ref, q, r), kw, _ = tensors(pkg, orc, case, dtype)
    clean = call_bw(pkg, orc, case, dtype)
    lane = 70
    others = np.array([b for b in range(B) if b != lane], dtype=np.int64)
    bad = x_ref.clone()
    bad[2, 1, lane] = float("nan")
    got = pkg.sim_ilqr_backward(params, dt, x0, u, xs, bad, u_ref, q, r, want=BW_OUTS, **kw)
    for name in BW_OUTS:
        same_bits(bp.take(clean[name], others), bp.take(got[name], others), name)
    assert torch.isnan(got["g0"][:, lane]).any() and torch.isnan(got["kff"][:, lane]).any() and torch.isnan(got["hmax"][lane])
    fkw = {k: v for k, v in kw.items() if k != "mu"}
    f_clean = pkg.sim_ilqr_forward(params, dt, x0, u, clean["kff"], clean["K"], x0, xs, x_ref, u_ref, q, r, want=FW_OUTS, **fkw)
    f_bad = pkg.sim_ilqr_forward(params, dt, x0, u, got["kff"], got["K"], x0, xs, x_ref, u_ref, q, r, want=FW_OUTS, **fkw)
    for name in FW_OUTS:
        same_bits(bp.take(f_clean[name], others), bp.take(f_bad[name], others), name)
    assert torch.isnan(f_bad["us"][:, lane]).any() and torch.isnan(f_bad["cost"][lane])


# ---- 4. dt = 0 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["single", "double"])
def test_dt_zero_is_the_closed_form(pkg, orc, model, dtype):
    case = (model, 0.0, 3, None)
    (params, dt, x0, u, xs, x_ref, u_ref, q, r), kw, h = tensors(pkg, orc, case, dtype)
    nt, nx, eps = case[2], sj.NX[model], _eps(dtype)
    mu = Tn(np.random.default_rng(3).choice([0.0, 0.01, 1.0], B), dtype)
    lim = 15.0
    assert torch.equal(xs, x0[None].expand(nt, nx, B))                        # the identity plant
    got = {n: N_(v) for n, v in pkg.sim_ilqr_backward(params, dt, x0, u, xs, x_ref, u_ref, q, r, mu=mu, u_limit=lim, want=BW_OUTS,
                                                      model=model).items()}
    m = N_(mu)
    un = h["us"] - (h["us"] - h["u_ref"]) * r / (r + m)
    kff = np.clip(un, -lim, lim) - h["us"]
    e = np.stack([lq.wrap_nearest(model, h["x0"] - h["x_ref"][t]) for t in range(nt + 1)])
    qv = np.asarray(q)
    g0 = (qv[None, :, None] * e).sum(axis=0)                                    # P_T = diag(q): the terminal term is one more
    hq = r * (h["us"] - h["u_ref"])
    dV = np.stack([(2 * kff * hq).sum(axis=0), (kff ** 2 * r).sum(axis=0)])
    assert (got["K"] == 0).all() and got["K"].shape == (nt, nx, B)
    assert (np.abs(un) > lim).any() and (np.abs(un) < lim).any()
    tol = 8 * nt * eps
    # kff = clamp(u - ..) - u cancels against u: its error, and hmax's, is relative to the lane's largest |u|
    u_max = np.abs(h["us"]).max(axis=0)
    # and dV carries kff's absolute error through its own derivative: 2 |h| and 2 r |kff| a tick
    scales = dict(kff=u_max, hmax=u_max * (r + m),
                  dV=(2 * np.abs(hq) + 2 * r * np.abs(kff)).sum(axis=0) * u_max + np.abs(dV).max(axis=0))
    for name, want in (("kff", kff), ("g0", g0), ("dV", dV), ("P0", np.tile(((nt + 1) * np.diag(qv))[:, :, None], (1, 1, B))),
                       ("hmax", (np.abs(kff) * (r + m)).max(axis=0))):
        ax = tuple(range(want.ndim - 1))
        d = (np.abs(got[name] - want).max(axis=ax) / scales.get(name, np.abs(want).max(axis=ax))).max()
        print("ilqr dt = 0 %s %s %s: worst lane %.2e of its scale (bound %.2e)" % (model, dtype, name, d, tol))
        assert d <= tol
    fw = pkg.sim_ilqr_forward(params, dt, x0, u, Tn(kff, dtype), None, None, None, x_ref, u_ref, q, r, u_limit=lim, model=model,
                              want=FW_OUTS)
    assert torch.equal(fw["xs"], xs) and torch.equal(fw["x_final"], x0)
    us = np.clip(h["us"] + N_(Tn(kff, dtype)), -lim, lim)
    J = (qv[None, :, None] * e ** 2).sum(axis=(0, 1)) + r * ((us - h["u_ref"]) ** 2).sum(axis=0)
    assert lane_dist(N_(fw["us"]), us).max() <= 2 * eps and (np.abs(N_(fw["cost"]) - J) <= tol * nx * J).all()


# ---- 5. the loop ------------------------------------------------------------------------------------------------------------
_LOOP = {}


def loop_run(pkg, model, clamped, dtype):
    key = (model, clamped, dtype)
    if key not in _LOOP:
        x0, u0, target, qf = il.loop_draws(model)
        args = ([float(v) for v in sj.DYN[model]], il.LOOP_DT, Tn(x0, dtype), Tn(u0, dtype), [float(v) for v in target], il.Q[model], il.R)
        kw = dict(terminal=qf, u_limit=float(il.loop_limit(model, clamped)), iterations=il.LOOP_ITERS, trials=il.LOOP_TRIALS,
                  model=model)
        _LOOP[key] = (args, kw, pkg.sim_ilqr(*args, **kw))
    return _LOOP[key]


LOOPS = [(m, c) for m in ("single", "double") for c in (False, True)]
LOOP_IDS = ["%s-%s" % (m, "clamped" if c else "free") for m, c in LOOPS]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model,clamped", LOOPS, ids=LOOP_IDS)
def test_the_loop_never_raises_the_cost_and_ends_at_the_references_minimum(pkg, orc, model, clamped, dtype):
    """fp32 sub-optimality measured on an MI355X, worst of the 32 lanes relative to the reference's converged cost (FP32_SUBOPT at
    the top of the file): 4-state free 4.43e-7, clamped at 4 N 1.28e-7; 6-state free 1.10e-6, clamped at 8 N 6.35e-6, with 2 to 12
    of the 12 iterations accepted per lane (fp64: 5 to 12) -- the float cost's own rounding, about 1e-7 J, ends the line search's
    progress there.  The bound is 10 x the figure.  fp64, measured: at most 1e-14; bound 1e-8."""
    (params, dt, x0, u0, target, q, r), kw, run = loop_run(pkg, model, clamped, dtype)
    h = N_(run["cost_history"])
    assert h.shape == (il.LOOP_ITERS + 1, il.LOOP_NB) and np.isfinite(h).all()
    assert (np.diff(h, axis=0) <= 0).all()
    acc = run["accepted"].cpu().numpy()
    assert acc.shape == (il.LOOP_ITERS, il.LOOP_NB) and (np.diff(h, axis=0)[~acc] == 0).all() and (np.diff(h, axis=0)[acc] < 0).all()
    same_bits(run["cost_history"][-1], run["cost"], "cost")
    lim = il.loop_limit(model, clamped)
    u = N_(run["u"])
    assert np.abs(u).max() <= lim
    if clamped:
        assert (np.abs(u) == lim).any(axis=0).sum() >= il.LOOP_NB / 4
    # the GPU's controls through the numpy plant and cost, against the reference loop's converged cost
    # (from the float64 start the reference minimised from: the sub-optimality is then >= 0 up to the reference's own residual)
    xs, us, J = il.forward_batch(orc, model, params, dt, il.loop_draws(model)[0], u, None, None, None, None, None,
                                 np.asarray(target), None, q, r, kw["terminal"], lim)
    assert np.array_equal(us, u)
    J_ref = il.loop_golden()["%s_%s" % (model, "clamped" if clamped else "free")]
    sub = (J - J_ref) / J_ref
    print("ilqr loop %s %s %s: sub-optimality of the returned controls against the reference's converged cost, worst lane %.3e "
          "(least %.3e); hmax at most %.2e; iterations accepted per lane %d .. %d" % (
              model, "clamped" if clamped else "free", dtype, sub.max(), sub.min(), N_(run["hmax"]).max(), acc.sum(axis=0).min(),
              acc.sum(axis=0).max()))
    if dtype == torch.float64:
        assert sub.max() <= 1e-8
    else:
        assert sub.max() <= 10 * FP32_SUBOPT[(model, clamped)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model,clamped", LOOPS, ids=LOOP_IDS)
def test_the_loop_is_the_public_calls_in_its_order(pkg, model, clamped, dtype):
    (params, dt, x0, u0, target, q, r), kw, run = loop_run(pkg, model, clamped, dtype)
    nb = il.LOOP_NB
    ckw = dict(terminal=kw["terminal"], u_limit=kw["u_limit"], model=model)
    first = pkg.sim_ilqr_forward(params, dt, x0, u0, None, None, None, None, target, None, q, r, want=("xs", "us", "cost"), **ckw)
    u, xs, J = first["us"], first["xs"], first["cost"]
    mu = torch.zeros(nb, dtype=dtype, device=DEV)
    hist, rejected = [J], 0
    for it in range(kw["iterations"]):
        bw = pkg.sim_ilqr_backward(params, dt, x0, u, xs, target, None, q, r, mu=mu, want=("K", "kff", "dV"), **ckw)
        alpha = torch.ones(nb, dtype=dtype, device=DEV)
        done = torch.zeros(nb, dtype=torch.bool, device=DEV)
        for _ in range(kw["trials"]):
            J_try = pkg.sim_ilqr_forward(params, dt, x0, u, bw["kff"], bw["K"], x0, xs, target, None, q, r, alpha=alpha, want="cost",
                                         **ckw)["cost"]
            pred = bw["dV"][0] * alpha + bw["dV"][1] * alpha * alpha
            done = done | ((pred < 0) & (J_try - J <= 1e-4 * pred))
            alpha = torch.where(done, alpha, 0.5 * alpha)
        alpha = torch.where(done, alpha, torch.zeros_like(alpha))
        fin = pkg.sim_ilqr_forward(params, dt, x0, u, bw["kff"], bw["K"], x0, xs, target, None, q, r, alpha=alpha,
                                   want=("xs", "us", "cost"), **ckw)
        keep = (~done).cpu().numpy().nonzero()[0]
        if keep.size:                                                           # a rejected lane keeps its trajectory bit for bit
            rejected += keep.size
            for name, old in (("xs", xs), ("us", u), ("cost", J)):
                same_bits(bp.take(old, keep), bp.take(fin[name], keep), "%s of the rejected lanes, iteration %d" % (name, it))
        same_bits(run["accepted"][it].to(torch.int32), done.to(torch.int32), "accepted[%d]" % it)
        u, xs, J = fin["us"], fin["xs"], fin["cost"]
        down = mu / 10.0
        mu = torch.where(done, torch.where(down < 1e-6, torch.zeros_like(mu), down), torch.clamp(10.0 * mu, min=1e-3))
        hist.append(J)
    last = pkg.sim_ilqr_backward(params, dt, x0, u, xs, target, None, q, r, mu=mu, want=("K", "hmax"), **ckw)
    assert rejected > 0                                                         # the converged lanes do reject
    for name, mine in (("u", u), ("xs", xs), ("cost", J), ("mu", mu), ("K", last["K"]), ("hmax", last["hmax"]),
                       ("cost_history", torch.stack(hist))):
        same_bits(run[name], mine, name)


def test_the_simulators_ilqr_is_sim_ilqr_on_its_state(pkg):
    (params, dt, x0, u0, target, q, r), kw, run = loop_run(pkg, "single", True, torch.float64)
    sim = pkg.BatchSimulator(il.LOOP_NB, dtype=torch.float64, device=0, model="single")
    sim.set_state(x0)
    got = sim.ilqr(params, dt, u0, target, q, r, **{k: v for k, v in kw.items() if k != "model"})
    for name in run:
        same_bits(run[name].to(torch.int32) if run[name].dtype == torch.bool else run[name],
                  got[name].to(torch.int32) if got[name].dtype == torch.bool else got[name], name)
    assert torch.equal(sim.get_state(), x0)                                     # a plan: the plant does not move
