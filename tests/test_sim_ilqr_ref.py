"""CPU: the numpy reference of the iLQR passes and of the loop above them (tests/helpers/sim_ilqr_ref.py) pinned, and the
conditions the GPU test's inputs must meet.  Both models throughout.

1. With mu = 0 and no limit, rolling the linearised system from dx_0 = 0 under du = kff + K dx gives the minimiser of the stacked
   least-squares problem, and dV1 + dV2 is that problem's cost change: both within 1e-9 of the largest entry.
2. With the reference equal to the trajectory itself kff = 0, dV = 0, and K, P0 are sim_lqr_ref.riccati's.
3. g0 with K and kff forced to zero (a very large mu) is half the finite-difference gradient of J in x0.
4. The float32-algebra run of the recursion stays finite; its gap is printed (the fp32 GPU bound is built from it).
5. The loop test's inputs, on the first 8 of the GPU test's 32 lanes: every lane's cost is non-increasing; in the clamped case at
   least a quarter of the lanes sit at +-u_limit on some tick; the runs at LOOP_ITERS and at LOOP_ITERS + 5 iterations agree in
   final cost to 1e-10 relative on every lane.  (The loop is deterministic, so the shorter run's cost is row LOOP_ITERS of the
   longer run's history.)  tests/golden/sim_ilqr_loop_costs.json, the converged costs of all 32 lanes that the GPU test reads, is
   held to these lanes.  The 4-state model starts +-0.3 off the upright under 4 N, the prototype's setting; the 6-state one
   +-0.1 under 8 N.
6. The limit case of the GPU test: the limit binds on some (lane, tick) pairs and not on others, and fewer than 2 % of the lanes
   have an unclamped control within 1e-9 of the limit."""
import numpy as np
import pytest

from helpers import sim_ilqr_ref as il
from helpers import sim_jac_ref as sj
from helpers import sim_lqr_ref as lq
from helpers import sim_rollout_ref as sr

NB = 8
MODELS = ["single", "double"]
DENSE = [c for c in il.CASES if c[1] > 0.0 and c[3] in (None, "dyn", "PT", "per")]


def _lane_pieces(orc, case, b):
    i = il.inputs(orc, case, NB)
    model, dt = case[0], case[1]
    xs, Phi, gam = lq.trajectory(orc, model, sr._params(i["prm"], b), dt, i["x0"][:, b], i["us"][:, b], sr._lane(i["f"], b))
    PT = il._terminal(i["q"], i["PT"], b)
    return i, xs, Phi, gam, PT


@pytest.mark.parametrize("case", DENSE, ids=lambda c: "%s-%g-%d-%s" % c)
def test_the_policy_is_the_stacked_least_squares_minimiser(orc, case):
    worst_du = worst_dv = 0.0
    for b in range(NB):
        i, xs, Phi, gam, PT = _lane_pieces(orc, case, b)
        e = il.residuals(case[0], i["x0"][:, b], xs, i["x_ref"][:, :, b])
        bw = il.backward(Phi, gam, e, i["us"][:, b], i["u_ref"][:, b], i["q"], i["r"], PT)
        du_dense, change = il.dense_step(Phi, gam, e, i["us"][:, b], i["u_ref"][:, b], i["q"], i["r"], PT)
        du = il.policy_rollout(Phi, gam, bw["K"], bw["kff"])
        worst_du = max(worst_du, np.abs(du - du_dense).max() / np.abs(du_dense).max())
        worst_dv = max(worst_dv, abs(bw["dV"].sum() - change) / max(abs(change), np.abs(bw["dV"]).max()))
        assert bw["dV"][0] < 0 < bw["dV"][1] and bw["dV"].sum() < 0
    print("ilqr ref %s-%g-%d-%s: policy against least squares, worst lane: du %.2e  dV1 + dV2 %.2e" % (case + (worst_du, worst_dv)))
    assert worst_du <= 1e-9 and worst_dv <= 1e-9


@pytest.mark.parametrize("case", DENSE, ids=lambda c: "%s-%g-%d-%s" % c)
def test_at_its_own_reference_it_is_the_lqr_recursion(orc, case):
    for b in range(NB):
        i, xs, Phi, gam, PT = _lane_pieces(orc, case, b)
        x_ref = np.concatenate([i["x0"][None, :, b], xs])
        e = il.residuals(case[0], i["x0"][:, b], xs, x_ref)
        bw = il.backward(Phi, gam, e, i["us"][:, b], i["us"][:, b], i["q"], i["r"], PT)
        assert (bw["kff"] == 0).all() and (bw["dV"] == 0).all() and (bw["g0"] == 0).all() and bw["hmax"] == 0
        K, P0 = lq.riccati(Phi, gam, i["q"], i["r"], PT)
        assert np.abs(bw["K"] - K).max() <= 1e-12 * np.abs(K).max()
        assert np.abs(bw["P0"] - P0).max() <= 1e-12 * np.abs(P0).max()


@pytest.mark.parametrize("model", MODELS)
def test_g0_is_half_the_gradient_of_the_cost_in_x0(orc, model):
    x_nom, u_nom, _, qf = lq.tracking_draws(model, 4)
    T, dt, prm, h = 8, 0.01, sj.DYN[model], 1e-6
    nx = sj.NX[model]
    target = np.zeros(nx)
    target[1:nx // 2] = np.pi / 2
    PT = lq.terminal_matrix(il.Q[model], qf)
    worst = 0.0
    for b in range(4):
        us, uref = u_nom[:T, b], np.zeros(T)
        xref = np.tile(target[None], (T + 1, 1))

        def J(x0):
            xs, _, _ = lq.trajectory(orc, model, prm, dt, x0, us)
            return il.cost(model, x0, xs, us, xref, uref, il.Q[model], il.R, PT)
        xs, Phi, gam = lq.trajectory(orc, model, prm, dt, x_nom[:, b], us)
        bw = il.backward(Phi, gam, il.residuals(model, x_nom[:, b], xs, xref), us, uref, il.Q[model], il.R, PT, mu=1e30)
        assert np.abs(bw["kff"]).max() < 1e-20 and np.abs(bw["K"]).max() < 1e-20
        fd = np.array([(J(x_nom[:, b] + h * np.eye(nx)[j]) - J(x_nom[:, b] - h * np.eye(nx)[j])) / (2 * h) for j in range(nx)])
        worst = max(worst, np.abs(bw["g0"] - fd / 2).max() / np.abs(fd / 2).max())
    print("ilqr ref %s: g0 against half the central difference of J in x0, worst lane %.2e" % (model, worst))
    assert worst <= 1e-6


@pytest.mark.parametrize("case", il.CASES, ids=il.IDS)
def test_float32_algebra_stays_finite(orc, case):
    ref, r32 = il.reference(orc, case, NB), il.reference(orc, case, NB, dtype=np.float32)
    names = ("K", "kff", "dV", "P0", "g0")
    assert all(np.isfinite(r32[n]).all() for n in names)

    def rel(a, b):
        ax = tuple(range(b.ndim - 1))
        s = np.abs(b).max(axis=ax)
        return float((np.abs(a - b).max(axis=ax) / np.where(s > 0, s, 1.0)).max())
    print("ilqr ref %s: float32-algebra gap, worst lane relative to its largest entry: %s" % (
        il.IDS[il.CASES.index(case)], "  ".join("%s %.2e" % (n, rel(r32[n], ref[n])) for n in names)))


_LOOPS = {}


def _loop(orc, model, clamped):
    key = (model, clamped)
    if key not in _LOOPS:
        x0, u0, target, qf = il.loop_draws(model, NB)
        lim = il.LOOP_LIMIT[model] if clamped else np.inf
        _LOOPS[key] = (lim, il.loop_batch(orc, model, sj.DYN[model], il.LOOP_DT, x0, u0, target, il.Q[model], il.R, qf, None, lim,
                                          il.LOOP_ITERS + 5, il.LOOP_TRIALS))
    return _LOOPS[key]


@pytest.mark.parametrize("clamped", [False, True], ids=["free", "clamped"])
@pytest.mark.parametrize("model", MODELS)
def test_the_loops_inputs_are_admissible(orc, model, clamped):
    lim, run = _loop(orc, model, clamped)
    h = run["cost_history"]
    at, end = h[il.LOOP_ITERS], h[-1]
    sat = (np.abs(run["u"]) == lim).any(axis=0)
    print("ilqr ref loop %s %s: cost %.3g .. %.3g, iterations accepted per lane %d .. %d, |J(%d) - J(%d)| / J at most %.1e, "
          "hmax at most %.1e, lanes at the limit %d of %d" % (
              model, "clamped at %g" % lim if clamped else "free", end.min(), end.max(), run["accepted"].sum(axis=0).min(),
              run["accepted"].sum(axis=0).max(), il.LOOP_ITERS, il.LOOP_ITERS + 5, (np.abs(at - end) / end).max(), run["hmax"].max(),
              sat.sum(), NB))
    assert (np.diff(h, axis=0) <= 0).all()
    assert (np.abs(at - end) <= 1e-10 * end).all()
    gold = il.loop_golden()["%s_%s" % (model, "clamped" if clamped else "free")]   # what the GPU test reads for all 32 lanes
    assert gold.shape == (il.LOOP_NB,) and (np.abs(at - gold[:NB]) <= 1e-12 * gold[:NB]).all()
    assert np.abs(run["u"]).max() <= lim
    if clamped:
        assert sat.sum() >= NB / 4
    # a rejected iteration leaves the cost where it was, to the bit
    assert (np.diff(h, axis=0)[~run["accepted"]] == 0).all()


@pytest.mark.parametrize("model", MODELS)
def test_the_limit_case_binds_and_stays_clear_of_ties(orc, model):
    case = (model, 0.0105, 5, "limit")
    ref = il.reference(orc, case)          # the GPU test's 130 lanes
    held = (np.abs(ref["un"]) > il.LIMIT)
    near = (np.abs(np.abs(ref["un"]) - il.LIMIT) <= 1e-9).any(axis=0)
    print("ilqr ref %s: the limit %g binds on %.0f %% of the (lane, tick) pairs; lanes within 1e-9 of it: %d" % (
        model, il.LIMIT, 100 * held.mean(), near.sum()))
    assert 0.1 <= held.mean() <= 0.9
    assert near.mean() <= 0.02
    assert (np.abs(ref["K"]).max(axis=1)[held] == 0).all()     # no feedback on a control that sits on the limit
    assert np.abs(il.inputs(orc, case)["us"]).max() <= il.LIMIT
