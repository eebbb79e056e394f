"""CPU: the numpy reference of the LQR gains along a plant trajectory and of the feedback rollout (tests/helpers/sim_lqr_ref.py)
pinned, and the conditions the GPU test's inputs must meet.

1. Two formulations: the textbook Riccati recursion and the T-step problem solved as one least-squares system agree in K_0 and
   P0 within 1e-12 of the lane's largest entry on every case of the GPU test.  The cap only shows the cases well conditioned.
2. The float32-algebra run of the recursion stays finite; its gap to float64 is printed (the fp32 GPU bound is built from it).
3. dt = 0: K = 0 and P0 = P_T + T diag(q).
4. The feedback cases: with u_limit = FB_LIMIT the clamp acts on between 10 % and 90 % of the (lane, tick) pairs, and some lane's
   state and nominal state lie on different sides of the +-pi cut at some tick.
5. Tracking: 60 ticks of 10 ms near the upright from a start moved by 1e-2 (every state, random signs): on every lane the open
   loop ends at least 4 x further from the nominal end state than it began (the premise) and the closed loop within 0.25 of the
   open loop's distance.  On all 130 lanes of the GPU test the reference gives: worst ratio 0.041 (4-state) and 0.134
   (6-state), open-loop growth at least 18.9 x and 13.9 x, |u| <= 3.8; here the first 16 of those lanes."""
import numpy as np
import pytest

from helpers import sim_jac_ref as sj
from helpers import sim_lqr_ref as lq

NB = 16   # lanes of the CPU checks: the first 16 of the GPU test's draws hold the wrapping and the bumper blocks (nb // 4 each)


def _lane_rel(a, b):
    ax = tuple(range(b.ndim - 1))
    s = np.abs(b).max(axis=ax)
    return float((np.abs(a - b).max(axis=ax) / np.where(s > 0, s, 1.0)).max())


@pytest.mark.parametrize("case", lq.CASES, ids=lq.IDS)
def test_the_recursion_is_the_stacked_least_squares_problem(orc, case):
    ref = lq.reference(orc, case, NB, dense=True)
    d = dict(K0=_lane_rel(ref["K"][0], ref["K0_dense"]), P0=_lane_rel(ref["P0"], ref["P0_dense"]))
    print("lqr ref %s: recursion against least squares, worst lane relative to its largest entry: %s; max |P0| %.2e, max |K| %.2e" % (
        lq.IDS[lq.CASES.index(case)], "  ".join("%s %.2e" % kv for kv in d.items()), np.abs(ref["P0"]).max(), np.abs(ref["K"]).max()))
    assert max(d.values()) <= 1e-12
    assert np.array_equal(ref["P0"], ref["P0"].transpose(1, 0, 2))
    assert np.linalg.eigvalsh(np.moveaxis(ref["P0"], -1, 0)).min() > 0.0


@pytest.mark.parametrize("case", lq.CASES, ids=lq.IDS)
def test_float32_algebra_stays_finite(orc, case):
    ref, r32 = lq.reference(orc, case, NB), lq.reference(orc, case, NB, dtype=np.float32)
    assert all(np.isfinite(r32[n]).all() for n in ("K", "P0"))
    print("lqr ref %s: float32-algebra gap, worst lane relative to its largest entry: K %.2e  P0 %.2e" % (
        lq.IDS[lq.CASES.index(case)], _lane_rel(r32["K"], ref["K"]), _lane_rel(r32["P0"], ref["P0"])))


@pytest.mark.parametrize("case", [c for c in lq.CASES if c[1] == 0.0], ids=lambda c: "%s-%g-%d-%s" % c)
def test_dt_zero_closed_form(orc, case):
    i = lq.inputs(orc, case, NB)
    ref = lq.reference(orc, case, NB)
    assert (ref["K"] == 0).all()
    want = (1 + case[2]) * np.diag(i["q"])
    assert np.abs(ref["P0"] - want[:, :, None]).max() <= 1e-14 * np.abs(want).max()
    PT = lq.terminal_costs(case[0], NB)
    got = lq.lqr_batch(orc, case[0], i["prm"], 0.0, i["x0"], i["us"], i["q"], i["r"], PT)
    want = PT + case[2] * np.diag(i["q"])[:, :, None]
    assert (got["K"] == 0).all() and np.abs(got["P0"] - want).max() <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("model", ["single", "double"])
def test_feedback_cases_clamp_and_cross_the_cut(orc, model):
    case = (model, 0.0105, 5, "clamp")
    i = lq.fb_inputs(orc, case)   # the GPU test's 130 lanes
    free_case = (model, 0.0105, 5, None)
    _, us_free = lq.fb_reference(orc, free_case)
    xs, us = lq.fb_reference(orc, case)
    frac = float((np.abs(us_free) > lq.FB_LIMIT).mean())
    acted = float((np.abs(us) == lq.FB_LIMIT).mean())
    print("lqr ref %s: the clamp at %g would act on %.0f %% of the unclamped law's (lane, tick) pairs and acts on %.0f %%" % (
        model, lq.FB_LIMIT, 100 * frac, 100 * acted))
    assert 0.1 <= acted <= 0.9 and np.abs(us).max() <= lq.FB_LIMIT
    nq = sj.NX[model] // 2
    x_at = np.concatenate([i["x0"][None], xs[:-1]])            # the state at each tick's start
    n_at = np.concatenate([i["x0_nom"][None], i["xs_nom"][:-1]])
    raw = (x_at - n_at)[:, 1:nq]
    crossing = np.abs(raw) > np.pi                             # opposite sides of the cut: the plain difference is a turn off
    assert crossing.any(axis=(0, 1)).sum() >= 1
    assert crossing[0, :, :2].all()                            # lanes 0 and 1 at tick 0, as drawn
    assert np.abs(lq.wrap_nearest(model, (x_at - n_at)[0])[1:nq, :2]).max() < 0.01   # and the wrapped difference is the small one


@pytest.mark.parametrize("model", ["single", "double"])
def test_tracking_beats_the_open_loop(orc, model):
    x_nom, u_nom, x0, qf = lq.tracking_draws(model, NB)
    dt, T = lq.TRACK_DT, lq.TRACK_T
    nom = lq.lqr_batch(orc, model, sj.DYN[model], dt, x_nom, u_nom, lq.Q[model], lq.R, qf)
    xs_open, _ = lq.closed_loop_batch(orc, model, sj.DYN[model], dt, x0, u_nom, None, None, None)
    xs_fb, us = lq.closed_loop_batch(orc, model, sj.DYN[model], dt, x0, u_nom, nom["K"], x_nom, nom["xs"], 300.0)
    d_open = lq.deviation(model, xs_open[-1], nom["xs"][-1])
    d_fb = lq.deviation(model, xs_fb[-1], nom["xs"][-1])
    print("lqr ref %s tracking over %d ticks: worst closed / open ratio %.3f, open-loop growth at least %.1f x, max |u| %.2f, "
          "max |K| %.1f" % (model, T, (d_fb / d_open).max(), (d_open / lq.TRACK_DELTA).min(), np.abs(us).max(),
                            np.abs(nom["K"]).max()))
    assert (d_open >= lq.TRACK_GROWTH * lq.TRACK_DELTA).all()  # the premise: the open loop does diverge, on every lane
    assert (d_fb <= lq.TRACK_RATIO * d_open).all()
    assert np.abs(us).max() < 300.0                          # the 300 N clamp is idle
