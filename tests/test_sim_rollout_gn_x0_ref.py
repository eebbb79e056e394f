"""The numpy reference of the rollout's forward mode in the initial state and of the normal equations of the fit of x0
(tests/helpers/sim_rollout_gn_x0_ref.py) pinned on the CPU, and the CPU twins that decide the estimation tests' figures.

1. The recurrence Phi_{t+1} = A_t Phi_t over the one-step reference's A_t at the oracle's own checkpoints gives the
   Richardson-extrapolated central differences of the oracle's rollout in each component of x0 (Phi_T), and g of the normal
   equations gives those of the cost, within the project's FD_BOUND of the lane's largest entry.  16 lanes of
   sim_jac_ref.states (lanes that wrap inside the first millisecond; for the 4-state model lanes beyond the bumpers), none left
   out; six (dt, T) cases for each model; the recording is the nominal trajectory plus uniform +-0.1, with random state weights
   in [0.5, 2] and per-sample weights in [0, 2].
2. dt = 0: Phi = I, H = sum om W, g = -sum om W r.
3. The CPU twin of sim_estimate_state on the 130 lanes of the GPU test's three cases: undamped Gauss-Newton from the truth
   +- (0.1 m, 0.1 rad, 0.2 m/s, 0.2 rad/s) -- the full perturbation the issue names, not shrunk -- recovers every lane's x0 to
   1e-9 within 8 iterations.
4. The CPU twin of WindowEstimator: 24 ticks, 64 lanes, a window of 8, noise-free positions, two iterations per tick; the
   worst current-state error from the tick the window is full.  The GPU test's bound is ten times that figure.

Measured here, worst lane: 1, over the twelve cases: Phi_T 6.0e-10, g 1.7e-9.  3, |x0 - truth| after iterations 1 - 4 (and
after 8): (a) 2.6e-2 5.5e-5 3.6e-10 4.0e-15 (1.6e-15), (b) 4.1e-2 7.0e-5 3.8e-10 8.0e-14 (9.0e-14), (c) 1.8e-1 1.0e-3 3.7e-8
1.1e-13 (7.9e-14); cond of the scaled H at most 15 / 34 / 32.  4: 3.42e-14 (helpers: WINDOW_TWIN_WORST = 3.5e-14).  Every test prints its figures before it asserts
(DESIGN.md 5j)."""
import numpy as np
import pytest

from helpers import sim_jac_ref as sj
from helpers import sim_param_ref as sp
from helpers import sim_rollout_gn_x0_ref as gx

LANES = 16
CASES = ((0.0105, 5), (0.02, 3), (0.001, 8), (0.01, 4), (0.0045, 6), (0.0025, 1))
FD_BOUND = 1e-7   # the project's bound for central differences (tests/test_sim_jac_ref.py)
B_EST = 130


def _inputs(model, T):
    x, _ = sj.states(model, LANES)
    rng = np.random.default_rng(41)
    us = rng.uniform(-20.0, 20.0, (T, LANES))
    noise = rng.uniform(-0.1, 0.1, (T, sj.NX[model], LANES))
    w = rng.uniform(0.5, 2.0, sj.NX[model])
    om = rng.uniform(0.0, 2.0, (T, LANES))
    return x, us, noise, w, om


@pytest.mark.parametrize("dt,T", CASES)
@pytest.mark.parametrize("model", ["single", "double"])
def test_recurrence_and_gradient_are_the_differences_of_the_oracles_rollout(orc, model, dt, T):
    x, us, noise, w, om = _inputs(model, T)
    prm = sj.DYN[model]
    xs, Phi = gx.oracle_route_batch(orc, model, prm, dt, x, us)
    x_obs = xs + noise
    _, g, H = gx.normal_equations(Phi, gx.gn.residuals(orc, model, x_obs, xs), w, om)
    fd_Phi = np.stack([gx.fd_transition(orc, model, prm, dt, x[:, b], us[:, b]) for b in range(LANES)], axis=-1)
    fd_g = np.stack([gx.fd_cost_gradient(orc, model, prm, dt, x[:, b], us[:, b], x_obs[:, :, b], w, om[:, b])
                     for b in range(LANES)], axis=-1)
    e_P, e_g = sp.lane_err(Phi[-1], fd_Phi).max(), sp.lane_err(g, fd_g).max()
    print("sim_rollout_gn_x0_ref %s dt=%g T=%d: recurrence vs Richardson differences, worst lane of %d relative to the lane's "
          "max: Phi_T %.2e  g %.2e (bound %.0e)" % (model, dt, T, LANES, e_P, e_g, FD_BOUND))
    assert max(e_P, e_g) <= FD_BOUND
    assert np.allclose(H, H.transpose(1, 0, 2), rtol=0, atol=1e-13 * np.abs(H).max())   # the same sums in einsum's two orders
    assert (np.linalg.eigvalsh(H.transpose(2, 0, 1)) >= -1e-12 * np.abs(H).max()).all()   # a sum of squares


@pytest.mark.parametrize("model", ["single", "double"])
def test_dt_zero_is_the_identity(orc, model):
    x, us, noise, w, om = _inputs(model, 3)
    nx = sj.NX[model]
    xs, Phi = gx.oracle_route_batch(orc, model, sj.DYN[model], 0.0, x, us)
    x_obs = xs + noise
    r = gx.gn.residuals(orc, model, x_obs, xs)
    cost, g, H = gx.normal_equations(Phi, r, w, om)
    assert (xs == x[None]).all() and (Phi == np.eye(nx)[None, :, :, None]).all()
    assert np.allclose(H, np.einsum("tb,jk->jkb", om, np.diag(w)), rtol=1e-14, atol=0)
    assert np.allclose(g, -np.einsum("tb,q,tqb->qb", om, w, r), rtol=1e-13, atol=1e-16)
    assert (cost > 0).all()


@pytest.mark.parametrize("name", sorted(gx.EST_CASES))
def test_cpu_twin_of_the_estimation_cases(orc, name):
    model, w = gx.EST_CASES[name]
    truth, start, us = gx.estimation_draws(model, B_EST)
    prm = sj.DYN[model]
    worst, conds = np.zeros(9), []
    for b in range(B_EST):
        x_obs = gx.sr.rollout(orc, model, prm, gx.EST_DT, truth[:, b], us[:, b])
        its, _ = gx.estimate(orc, model, prm, gx.EST_DT, start[:, b], us[:, b], x_obs, w, iterations=8)
        worst = np.maximum(worst, np.abs(its - truth[:, b]).max(axis=1))
        _, _, H, _ = gx.normal_equations_at(orc, model, prm, gx.EST_DT, truth[:, b], us[:, b], x_obs, w)
        d = 1.0 / np.sqrt(np.diag(H))
        conds.append(float(np.linalg.cond(H * d[:, None] * d[None, :])))
    print("estimation twin (%s) %s weights %s, start = truth +- %s: worst lane of %d |x0 - truth| after iterations 0..8: %s; "
          "cond(scaled H) <= %.1e" % (name, model, w, gx.perturbation(model), B_EST, " ".join("%.1e" % e for e in worst),
                                       max(conds)))
    assert worst[8] <= 1e-9


def test_arrival_cost_alone_returns_the_prior(orc):
    """every tick weight 0 and prior_info = 1: the fit is the arrival cost, one step lands on the prior, H is Pi"""
    model = "single"
    truth, start, us = gx.estimation_draws(model, 4)
    for b in range(4):
        x_obs = gx.sr.rollout(orc, model, sj.DYN[model], gx.EST_DT, truth[:, b], us[:, b])
        its, _ = gx.estimate(orc, model, sj.DYN[model], gx.EST_DT, start[:, b], us[:, b], x_obs, None, om=np.zeros(gx.EST_T),
                             iterations=1, prior=truth[:, b], prior_info=np.ones(4))
        assert np.abs(its[1] - truth[:, b]).max() <= 4 * np.finfo(np.float64).eps * np.abs(truth[:, b]).max()
        _, _, H, _ = gx.normal_equations_at(orc, model, sj.DYN[model], gx.EST_DT, its[1], us[:, b], x_obs, None, np.zeros(gx.EST_T),
                                            truth[:, b], np.ones(4))
        assert (H == np.eye(4)).all()


def test_cpu_twin_of_the_window_estimator(orc):
    worst = gx.window_twin_figure(orc)
    print("window twin: %d lanes, %d ticks, window %d, %d iterations a tick, positions only: worst |current state - truth| from "
          "the tick the window is full %.2e" % (gx.WINDOW_B, gx.WINDOW_TICKS, gx.WINDOW_T, gx.WINDOW_ITERATIONS, worst))
    assert worst <= gx.WINDOW_TWIN_WORST
