"""The numpy reference of the rollout's forward mode and of the Gauss-Newton normal equations
(tests/helpers/sim_rollout_gn_ref.py) pinned on the CPU.

1. The recurrence S_{t+1} = A_t S_t + P_t over the one-step references' A_t and P_t at the oracle's own checkpoints gives the
   Richardson-extrapolated central differences of the oracle's rollout in each parameter (S_T), and g of the normal equations
   gives those of the cost, within the project's FD_BOUND of the lane's largest entry.  16 lanes of sim_jac_ref.states (lanes
   that wrap inside the first millisecond; for the 4-state model lanes beyond the bumpers), none left out; the recording is
   the nominal trajectory plus uniform +-0.1, with random state weights in [0.5, 2] and per-sample weights in [0, 2].
2. dt = 0: S = 0, g = 0, H = 0 and the cost is the weighted residual of x0.
3. The CPU twin of the GPU identification cases on all 130 lanes: undamped Gauss-Newton on the normal equations with central
   differences of the oracle's rollout recovers every lane's parameters to 1e-9 relative within 8 iterations.

Measured here, worst lane over the six cases of 1: S_T 2.2e-9, g 1.9e-9.  3, worst lane after iterations 1 - 4:
(a) 8.1e-2 1.9e-3 2.8e-7 1.8e-13, (b) 1.1e-1 1.6e-3 1.4e-6 2.6e-11 (9e-12 after), (c) 2.5e-2 7.9e-4 6.3e-7 4.0e-13; cond of the scaled H at
most 1.3e3 / 2.4e4 / 3.3e2.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from helpers import sim_jac_ref as sj
from helpers import sim_param_ref as sp
from helpers import sim_rollout_gn_ref as gn

LANES = 16
CASES = ((0.0105, 5), (0.02, 3), (0.001, 8))
FD_BOUND = 1e-7   # the project's bound for central differences (tests/test_sim_jac_ref.py)
B_IDENT = 130


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
    xs, S = gn.oracle_route_batch(orc, model, prm, dt, x, us)
    x_obs = xs + noise
    _, g, H = gn.normal_equations(S, gn.residuals(orc, model, x_obs, xs), w, om)
    fd_S = np.stack([gn.fd_sensitivity(orc, model, prm, dt, x[:, b], us[:, b]) for b in range(LANES)], axis=-1)
    fd_g = np.stack([gn.fd_cost_gradient(orc, model, prm, dt, x[:, b], us[:, b], x_obs[:, :, b], w, om[:, b])
                     for b in range(LANES)], axis=-1)
    e_S, e_g = sp.lane_err(S[-1], fd_S).max(), sp.lane_err(g, fd_g).max()
    print("sim_rollout_gn_ref %s dt=%g T=%d: recurrence vs Richardson differences, worst lane of %d relative to the lane's "
          "max: S_T %.2e  g %.2e (bound %.0e)" % (model, dt, T, LANES, e_S, e_g, FD_BOUND))
    assert max(e_S, e_g) <= FD_BOUND
    assert np.allclose(H, H.transpose(1, 0, 2), rtol=1e-13, atol=0)   # the same sums in einsum's two orders
    assert (np.linalg.eigvalsh(H.transpose(2, 0, 1)) >= -1e-12 * np.abs(H).max()).all()   # a sum of squares


@pytest.mark.parametrize("model", ["single", "double"])
def test_dt_zero_has_no_sensitivity(orc, model):
    x, us, noise, w, om = _inputs(model, 3)
    xs, S = gn.oracle_route_batch(orc, model, sj.DYN[model], 0.0, x, us)
    x_obs = xs + noise
    r = gn.residuals(orc, model, x_obs, xs)
    cost, g, H = gn.normal_equations(S, r, w, om)
    assert (xs == x[None]).all() and not S.any() and not g.any() and not H.any()
    want = sum(0.5 * om[t] * np.einsum("q,qb,qb->b", w, r[t], r[t]) for t in range(3))
    assert np.allclose(cost, want, rtol=1e-14, atol=0) and (cost > 0).all()


@pytest.mark.parametrize("name", sorted(gn.IDENT_CASES))
def test_cpu_twin_of_the_identification_cases(orc, name):
    model, idx, w = gn.IDENT_CASES[name]
    true, start, x0, us = gn.identification_draws(model, idx, B_IDENT)
    worst, conds = np.zeros(9), []
    for b in range(B_IDENT):
        x_obs = gn.sr.rollout(orc, model, true[:, b], gn.IDENT_DT, x0[:, b], us[:, b])
        its, cond = gn.identify(orc, model, start[:, b], idx, gn.IDENT_DT, x0[:, b], us[:, b], x_obs, w, iterations=8)
        worst = np.maximum(worst, np.abs(its[:, idx] / true[idx, b] - 1.0).max(axis=1))
        conds.append(cond)
    print("identification twin (%s) %s idx %s weights %s: worst lane of %d after iterations 1..8: %s; cond(scaled H) <= %.1e"
          % (name, model, idx, w, B_IDENT, " ".join("%.1e" % e for e in worst[1:]), max(conds)))
    assert worst[1:].min() <= 1e-9 and worst[8] <= 1e-9
