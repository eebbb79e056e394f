"""The numpy reference of the plant rollout and its adjoint (tests/helpers/sim_rollout_ref.py) pinned on the CPU: the
adjoint recurrence over the one-step references' A_t, Bu_t, P_t gives the Richardson-extrapolated central differences of
the whole rollout's loss  sum_t gbar_t . wrapped_diff(x_{t+1}, x_{t+1}^nom)  on the oracle, in x0, in the T controls and in
the parameters, within the project's FD_BOUND of each lane's max |entry| of that output; dt = 0 is the identity; T = 1 is
the one-step reference.  16 lanes of sim_jac_ref.states (lanes that wrap inside the first millisecond, and for the 4-state
model lanes beyond the bumpers), all of them counted.  CPU only.

Measured here, worst lane over the six cases, g_x0 / g_u / g_p: 9.2e-10 / 4.3e-9 / 2.2e-9; every test prints its figures
before it asserts."""
import numpy as np
import pytest

from helpers import sim_jac_ref as sj
from helpers import sim_param_ref as sp
from helpers import sim_rollout_ref as sr

LANES = 16
CASES = ((0.0105, 5), (0.02, 3), (0.001, 8))
FD_BOUND = 1e-7   # the project's bound for central differences (tests/test_sim_jac_ref.py)


def _inputs(model, T):
    x, _ = sj.states(model, LANES)
    rng = np.random.default_rng(41)
    us = rng.uniform(-20.0, 20.0, (T, LANES))
    gb = rng.uniform(-1.0, 1.0, (T, sj.NX[model], LANES))
    return x, us, gb


@pytest.mark.parametrize("dt,T", CASES)
@pytest.mark.parametrize("model", ["single", "double"])
def test_adjoint_is_the_gradient_of_the_rollout_loss(orc, model, dt, T):
    x, us, gb = _inputs(model, T)
    _, g_x0, g_u, g_p = sr.adjoint_batch(orc, model, sj.DYN[model], dt, x, us, gbar=gb)
    f_x0, f_u, f_p = sr.fd_gradients_batch(orc, model, sj.DYN[model], dt, x, us, gb)
    errs = [sp.lane_err(g, f).max() for g, f in ((g_x0, f_x0), (g_u, f_u), (g_p, f_p))]
    print("sim_rollout_ref %s dt=%g T=%d: adjoint vs Richardson differences of the loss, worst lane of %d, relative to the "
          "lane's max: g_x0 %.2e  g_u %.2e  g_p %.2e (bound %.0e)" % (model, dt, T, LANES, *errs, FD_BOUND))
    assert max(errs) <= FD_BOUND


@pytest.mark.parametrize("model", ["single", "double"])
def test_dt_zero_is_the_identity(orc, model):
    x, us, gb = _inputs(model, 3)
    gf = gb[0] * 0.5
    xs, g_x0, g_u, g_p = sr.adjoint_batch(orc, model, sj.DYN[model], 0.0, x, us, gbar=gb, gbar_final=gf)
    for t in range(3):
        assert (xs[t] == x).all()
    assert np.array_equal(g_x0, ((gb[2] + gf) + gb[1]) + gb[0])
    assert not g_u.any() and not g_p.any()


@pytest.mark.parametrize("model", ["single", "double"])
def test_one_tick_is_the_one_step_reference(orc, model):
    dt = 0.0105
    x, us, gb = _inputs(model, 1)
    xs, g_x0, g_u, g_p = sr.adjoint_batch(orc, model, sj.DYN[model], dt, x, us, gbar_final=gb[0])
    xn, A, Bu = sj.step_ref_batch(orc, model, sj.DYN[model], dt, x, us[0])
    P = sp.param_jacobian_batch(orc, model, sj.DYN[model], dt, x, us[0])
    # the step references integrate with the oracle's RK4 pieces, the rollout with its simulator: 1e-12, the suite's
    # tolerance between the two
    assert max(np.abs(sj.wrapped_diff(orc, model, xs[0][:, b], xn[:, b])).max() for b in range(LANES)) <= 1e-12
    # one level of the recurrence, and the batched recurrence on given matrices (the GPU tests' form): the same sums in
    # another order, 1e-13 of the output's max
    r_x0, r_u, r_p = sr.recurrence(A[None], Bu[None], P[None], gbar_final=gb[0])
    assert np.allclose(r_x0, np.einsum("rcb,rb->cb", A, gb[0]), rtol=0, atol=1e-13 * np.abs(g_x0).max())
    assert np.allclose(r_x0, g_x0, rtol=0, atol=1e-13 * np.abs(g_x0).max())
    assert np.allclose(r_u, g_u, rtol=0, atol=1e-13 * np.abs(g_u).max())
    assert np.allclose(r_p, g_p, rtol=0, atol=1e-13 * np.abs(g_p).max())
