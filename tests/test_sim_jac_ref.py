"""The numpy reference of the plant step's Jacobians (tests/helpers/sim_jac_ref.py) pinned on the CPU: its state is the
oracle simulator's exactly, and its A, B are central differences of the oracle simulator.  CPU only."""
import numpy as np
import pytest

from helpers import sim_jac_ref as sj

LANES = 32
DTS = (0.01, 0.0105, 0.02)
# central differences with a state step of 1e-6 and a control step of 1e-4, relative to max |A| / max |B|.  Measured on
# these lanes: 1.9e-9 (A) and 1.6e-9 (B) at worst; the bound is about 50 times that because finite differences are noisy.
FD_BOUND = 1e-7


def test_sub_steps_are_the_hosts():
    assert sj.sub_steps(0.0) == []
    assert sj.sub_steps(0.001) == [0.001]
    hs = sj.sub_steps(0.0025)
    assert len(hs) == 3 and hs[:2] == [0.001, 0.001] and abs(hs[2] - 0.0005) < 1e-15
    assert len(sj.sub_steps(0.0105)) == 11 and len(sj.sub_steps(0.02)) in (20, 21)


@pytest.mark.parametrize("model", ["single", "double"])
def test_reference_state_is_the_oracle_simulators(orc, model):
    x, u = sj.random_lanes(np.random.default_rng(11), model, LANES)
    for dt in DTS:
        worst = 0.0
        for b in range(LANES):
            xn, _, _ = sj.step_ref(orc, model, sj.DYN[model], dt, x[:, b], u[b])
            worst = max(worst, np.abs(xn - orc.sim_step_model(model, sj.DYN[model], dt, u[b], x[:, b])).max())
        assert worst == 0.0, (model, dt, worst)


@pytest.mark.parametrize("model", ["single", "double"])
def test_reference_jacobians_are_the_simulators_derivatives(orc, model):
    x, u = sj.random_lanes(np.random.default_rng(11), model, LANES)
    worst_a = worst_b = 0.0
    for dt in DTS:
        for b in range(LANES):
            _, A, B = sj.step_ref(orc, model, sj.DYN[model], dt, x[:, b], u[b])
            An, Bn = sj.fd_jacobians(orc, model, sj.DYN[model], dt, x[:, b], u[b])
            worst_a = max(worst_a, np.abs(A - An).max() / np.abs(A).max())
            worst_b = max(worst_b, np.abs(B - Bn).max() / np.abs(B).max())
    print("sim_jac_ref vs central differences, %s: A %.2e  B %.2e" % (model, worst_a, worst_b))
    assert worst_a <= FD_BOUND and worst_b <= FD_BOUND, (worst_a, worst_b)


def test_dt_zero_is_the_identity(orc):
    x, u = sj.random_lanes(np.random.default_rng(3), "single", 2)
    xn, A, B = sj.step_ref(orc, "single", sj.DYN["single"], 0.0, x[:, 0], u[0])
    assert np.array_equal(xn, x[:, 0]) and np.array_equal(A, np.eye(4)) and not B.any()


def test_forces_enter_the_single_model(orc):
    """orc.rk4 with zero forces is orc.rk4_model; with forces the step differs and the reference follows the oracle's
    simulator."""
    x, u = sj.random_lanes(np.random.default_rng(5), "single", 4)
    for b in range(4):
        a = sj.step_ref(orc, "single", sj.DYN["single"], 0.0025, x[:, b], u[b])
        z = sj.step_ref(orc, "single", sj.DYN["single"], 0.0025, x[:, b], u[b], (0.0, 0.0), (0.0, 0.0))
        for p, q in zip(a, z):
            assert np.array_equal(p, q)
        f = sj.step_ref(orc, "single", sj.DYN["single"], 0.0025, x[:, b], u[b], (2.0, 0.0), (0.5, -1.0))
        o = orc.Simulator()
        o.set_state(x[:, b])
        o.step(sj.DYN["single"], 0.0025, u[b], (2.0, 0.0), (0.5, -1.0))
        assert np.array_equal(f[0], o.get_state()) and not np.array_equal(f[0], a[0])
