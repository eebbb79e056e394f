"""Numpy reference for the plant step with its first derivatives (include/cpmpc.h: cpmpc_sim_step_jac_batch), built on the
CPU oracle's own per-sub-step RK4 Jacobians.  TEST INFRASTRUCTURE ONLY.

  sub_steps     the host's sub-step sequence of a step of length dt (simulator.cc:18-22 in double: 1 ms, a shorter last one)
  step_ref      x+, A = dx+/dx, B = dx+/du of one problem: per sub-step orc.rk4_model (orc.rk4 with external forces), the pole
                angles wrapped with orc.mod_pi, A <- A_i A, B <- A_i B + B_i (the control is held; the wrap has unit derivative)
  step_ref_batch  the same for [nx, B] states
  fd_jacobians  central differences of orc.sim_step_model, angle differences wrapped
  states        the seeded test states: the simulator test's distribution, with a block of lanes that wrap inside the step
                and, for the 4-state model, a block beyond the bumpers"""
import numpy as np

DYN = {"single": [1.0, 0.1, 0.25, 9.81, 0.03, 0.1, 0.13, 0.8, 100.0],   # optimization_test.cc:20 (conftest.DYN_TEST)
       "double": [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]}                       # m_b, m_1, m_2, l_1, l_2, g (test_gpu_double.DYN)
NX = {"single": 4, "double": 6}
BUMPER_X = 0.8   # x_s of DYN["single"]


def sub_steps(dt):
    hs, rem = [], float(dt)
    while rem > 0.0:
        hs.append(min(rem, 0.001))
        rem -= 0.001
    return hs


def _wrap(orc, model, x):
    nq = NX[model] // 2
    for t in range(1, nq):
        x[t] = orc.mod_pi(x[t])
    return x


def step_ref(orc, model, params, dt, x, u, f_base=None, f_mass=None):
    nx = NX[model]
    x = np.array(x, dtype=np.float64)
    A, B = np.eye(nx), np.zeros(nx)
    for h in sub_steps(dt):
        if f_base is None and f_mass is None:
            x, Ai, Bi = orc.rk4_model(model, params, x, u, h)
        else:
            assert model == "single"
            x, Ai, Bi = orc.rk4(params, x, u, h, f_base, f_mass)
        x = _wrap(orc, model, x)
        A = Ai @ A
        B = Ai @ B + Bi
    return x, A, B


def step_ref_batch(orc, model, params, dt, x, u, fext=None):
    """x [nx, B], u [B], fext None, 4 shared values or [4, B] -> x+ [nx, B], A [nx, nx, B], Bu [nx, B]."""
    nx, nb = x.shape
    xn, A, Bu = np.zeros((nx, nb)), np.zeros((nx, nx, nb)), np.zeros((nx, nb))
    for b in range(nb):
        fb = fm = None
        if fext is not None:
            f = np.asarray(fext, dtype=np.float64)
            f = f[:, b] if f.ndim == 2 else f
            fb, fm = f[:2], f[2:]
        xn[:, b], A[:, :, b], Bu[:, b] = step_ref(orc, model, params, dt, x[:, b], u[b], fb, fm)
    return xn, A, Bu


def wrapped_diff(orc, model, a, b):
    d = np.array(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return _wrap(orc, model, d)


def fd_jacobians(orc, model, params, dt, x, u, hx=1e-6, hu=1e-4):
    nx = NX[model]
    x = np.asarray(x, dtype=np.float64)
    A, B = np.zeros((nx, nx)), np.zeros(nx)
    for c in range(nx):
        e = np.zeros(nx)
        e[c] = hx
        A[:, c] = wrapped_diff(orc, model, orc.sim_step_model(model, params, dt, u, x + e),
                               orc.sim_step_model(model, params, dt, u, x - e)) / (2 * hx)
    B[:] = wrapped_diff(orc, model, orc.sim_step_model(model, params, dt, u + hu, x),
                        orc.sim_step_model(model, params, dt, u - hu, x)) / (2 * hu)
    return A, B


def random_lanes(rng, model, nb):
    """b_x +-0.5, angles anywhere in (-pi, pi], velocities +-2, u +-50."""
    nq = NX[model] // 2
    x = np.concatenate([rng.uniform(-0.5, 0.5, (1, nb)), rng.uniform(-np.pi, np.pi, (nq - 1, nb)),
                        rng.uniform(-2.0, 2.0, (nq, nb))])
    return x, rng.uniform(-50.0, 50.0, nb)


def states(model, nb, seed=9):
    """The simulator test's states (test_gpu_parity.test_simulator_matches_oracle) for nb lanes: b_x +-0.6, angles anywhere,
    b_x' +-1, angle rates +-3, u +-20; lanes [0, nb/4) with every pole at theta in [2.9, 3.14] and theta' in [2, 6] (the wrap
    happens inside the step; for lanes 0 and 1 inside its first millisecond); for the 4-state model lanes [nb/4, nb/2) with
    |b_x| in [0.85, 1.2], beyond the bumpers."""
    rng = np.random.default_rng(seed + NX[model])
    nq = NX[model] // 2
    x = np.concatenate([rng.uniform(-0.6, 0.6, (1, nb)), rng.uniform(-np.pi, np.pi, (nq - 1, nb)),
                        rng.uniform(-1.0, 1.0, (1, nb)), rng.uniform(-3.0, 3.0, (nq - 1, nb))])
    k = max(nb // 4, 1)
    x[1:nq, :k] = rng.uniform(2.9, 3.14, (nq - 1, k))
    x[nq + 1:, :k] = rng.uniform(2.0, 6.0, (nq - 1, k))
    if nb >= 8:
        x[1:nq, :2] = 3.1414   # 1.9e-4 rad below pi at 2 rad/s or more: these two wrap inside the first sub-step of any dt
    if model == "single" and nb >= 4:
        x[0, k:2 * k] = rng.uniform(BUMPER_X + 0.05, 1.2, k) * rng.choice([-1.0, 1.0], k)
    return x, rng.uniform(-20.0, 20.0, nb)
