"""Numpy reference for the rollout's forward mode in the initial state and the Gauss-Newton normal equations of the fit of x0
over a window (include/cpmpc.h: cpmpc_sim_rollout_gn_x0_batch), and CPU twins of sim_estimate_state and WindowEstimator, built
on the CPU oracle and the one-step reference of sim_jac_ref.  float64 throughout.  TEST INFRASTRUCTURE ONLY.

  transitions       Phi [T, nx, nx, B], Phi[t] = dxs[t]/dx0: the recurrence Phi_{t+1} = A_t Phi_t from Phi_0 = I on given per-tick
                    matrices A [T, nx, nx, B] (the GPU tests feed it sim_step_jacobian's, and their absolute values for the bound)
  normal_equations  sim_rollout_gn_ref.normal_equations on Phi in the place of S: cost [B], g [nx, B], H [nx, nx, B]
  oracle_route      one problem: the oracle's rollout and A_t from sim_jac_ref.step_ref at the oracle's own checkpoints
                    -> xs [T, nx], Phi [T, nx, nx]; oracle_route_batch the same for [nx, B] states
  fd_transition     dxs[T-1]/dx0 [nx, nx] of one problem: Richardson central differences of the oracle's rollout in each
                    component of x0, sim_rollout_ref's step (h = 1e-5)
  cost / fd_cost_gradient  the fit's cost on the oracle's rollout and its Richardson central differences in x0
  normal_equations_at  one problem: cost, g, H, x_final at a trial x0, with the arrival cost where a prior is given
  estimate          one problem: the twin of sim_estimate_state, undamped -> the iterates [iterations + 1, nx], x_final
  window_estimates  one problem: the twin of WindowEstimator fed tick by tick -> the current-state estimate after every tick"""
import numpy as np

from helpers import sim_jac_ref as sj
from helpers import sim_rollout_gn_ref as gn
from helpers import sim_rollout_ref as sr

normal_equations = gn.normal_equations


def transitions(A):
    T, nx, _, nb = A.shape
    Phi = np.zeros((T, nx, nx, nb))
    cur = np.tile(np.eye(nx)[:, :, None], (1, 1, nb))
    for t in range(T):
        cur = np.einsum("rcb,cjb->rjb", A[t], cur)
        Phi[t] = cur
    return Phi


def oracle_route(orc, model, params, dt, x0, us, fext=None):
    nx, T = sj.NX[model], len(us)
    xs = sr.rollout(orc, model, params, dt, x0, us, fext)
    fb, fm = (None, None) if fext is None else (fext[:2], fext[2:])
    A = np.zeros((T, nx, nx, 1))
    for t in range(T):
        xt = np.asarray(x0, dtype=np.float64) if t == 0 else xs[t - 1]
        _, A[t, :, :, 0], _ = sj.step_ref(orc, model, params, dt, xt, float(us[t]), fb, fm)
    return xs, transitions(A)[..., 0]


def oracle_route_batch(orc, model, params, dt, x0, us, fext=None):
    """x0 [nx, B], us [T, B], params np numbers or [np, B] -> xs [T, nx, B], Phi [T, nx, nx, B]"""
    nx, nb = x0.shape
    T = us.shape[0]
    xs, Phi = np.zeros((T, nx, nb)), np.zeros((T, nx, nx, nb))
    for b in range(nb):
        xs[:, :, b], Phi[..., b] = oracle_route(orc, model, sr._params(params, b), dt, x0[:, b], us[:, b], sr._lane(fext, b))
    return xs, Phi


def _bumped(x, i, h):
    y = np.array(x, dtype=np.float64)
    y[i] += h
    return y


def fd_transition(orc, model, params, dt, x0, us, fext=None):
    nx = sj.NX[model]
    nom = sr.rollout(orc, model, params, dt, x0, us, fext)[-1]
    Phi = np.zeros((nx, nx))
    for c in range(nx):
        Phi[:, c] = gn._richardson(lambda e, c=c: sj.wrapped_diff(orc, model, sr.rollout(orc, model, params, dt, _bumped(x0, c, e),
                                                                                          us, fext)[-1], nom), sr.H_STATE)
    return Phi


def cost(orc, model, params, dt, x0, us, x_obs, w=None, om=None, fext=None):
    return gn.cost(orc, model, params, dt, x0, us, x_obs, w, om, fext)


def fd_cost_gradient(orc, model, params, dt, x0, us, x_obs, w=None, om=None, fext=None):
    return np.array([gn._richardson(lambda e, c=c: cost(orc, model, params, dt, _bumped(x0, c, e), us, x_obs, w, om, fext),
                                    sr.H_STATE) for c in range(sj.NX[model])])


def wrap_state_diff(model, d):
    """a difference of states with its pole angles to the nearest multiple of 2 pi"""
    d = np.array(d, dtype=np.float64)
    nq = sj.NX[model] // 2
    d[1:nq] -= 2 * np.pi * np.round(d[1:nq] / (2 * np.pi))
    return d


def normal_equations_at(orc, model, params, dt, x0, us, x_obs, w=None, om=None, prior=None, prior_info=None):
    """-> cost, g [nx], H [nx, nx], x_final [nx] of one problem at x0; prior_info [nx] (a diagonal) or [nx, nx]"""
    xs, Phi = oracle_route(orc, model, params, dt, x0, us)
    r = gn.residuals(orc, model, np.asarray(x_obs)[:, :, None], xs[:, :, None])
    c, g, H = normal_equations(Phi[..., None], r, w, None if om is None else np.asarray(om)[:, None])
    c, g, H = float(c[0]), g[:, 0], H[:, :, 0]
    if prior is not None:
        Pi = np.diag(prior_info) if np.ndim(prior_info) == 1 else np.asarray(prior_info)
        d = wrap_state_diff(model, np.asarray(x0) - prior)
        c, g, H = c + 0.5 * d @ Pi @ d, g + Pi @ d, H + Pi
    return c, g, H, xs[-1]


def positive_definite(H):
    d = np.diag(H)
    if not (d > 0).all():
        return False
    s = 1.0 / np.sqrt(d)
    try:
        L = np.linalg.cholesky(H * s[:, None] * s[None, :])
    except np.linalg.LinAlgError:
        return False
    return bool((np.diag(L) ** 2 > 8 * len(d) * np.finfo(np.float64).eps).all())


def estimate(orc, model, params, dt, start, us, x_obs, w=None, om=None, iterations=8, prior=None, prior_info=None):
    """undamped Gauss-Newton from `start`, every step taken -> the iterates [iterations + 1, nx] and x_final at the last one.
    As sim_estimate_state, a problem whose diagonally scaled H has a Cholesky pivot at or below 8 nx eps (the window does not
    determine x0) stops and keeps what it has."""
    x0 = np.array(start, dtype=np.float64)
    out = [x0.copy()]
    _, g, H, xf = normal_equations_at(orc, model, params, dt, x0, us, x_obs, w, om, prior, prior_info)
    for _ in range(iterations):
        if not positive_definite(H):
            out += [x0.copy()] * (iterations + 1 - len(out))
            break
        x0 = x0 - np.linalg.solve(H, g)
        _, g, H, xf = normal_equations_at(orc, model, params, dt, x0, us, x_obs, w, om, prior, prior_info)
        out.append(x0.copy())
    return np.array(out), xf


def window_estimates(orc, model, params, dt, guess, us, ys, window, w=None, iterations=2):
    """The twin of WindowEstimator for one problem: push(us[t], ys[t]) then estimate(iterations) for every tick t; the guess
    of the window's first state moves one plant tick on whenever a full window drops its oldest tick.
    -> the current-state estimates [len(us), nx]"""
    x0 = np.array(guess, dtype=np.float64)
    out = np.zeros((len(us), sj.NX[model]))
    for t in range(len(us)):
        lo = max(0, t + 1 - window)
        if t + 1 > window:
            x0 = sr.rollout(orc, model, params, dt, x0, us[lo - 1:lo])[-1]
        its, out[t] = estimate(orc, model, params, dt, x0, us[lo:t + 1], ys[lo:t + 1], w, iterations=iterations)
        x0 = its[-1]
    return out


# the estimation cases of the GPU test and of its CPU twin: (model, state weights or None)
EST_CASES = {"a": ("single", None),                                # every state measured
             "b": ("single", (1.0, 1.0, 0.0, 0.0)),                 # positions only
             "c": ("double", (1.0, 1.0, 1.0, 0.0, 0.0, 0.0))}       # positions only
EST_DT, EST_T = 0.0105, 8
# the start of the fit: the truth +- (0.1 m, 0.1 rad, 0.2 m/s, 0.2 rad/s), the sign drawn per entry.  Decided on the CPU twin
# (tests/test_sim_rollout_gn_x0_ref.py, where the figures are): the full perturbation converges in 8 undamped iterations.
EST_PERTURBATION = {"position": 0.1, "angle": 0.1, "velocity": 0.2, "rate": 0.2}


def perturbation(model):
    nq = sj.NX[model] // 2
    p = EST_PERTURBATION
    return np.array([p["position"]] + [p["angle"]] * (nq - 1) + [p["velocity"]] + [p["rate"]] * (nq - 1))


def estimation_draws(model, nb, T=EST_T, seed=23):
    """-> truth x0 [nx, nb], the starting guess [nx, nb], us [T, nb]; the recording is the rollout from the truth"""
    rng = np.random.default_rng(seed)
    x0, _ = sj.random_lanes(rng, model, nb)
    us = rng.uniform(-20.0, 20.0, (T, nb))
    start = x0 + perturbation(model)[:, None] * rng.choice([-1.0, 1.0], x0.shape)
    return x0, start, us


WINDOW_B, WINDOW_TICKS, WINDOW_T, WINDOW_ITERATIONS = 64, 24, 8, 2
# what window_twin_figure returns on these draws (3.42e-14, rounded up): tests/test_sim_rollout_gn_x0_ref.py holds the twin to
# it, and the GPU test holds WindowEstimator to ten times it without running the twin again (17 s of CPU)
WINDOW_TWIN_WORST = 3.5e-14


def window_draws(model="single", nb=WINDOW_B, ticks=WINDOW_TICKS, seed=29):
    """-> truth x0 [nx, nb], the first guess [nx, nb] (the truth perturbed as above), us [ticks, nb]"""
    return estimation_draws(model, nb, ticks, seed)


def window_twin_figure(orc):
    """The worst current-state error of the WindowEstimator twin from the tick its window is full (the GPU test multiplies it
    by 10): positions only, two iterations per tick."""
    model = "single"
    truth, guess, us = window_draws(model)
    w = EST_CASES["b"][1]
    worst = 0.0
    for b in range(WINDOW_B):
        xs = sr.rollout(orc, model, sj.DYN[model], EST_DT, truth[:, b], us[:, b])
        est = window_estimates(orc, model, sj.DYN[model], EST_DT, guess[:, b], us[:, b], xs, WINDOW_T, w,
                                  WINDOW_ITERATIONS)
        err = np.abs(np.array([wrap_state_diff(model, e - x) for e, x in zip(est, xs)])).max(axis=1)
        worst = max(worst, err[WINDOW_T - 1:].max())
    return worst
