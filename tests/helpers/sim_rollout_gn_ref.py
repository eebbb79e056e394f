"""Numpy reference for the rollout's forward mode in the parameters and the Gauss-Newton normal equations of a window
(include/cpmpc.h: cpmpc_sim_rollout_gn_batch), built on the CPU oracle and the one-step references.  float64 throughout.
TEST INFRASTRUCTURE ONLY.

  sensitivities     S [T, nx, np, B], S[t] = dxs[t]/dp: the recurrence S_{t+1} = A_t S_t + P_t from S_0 = 0 on given per-tick
                    matrices A [T, nx, nx, B], P [T, nx, np, B] (the GPU tests feed it the one-tick calls' matrices, and their
                    absolute values for the error bound)
  normal_equations  cost [B], g [np, B], H [np, np, B] from S, the residuals r [T, nx, B], the state weights w [nx] and the
                    per-sample weights om [T, B]:  cost = 1/2 sum om r^T W r,  g = -sum om S^T W r,  H = sum om S^T W S
  residuals         r [T, nx, B] = wrapped_diff(x_obs[t], xs[t]) per lane
  oracle_route      one problem: the oracle's rollout, A_t from sim_jac_ref.step_ref and P_t from sim_param_ref.param_jacobian at
                    the oracle's own checkpoints -> xs [T, nx], S [T, nx, np]; oracle_route_batch the same for [nx, B] states
  fd_sensitivity    dxs[T-1]/dp [nx, np] of one problem: Richardson central differences of the oracle's rollout in each
                    parameter, sim_rollout_ref's step sizes (h = 1e-4 max(|p_j|, 1e-3))
  cost / fd_cost_gradient  the fit's cost on the oracle's rollout and its Richardson central differences in each parameter
  identify          one problem: undamped Gauss-Newton on the normal equations H d = J^T W r with J by central differences of
                    the oracle's rollout in the chosen parameters -> the iterates"""
import numpy as np

from helpers import sim_jac_ref as sj
from helpers import sim_param_ref as sp
from helpers import sim_rollout_ref as sr


def sensitivities(A, P):
    T, nx, npar, nb = P.shape
    S = np.zeros((T, nx, npar, nb))
    cur = np.zeros((nx, npar, nb))
    for t in range(T):
        cur = np.einsum("rcb,cjb->rjb", A[t], cur) + P[t]
        S[t] = cur
    return S


def normal_equations(S, r, w=None, om=None):
    T, nx, npar, nb = S.shape
    w = np.ones(nx) if w is None else np.asarray(w, dtype=np.float64)
    om = np.ones((T, nb)) if om is None else np.asarray(om, dtype=np.float64)
    wr = w[None, :, None] * r
    cost = 0.5 * np.einsum("tb,tqb,tqb->b", om, wr, r)
    g = -np.einsum("tb,tqjb,tqb->jb", om, S, wr)
    H = np.einsum("tb,tqjb,q,tqkb->jkb", om, S, w, S)
    return cost, g, H


def residuals(orc, model, x_obs, xs):
    """x_obs, xs [T, nx, B] -> wrapped x_obs - xs"""
    r = np.zeros_like(xs)
    for t in range(xs.shape[0]):
        for b in range(xs.shape[2]):
            r[t, :, b] = sj.wrapped_diff(orc, model, x_obs[t, :, b], xs[t, :, b])
    return r


def oracle_route(orc, model, params, dt, x0, us, fext=None):
    nx, npar, T = sj.NX[model], sp.NP[model], len(us)
    xs = sr.rollout(orc, model, params, dt, x0, us, fext)
    fb, fm = (None, None) if fext is None else (fext[:2], fext[2:])
    A, P = np.zeros((T, nx, nx, 1)), np.zeros((T, nx, npar, 1))
    for t in range(T):
        xt = np.asarray(x0, dtype=np.float64) if t == 0 else xs[t - 1]
        _, A[t, :, :, 0], _ = sj.step_ref(orc, model, params, dt, xt, float(us[t]), fb, fm)
        if sj.sub_steps(dt):
            P[t, :, :, 0] = sp.param_jacobian(orc, model, params, dt, xt, float(us[t]), fext=fext)
    return xs, sensitivities(A, P)[..., 0]


def oracle_route_batch(orc, model, params, dt, x0, us, fext=None):
    """x0 [nx, B], us [T, B], params np numbers or [np, B] -> xs [T, nx, B], S [T, nx, np, B]"""
    nx, nb = x0.shape
    T = us.shape[0]
    xs, S = np.zeros((T, nx, nb)), np.zeros((T, nx, sp.NP[model], nb))
    for b in range(nb):
        xs[:, :, b], S[..., b] = oracle_route(orc, model, sr._params(params, b), dt, x0[:, b], us[:, b], sr._lane(fext, b))
    return xs, S


def _richardson(f, h):
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * d2 - d1) / 3.0


def _bumped(prm, j, h):
    q = np.array(prm, dtype=np.float64)
    q[j] += h
    return q


def fd_sensitivity(orc, model, params, dt, x0, us, fext=None):
    nx, npar = sj.NX[model], sp.NP[model]
    prm = np.asarray(params, dtype=np.float64)
    nom = sr.rollout(orc, model, prm, dt, x0, us, fext)[-1]
    S = np.zeros((nx, npar))
    for j in range(npar):
        h = sr.REL_PARAM * max(abs(float(prm[j])), 1e-3)
        S[:, j] = _richardson(lambda e, j=j: sj.wrapped_diff(orc, model, sr.rollout(orc, model, _bumped(prm, j, e), dt, x0, us,
                                                                                     fext)[-1], nom), h)
    return S


def cost(orc, model, params, dt, x0, us, x_obs, w=None, om=None, fext=None):
    """one problem: x_obs [T, nx], om [T]"""
    xs = sr.rollout(orc, model, params, dt, x0, us, fext)
    w = np.ones(sj.NX[model]) if w is None else np.asarray(w, dtype=np.float64)
    total = 0.0
    for t in range(len(us)):
        r = sj.wrapped_diff(orc, model, x_obs[t], xs[t])
        total += 0.5 * (1.0 if om is None else float(om[t])) * float(r @ (w * r))
    return total


def fd_cost_gradient(orc, model, params, dt, x0, us, x_obs, w=None, om=None, fext=None):
    prm = np.asarray(params, dtype=np.float64)
    return np.array([_richardson(lambda e, j=j: cost(orc, model, _bumped(prm, j, e), dt, x0, us, x_obs, w, om, fext),
                                 sr.REL_PARAM * max(abs(float(prm[j])), 1e-3)) for j in range(sp.NP[model])])


def identify(orc, model, start, idx, dt, x0, us, x_obs, w=None, iterations=8):
    """-> the iterates [iterations + 1, np] of one problem and the condition number of the diagonally scaled H at the start"""
    nx, T = sj.NX[model], len(us)
    w = np.ones(nx) if w is None else np.asarray(w, dtype=np.float64)
    prm = np.array(start, dtype=np.float64)
    out, cond = [prm.copy()], None
    for _ in range(iterations):
        xs = sr.rollout(orc, model, prm, dt, x0, us)
        r = np.concatenate([sj.wrapped_diff(orc, model, x_obs[t], xs[t]) for t in range(T)])
        J = np.zeros((T * nx, len(idx)))
        for c, j in enumerate(idx):
            h = sr.REL_PARAM * max(abs(float(prm[j])), 1e-3)
            hi = sr.rollout(orc, model, _bumped(prm, j, h), dt, x0, us)
            lo = sr.rollout(orc, model, _bumped(prm, j, -h), dt, x0, us)
            J[:, c] = np.concatenate([sj.wrapped_diff(orc, model, hi[t], lo[t]) for t in range(T)]) / (2 * h)
        W = np.tile(w, T)
        H = J.T @ (W[:, None] * J)
        if cond is None:
            d = 1.0 / np.sqrt(np.diag(H))
            cond = float(np.linalg.cond(H * d[:, None] * d[None, :]))
        prm[idx] += np.linalg.solve(H, J.T @ (W * r))
        out.append(prm.copy())
    return np.array(out), cond


# the identification cases of the GPU test and of its CPU twin: (model, parameter indices, state weights or None)
IDENT_CASES = {"a": ("single", [1, 2, 4], None),                       # m_1, l_1, mu_b; every state observed
               "b": ("single", [1, 2, 4], (1.0, 1.0, 0.0, 0.0)),        # the same, velocities never seen
               "c": ("double", [1, 3, 4], None)}
IDENT_DT, IDENT_T = 0.0105, 8


def identification_draws(model, idx, nb, T=IDENT_T):
    """-> true [np, nb] (DYN with the idx rows scaled by up to +-10 %), start [np, nb] (DYN), x0 [nx, nb], us [T, nb]; the
    recording is the rollout under `true`"""
    rng = np.random.default_rng(17)
    start = np.tile(np.array(sj.DYN[model], dtype=np.float64)[:, None], (1, nb))
    true = start.copy()
    true[idx] *= rng.uniform(0.9, 1.1, (3, nb))
    x0, _ = sj.random_lanes(rng, model, nb)
    us = rng.uniform(-20.0, 20.0, (T, nb))
    return true, start, x0, us
