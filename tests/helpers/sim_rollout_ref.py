"""Numpy reference for the plant rollout over T ticks and its adjoint (include/cpmpc.h: cpmpc_sim_rollout_batch,
cpmpc_sim_rollout_vjp_batch), built on the CPU oracle and the two one-step references.  TEST INFRASTRUCTURE ONLY.

  rollout        xs [T, nx] of one problem: the oracle's plant step chained, x_{t+1} = Step(x_t, u_t, dt)
  adjoint        (xs, g_x0 [nx], g_u [T], g_p [np]) of one problem for cotangents gbar [T, nx] on every x_{t+1} and / or
                 gbar_final [nx] on x_T: from the last tick down, lambda += gbar[t]; g_u[t] = Bu_t . lambda,
                 g_p += P_t^T lambda, lambda <- A_t^T lambda, with A_t, Bu_t from sim_jac_ref.step_ref and P_t from
                 sim_param_ref.param_jacobian at x_t.  dt = 0: lambda is the cotangents added up, nothing else
  recurrence     the same recurrence on given per-tick matrices A [T, nx, nx, B], Bu [T, nx, B], P [T, nx, np, B], batched
                 (the GPU tests feed it the one-step calls' matrices, and their absolute values for the error bound)
  loss           sum_t gbar[t] . wrapped_diff(x_{t+1}, xs_nom[t]): the scalar whose gradient the adjoint is
  fd_gradients   Richardson-extrapolated central differences (4 d(h/2) - d(h)) / 3 of that loss on the oracle's rollout:
                 h = 1e-5 in the state, 1e-3 in the controls, 1e-4 max(|p_j|, 1e-3) in the parameters
  *_batch        the same for [nx, B] states, u [T, B], gbar [T, nx, B]; params np numbers or [np, B]"""
import numpy as np

from helpers import sim_jac_ref as sj
from helpers import sim_param_ref as sp

H_STATE, H_CONTROL, REL_PARAM = 1e-5, 1e-3, 1e-4


def rollout(orc, model, params, dt, x0, us, fext=None):
    x = np.array(x0, dtype=np.float64)
    xs = np.zeros((len(us), sj.NX[model]))
    for t, u in enumerate(us):
        x = np.array(sp.plant(orc, model, params, dt, x, float(u), fext), dtype=np.float64)
        xs[t] = x
    return xs


def adjoint(orc, model, params, dt, x0, us, gbar=None, gbar_final=None, fext=None):
    nx, npar, T = sj.NX[model], sp.NP[model], len(us)
    xs = rollout(orc, model, params, dt, x0, us, fext)
    lam, g_u, g_p = np.zeros(nx), np.zeros(T), np.zeros(npar)
    fb, fm = (None, None) if fext is None else (fext[:2], fext[2:])
    for t in range(T - 1, -1, -1):
        if gbar is not None:
            lam = lam + gbar[t]
        if gbar_final is not None and t == T - 1:
            lam = lam + gbar_final
        if not sj.sub_steps(dt):
            continue
        xt = np.asarray(x0, dtype=np.float64) if t == 0 else xs[t - 1]
        _, A, Bu = sj.step_ref(orc, model, params, dt, xt, float(us[t]), fb, fm)
        P = sp.param_jacobian(orc, model, params, dt, xt, float(us[t]), fext=fext)
        g_u[t] = Bu @ lam
        g_p += P.T @ lam
        lam = A.T @ lam
    return xs, lam, g_u, g_p


def recurrence(A, Bu, P, gbar=None, gbar_final=None):
    """A [T, nx, nx, B], Bu [T, nx, B], P [T, nx, np, B] or None -> g_x0 [nx, B], g_u [T, B], g_p [np, B] (zeros without P)."""
    T, nx, _, nb = A.shape
    lam, g_u = np.zeros((nx, nb)), np.zeros((T, nb))
    g_p = np.zeros((P.shape[2] if P is not None else 0, nb))
    for t in range(T - 1, -1, -1):
        if gbar is not None:
            lam = lam + gbar[t]
        if gbar_final is not None and t == T - 1:
            lam = lam + gbar_final
        g_u[t] = np.einsum("rb,rb->b", Bu[t], lam)
        if P is not None:
            g_p += np.einsum("rjb,rb->jb", P[t], lam)
        lam = np.einsum("rcb,rb->cb", A[t], lam)
    return lam, g_u, g_p


def loss(orc, model, params, dt, x0, us, gbar, xs_nom, fext=None):
    xs = rollout(orc, model, params, dt, x0, us, fext)
    return sum(float(gbar[t] @ sj.wrapped_diff(orc, model, xs[t], xs_nom[t])) for t in range(len(us)))


def fd_gradients(orc, model, params, dt, x0, us, gbar, fext=None):
    nx, npar, T = sj.NX[model], sp.NP[model], len(us)
    x0, us = np.asarray(x0, dtype=np.float64), np.asarray(us, dtype=np.float64)
    prm = np.asarray(params, dtype=np.float64)
    nom = rollout(orc, model, prm, dt, x0, us, fext)

    def L(x, u, p):
        return loss(orc, model, p, dt, x, u, gbar, nom, fext)

    def richardson(f, h):
        d1 = (f(h) - f(-h)) / (2 * h)
        d2 = (f(0.5 * h) - f(-0.5 * h)) / h
        return (4.0 * d2 - d1) / 3.0

    def bump(v, i, h):
        w = v.copy()
        w[i] += h
        return w

    g_x0 = np.array([richardson(lambda h, i=i: L(bump(x0, i, h), us, prm), H_STATE) for i in range(nx)])
    g_u = np.array([richardson(lambda h, t=t: L(x0, bump(us, t, h), prm), H_CONTROL) for t in range(T)])
    g_p = np.array([richardson(lambda h, j=j: L(x0, us, bump(prm, j, h)), REL_PARAM * max(abs(float(prm[j])), 1e-3))
                    for j in range(npar)])
    return g_x0, g_u, g_p


def _lane(a, b):
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    return a[..., b] if a.ndim >= 2 else a


def _params(params, b):
    prm = np.asarray(params, dtype=np.float64)
    return prm[:, b] if prm.ndim == 2 else prm


def rollout_batch(orc, model, params, dt, x0, us, fext=None):
    """x0 [nx, B], us [T, B] -> xs [T, nx, B]"""
    nx, nb = x0.shape
    xs = np.zeros((us.shape[0], nx, nb))
    for b in range(nb):
        xs[:, :, b] = rollout(orc, model, _params(params, b), dt, x0[:, b], us[:, b], _lane(fext, b))
    return xs


def adjoint_batch(orc, model, params, dt, x0, us, gbar=None, gbar_final=None, fext=None):
    """-> xs [T, nx, B], g_x0 [nx, B], g_u [T, B], g_p [np, B]"""
    nx, nb = x0.shape
    T = us.shape[0]
    xs, g_x0, g_u, g_p = np.zeros((T, nx, nb)), np.zeros((nx, nb)), np.zeros((T, nb)), np.zeros((sp.NP[model], nb))
    for b in range(nb):
        xs[:, :, b], g_x0[:, b], g_u[:, b], g_p[:, b] = adjoint(
            orc, model, _params(params, b), dt, x0[:, b], us[:, b], None if gbar is None else gbar[:, :, b],
            None if gbar_final is None else gbar_final[:, b], _lane(fext, b))
    return xs, g_x0, g_u, g_p


def fd_gradients_batch(orc, model, params, dt, x0, us, gbar, fext=None):
    nx, nb = x0.shape
    g_x0, g_u, g_p = np.zeros((nx, nb)), np.zeros((us.shape[0], nb)), np.zeros((sp.NP[model], nb))
    for b in range(nb):
        g_x0[:, b], g_u[:, b], g_p[:, b] = fd_gradients(orc, model, _params(params, b), dt, x0[:, b], us[:, b],
                                                        gbar[:, :, b], _lane(fext, b))
    return g_x0, g_u, g_p
