"""Numpy reference for the plant step's derivative in the dynamics parameters (include/cpmpc.h:
cpmpc_sim_step_param_jac_batch), built on the CPU oracle's simulator alone.  TEST INFRASTRUCTURE ONLY.

  plant           the oracle's Simulator::Step of one problem (external forces: the 4-state model's)
  param_jacobian  P = dx+/dp of one problem [nx, np]: per parameter the Richardson-extrapolated central difference
                  (4 d(h/2) - d(h)) / 3 with h_j = rel max(|p_j|, 1e-3), state differences through sim_jac_ref.wrapped_diff
  param_jacobian_batch  the same for [nx, B] states; params np numbers or [np, B]
All comparisons against it are relative to the lane's max |P| over the whole matrix: single columns (v_mu_b: 1e-7 of the
largest) are not resolvable by differences."""
import numpy as np

from helpers import sim_jac_ref as sj

NP = {"single": 9, "double": 6}
COL_XS, COL_KS = 7, 8   # the bumper columns of the 4-state model


def plant(orc, model, params, dt, x, u, fext=None):
    if fext is None:
        return orc.sim_step_model(model, params, dt, u, x)
    assert model == "single"
    sim = orc.Simulator()
    sim.set_state(x)
    sim.step(list(params), dt, u, tuple(fext[:2]), tuple(fext[2:]))
    return sim.get_state()


def _central(orc, model, params, dt, x, u, j, h, fext):
    hi, lo = np.array(params, dtype=np.float64), np.array(params, dtype=np.float64)
    hi[j] += h
    lo[j] -= h
    return sj.wrapped_diff(orc, model, plant(orc, model, hi, dt, x, u, fext), plant(orc, model, lo, dt, x, u, fext)) / (2 * h)


def param_jacobian(orc, model, params, dt, x, u, rel=1e-4, fext=None, richardson=True):
    nx, npar = sj.NX[model], NP[model]
    P = np.zeros((nx, npar))
    for j in range(npar):
        h = rel * max(abs(float(params[j])), 1e-3)
        d = _central(orc, model, params, dt, x, u, j, h, fext)
        if richardson:
            d = (4.0 * _central(orc, model, params, dt, x, u, j, 0.5 * h, fext) - d) / 3.0
        P[:, j] = d
    return P


def param_jacobian_batch(orc, model, params, dt, x, u, rel=1e-4, fext=None):
    """x [nx, B], u [B], params np numbers or [np, B], fext None, 4 shared values or [4, B] -> P [nx, np, B]."""
    nx, nb = x.shape
    prm = np.asarray(params, dtype=np.float64)
    P = np.zeros((nx, NP[model], nb))
    for b in range(nb):
        f = None
        if fext is not None:
            f = np.asarray(fext, dtype=np.float64)
            f = f[:, b] if f.ndim == 2 else f
        P[:, :, b] = param_jacobian(orc, model, prm[:, b] if prm.ndim == 2 else prm, dt, x[:, b], u[b], rel, f)
    return P


def plant_batch(orc, model, params, dt, x, u, fext=None):
    prm = np.asarray(params, dtype=np.float64)
    out = np.zeros_like(x)
    for b in range(x.shape[1]):
        f = None
        if fext is not None:
            f = np.asarray(fext, dtype=np.float64)
            f = f[:, b] if f.ndim == 2 else f
        out[:, b] = plant(orc, model, prm[:, b] if prm.ndim == 2 else prm, dt, x[:, b], u[b], f)
    return out


def lane_err(got, ref):
    """per lane: max |got - ref| over the leading axes, relative to the lane's max |ref|"""
    ax = tuple(range(ref.ndim - 1))
    return np.abs(got - ref).max(axis=ax) / np.abs(ref).max(axis=ax)
