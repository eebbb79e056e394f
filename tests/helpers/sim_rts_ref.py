"""Numpy reference for the Rauch-Tung-Striebel smoother over a window (include/cpmpc.h: cpmpc_sim_rts_batch), formulated
differently from the kernel on purpose: np.linalg.solve on the UNSCALED P-, full matrices, on sim_ekf_ref.run's xs, Ps, Pms and
sim_ekf_ref.predict's A.  TEST INFRASTRUCTURE ONLY.

  scaled_pivots  the pivots of the Cholesky factorisation of the diagonally scaled matrix (unit diagonal): the kernel's test
                 for "positive definite", restated; a pivot at or below 8 nx eps, a diagonal entry not positive or a
                 non-finite pivot says no
  smooth         one problem: a filter run (sim_ekf_ref.run's dict) -> xs_smooth [T+1, nx], Ps_smooth [T+1, nx, nx], ok,
                 the gains, the smallest pivot, and the REACH of input errors (below).  dtype=np.float32 redoes ONLY the
                 smoother's algebra in float32, on the float64 x-, A and filter results handed in
  run_batch      filter and smoother for [nx, B] states; dtype applies to the filter's algebra and the smoother's alike
  filtered_variances  dt = 0, diagonal P0, q = 0: the filter's variances at every index, the largest term of the smoother's sum
  reference      run_batch on a case of sim_ekf_ref.CASES, made once per (case, lanes, dtype, arrays) and left unchanged

The reach.  x^s_t = x_t + G_t (x^s_{t+1} - x-_{t+1}): an error of size e max(1, |x|) in every filtered and predicted state
(what a float plant leaves: the siblings' state bound) reaches x^s_t, to first order, as e reach_x[t] with
    reach_x[T] = max(1, |x_T|),   reach_x[t] = max(1, |x_t|) + |G_t| (reach_x[t+1] + max(1, |x-_{t+1}|)),
products of |G| as nis_dx is a sum of |S^-1 nu| for nis.  For the covariances, P^s_t = P_t + G_t (P^s_{t+1} - P-_{t+1}) G_t^T:
entry (i, j) of a covariance has the scale s_i s_j, s = sqrt(diag P) (|P_ij| <= s_i s_j, and never above max|P|, the scale
the filter's test uses): a float A, e |A| off, moves (A P A^T)_ij by at most 2 e (|A| s)_i (|A| s)_j.  An error of e s_i s_j
in every filtered and predicted covariance reaches P^s_t, to first order and with G_t held, ENTRY BY ENTRY as e reach_P[t] with
    reach_P[T] = s_T s_T^T,   reach_P[t] = s_t s_t^T + |G_t| (reach_P[t+1] + s-_{t+1} s-_{t+1}^T) |G_t|^T.
A norm of G in its place (|G|_inf^2 max|P|) mixes the units -- a velocity's variance into a position's, then back through a
gain of 1 / dt -- and compounds 30 to 100 times a tick; entry by entry the reach stays within a few times the entry's own
scale (tests/test_sim_rts_ref.py holds it there), so the bound made from it still tells a right covariance from a wrong one."""
import numpy as np

from helpers import sim_ekf_ref as ek
from helpers import sim_jac_ref as sj
from helpers import sim_rollout_ref as sr


def scaled_pivots(P, dtype=np.float64):
    """P [n, n] symmetric -> (the pivots d_j of the Cholesky factorisation of D P D, D = diag(P)^-1/2, in `dtype`; positive
    definite by the kernel's rule?)"""
    P = np.asarray(P, dtype=dtype)
    n = P.shape[0]
    diag = np.diag(P)
    if not (diag > 0).all():
        return np.full(n, np.nan), False
    s = (dtype(1) / np.sqrt(diag)).astype(dtype)
    S = (P * s[:, None] * s[None, :]).astype(dtype)
    L = np.zeros((n, n), dtype=dtype)
    piv = np.zeros(n, dtype=dtype)
    ok = True
    for j in range(n):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        piv[j] = d
        if not (d > 8 * n * np.finfo(dtype).eps) or not np.isfinite(d):
            ok = False
            d = dtype(1)
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return piv, ok


def _scale(P):
    """s s^T, s = sqrt(diag P): the scale of each entry of a covariance (a diagonal entry that is not positive counts as 0)"""
    s = np.sqrt(np.maximum(np.diag(P), 0.0))
    return np.outer(s, s)


def smooth(orc, model, params, dt, x0, P0, us, flt, fext=None, dtype=np.float64):
    """One problem.  flt = sim_ekf_ref.run's dict for the same inputs.  -> dict xs_smooth [T+1, nx], Ps_smooth [T+1, nx, nx],
    ok (bool), G [T, nx, nx], min_pivot, reach_x [T+1, nx], reach_P [T+1, nx, nx]; float64 whatever `dtype` the algebra ran in."""
    nx, T = sj.NX[model], len(us)
    L = np.tril(np.asarray(P0, dtype=np.float64))
    xf = np.concatenate([np.asarray(x0, dtype=np.float64)[None], flt["xs"]])            # index 0 .. T
    Pf = np.concatenate([(L + L.T - np.diag(np.diag(L)))[None], flt["Ps"]])
    xs_s, Ps_s = np.zeros((T + 1, nx)), np.zeros((T + 1, nx, nx))
    G_all = np.zeros((T, nx, nx))
    reach_x, reach_P = np.zeros((T + 1, nx)), np.zeros((T + 1, nx, nx))
    x_s, P_s = xf[T].astype(dtype), Pf[T].astype(dtype)
    xs_s[T], Ps_s[T] = x_s, P_s
    reach_x[T], reach_P[T] = np.maximum(1.0, np.abs(xf[T])), _scale(Pf[T])
    ok, min_pivot = True, np.inf
    for t in range(T - 1, -1, -1):
        xm, A = ek.predict(orc, model, params, dt, xf[t], us[t], fext)
        Pm = flt["Pms"][t]
        piv, pd = scaled_pivots(Pm, dtype)
        if pd:
            min_pivot = min(min_pivot, float(piv.min()))
            AP = A.astype(dtype) @ Pf[t].astype(dtype)
            G = np.linalg.solve(Pm.astype(dtype), AP).T                                   # P- is symmetric
            d = ek._wrap_nearest(model, x_s - xm.astype(dtype))
            step = G @ d
            x_new = xf[t].astype(dtype) + step
            if (step != 0).any():
                x_new = sj._wrap(orc, model, np.array(x_new, dtype=np.float64)).astype(dtype)
            P_new = Pf[t].astype(dtype) + G @ (P_s - Pm.astype(dtype)) @ G.T
            P_new = (P_new + P_new.T) / dtype(2)
        else:
            ok = False
            G = np.zeros((nx, nx), dtype=dtype)
            x_new, P_new = xf[t].astype(dtype), Pf[t].astype(dtype)
        x_s, P_s = x_new, P_new
        xs_s[t], Ps_s[t], G_all[t] = x_s, P_s, G
        aG = np.abs(np.asarray(G, dtype=np.float64))
        reach_x[t] = np.maximum(1.0, np.abs(xf[t])) + aG @ (reach_x[t + 1] + np.maximum(1.0, np.abs(xm)))
        reach_P[t] = _scale(Pf[t]) + aG @ (reach_P[t + 1] + _scale(Pm)) @ aG.T
    return dict(xs_smooth=xs_s, Ps_smooth=Ps_s, ok=ok, G=G_all, min_pivot=min_pivot, reach_x=reach_x, reach_P=reach_P)


def run_batch(orc, model, params, dt, x0, P0, us, ys, w, q, om=None, fext=None, dtype=np.float64):
    """x0 [nx, B], P0 [nx, nx, B], us [T, B], ys [T, nx, B], om [T, B] or None, params np numbers or [np, B], fext None, 4
    shared numbers or [4, B] -> the filter's dict (sim_ekf_ref.run_batch) with xs_smooth [T+1, nx, B], Ps_smooth
    [T+1, nx, nx, B], x0_smooth, P0_smooth, ok [B] int, G [T, nx, nx, B], min_pivot [B], reach_x [T+1, nx, B], reach_P [T+1, nx, nx, B]"""
    nx, nb = x0.shape
    T = us.shape[0]
    out = ek.run_batch(orc, model, params, dt, x0, P0, us, ys, w, q, om, fext, dtype=dtype)
    out.update(xs_smooth=np.zeros((T + 1, nx, nb)), Ps_smooth=np.zeros((T + 1, nx, nx, nb)), ok=np.zeros(nb, dtype=np.int64),
               G=np.zeros((T, nx, nx, nb)), min_pivot=np.zeros(nb), reach_x=np.zeros((T + 1, nx, nb)),
               reach_P=np.zeros((T + 1, nx, nx, nb)))
    for b in range(nb):
        flt = dict(xs=out["xs"][:, :, b], Ps=out["Ps"][..., b], Pms=out["Pms"][..., b])
        r = smooth(orc, model, sr._params(params, b), dt, x0[:, b], P0[:, :, b], us[:, b], flt, sr._lane(fext, b), dtype)
        out["xs_smooth"][:, :, b], out["Ps_smooth"][..., b], out["ok"][b] = r["xs_smooth"], r["Ps_smooth"], int(r["ok"])
        out["G"][..., b], out["min_pivot"][b] = r["G"], r["min_pivot"]
        out["reach_x"][:, :, b], out["reach_P"][..., b] = r["reach_x"], r["reach_P"]
    out["x0_smooth"], out["P0_smooth"] = out["xs_smooth"][0], out["Ps_smooth"][0]
    return out


def filtered_variances(p0_diag, w, om, T):
    """dt = 0, diagonal P0, q = 0, one problem: om [T] or None -> [T+1, nx], the FILTERED variances (P0^-1 + sum_{s < t} om_s W)^-1
    of index t = 0 .. T (index 0 is P0's diagonal): the size of the terms of P_t + (P^s_{t+1} - P-_{t+1}) at that index"""
    om = np.ones(T) if om is None else np.asarray(om, dtype=np.float64)
    seen = np.concatenate([[0.0], np.cumsum(om)])
    return 1.0 / (1.0 / np.asarray(p0_diag, dtype=np.float64)[None] + seen[:, None] * np.asarray(w, dtype=np.float64)[None])


_REF = {}


def reference(orc, case, nb=ek.B, dtype=np.float64, arrays=None, key=None):
    """run_batch on the case's inputs, or on `arrays` (the same dict with the values a float tensor holds; `key` names them).
    Made once per (case, nb, dtype, key) and shared: nobody writes to it."""
    k = (case, nb, np.dtype(dtype).name, key if arrays is not None else None)
    if arrays is not None and key is None:
        k = None
    if k is None or k not in _REF:
        i = ek.inputs(orc, case, nb) if arrays is None else arrays
        r = run_batch(orc, case[0], i["prm"], case[1], i["x0"], i["P0"], i["us"], i["ys"], i["w"], i["q"], i["om"], i["f"],
                      dtype=dtype)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        if k is None:
            return r
        _REF[k] = r
    return _REF[k]
