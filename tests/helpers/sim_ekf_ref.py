"""Numpy reference for the extended Kalman filter over a window (include/cpmpc.h: cpmpc_sim_ekf_batch), formulated differently
from the kernel on purpose, and CPU twins of StateFilter and of WindowEstimator with its rolling prior.  Built on the CPU oracle
through sim_jac_ref.step_ref.  TEST INFRASTRUCTURE ONLY.

  predict            x-, A of one tick from the filtered state (sim_jac_ref.step_ref)
  joint_update       the JOINT measurement update over the measured rows: K = P- H^T (H P- H^T + R)^-1, the Joseph form for P,
                     the innovation's pole angles wrapped -> x, P, nis.  `dtype` is the type the algebra runs in.
  sequential_update  the same filter restated as the kernel runs it: one measured state at a time, no inverse
  run                one problem over T ticks -> xs [T, nx], Ps [T, nx, nx], P-s [T, nx, nx] (before the update), nis.
                     dtype=np.float32 redoes ONLY the covariance and update algebra in float32, on the float64 x- and A: it
                     measures how sensitive the filter is to float32 rounding
  run_batch          the same for [nx, B] states
  constant_state     the closed form at dt = 0 with a diagonal P0 and q = 0: P = (P0^-1 + sum_t om_t W)^-1 and the weighted mean
  window_prior_estimates  the twin of WindowEstimator(prior_cov=...): sim_rollout_gn_x0_ref.window_estimates where there is no
                     prior, else its loop with the arrival cost advanced by one filter tick per dropped sample
  CASES / inputs     the cases of tests/test_gpu_sim_ekf.py and their draws, pinned as admissible by tests/test_sim_ekf_ref.py"""
import numpy as np

from helpers import sim_jac_ref as sj
from helpers import sim_rollout_gn_x0_ref as gx
from helpers import sim_rollout_ref as sr


def _wrap_nearest(model, d):
    """a difference of states, its pole angles to the nearest multiple of 2 pi; in d's own type"""
    d = np.array(d)
    nq = sj.NX[model] // 2
    two_pi = d.dtype.type(2 * np.pi)
    d[1:nq] = d[1:nq] - two_pi * np.round(d[1:nq] / two_pi)
    return d


def predict(orc, model, params, dt, x, u, fext=None):
    fb, fm = (None, None) if fext is None else (fext[:2], fext[2:])
    xm, A, _ = sj.step_ref(orc, model, params, dt, x, float(u), fb, fm)
    return xm, A


def joint_update(orc, model, xm, Pm, y, rho, dtype=np.float64):
    """xm [nx], Pm [nx, nx], y [nx], rho [nx] (inverse variances, 0 = not measured) -> x, P, nis"""
    idx = np.nonzero(np.asarray(rho) > 0)[0]
    if idx.size == 0:
        return np.array(xm, dtype=dtype), np.array(Pm, dtype=dtype), dtype(0)
    nx = len(xm)
    xm, Pm, y = np.asarray(xm, dtype=dtype), np.asarray(Pm, dtype=dtype), np.asarray(y, dtype=dtype)
    H = np.eye(nx, dtype=dtype)[idx]
    R = np.diag((1.0 / np.asarray(rho, dtype=np.float64)[idx]).astype(dtype))
    S = H @ Pm @ H.T + R
    nu = _wrap_nearest(model, y - xm)[idx]
    K = np.linalg.solve(S, H @ Pm).T            # S and P- are symmetric
    x = xm + K @ nu
    IKH = np.eye(nx, dtype=dtype) - K @ H
    P = IKH @ Pm @ IKH.T + K @ R @ K.T
    nis = nu @ np.linalg.solve(S, nu)
    x = sj._wrap(orc, model, np.array(x, dtype=np.float64)).astype(dtype)   # an update acted: the pole angles to (-pi, pi]
    return x, (P + P.T) / dtype(2), dtype(nis)


def sequential_update(orc, model, xm, Pm, y, rho, dtype=np.float64):
    """the kernel's statements in numpy: one measured state at a time in index order"""
    x, P = np.array(xm, dtype=dtype), np.array(Pm, dtype=dtype)
    nis, acted = dtype(0), False
    nx = len(x)
    for i in range(nx):
        if not rho[i] > 0:
            continue
        rv = dtype(1) / dtype(rho[i])
        s = P[i, i] + rv
        d = np.zeros(nx, dtype=dtype)
        d[i] = dtype(y[i]) - x[i]
        nu = _wrap_nearest(model, d)[i]
        gain = P[:, i] / s
        x = x + gain * nu
        nis = nis + nu * nu / s
        new = P - np.outer(gain, P[i, :])
        new[:, i] = gain * rv
        new[i, :] = gain * rv
        P, acted = new, True
    if acted:
        x = sj._wrap(orc, model, np.array(x, dtype=np.float64)).astype(dtype)
    return x, P, nis


def run(orc, model, params, dt, x0, P0, us, ys, w, q, om=None, fext=None, dtype=np.float64, update=joint_update):
    """One problem.  x0 [nx], P0 [nx, nx] (its lower triangle is read), us [T], ys [T, nx], w [nx] inverse variances, q [nx]
    process-noise variances, om [T] or None -> dict xs [T, nx], Ps [T, nx, nx], Pms [T, nx, nx], nis, and nis_dx = sum_t
    |d nis / d x-_t| . max(1, |x-_t|), the first-order reach of a relative error of the predicted states into nis.  Everything
    comes back as float64 whatever `dtype` the covariance and update algebra ran in."""
    nx, T = sj.NX[model], len(us)
    L = np.tril(np.asarray(P0, dtype=np.float64))
    P = (L + L.T - np.diag(np.diag(L))).astype(dtype)
    x = np.asarray(x0, dtype=np.float64)
    Q = np.diag(np.asarray(q, dtype=np.float64)).astype(dtype)
    w = np.asarray(w, dtype=np.float64)
    xs, Ps, Pms = np.zeros((T, nx)), np.zeros((T, nx, nx)), np.zeros((T, nx, nx))
    nis, nis_dx = dtype(0), 0.0
    for t in range(T):
        xm, A = predict(orc, model, params, dt, x, us[t], fext)
        A = A.astype(dtype)
        Pm = A @ P @ A.T + Q
        Pm = (Pm + Pm.T) / dtype(2)
        rho = w * (1.0 if om is None else float(om[t]))
        if (rho > 0).any():
            # d nis / d x- = -2 S^-1 nu on the measured rows: what an error of x- does to nis, in float64 whatever dtype is
            idx = np.nonzero(rho > 0)[0]
            S = np.asarray(Pm, dtype=np.float64)[np.ix_(idx, idx)] + np.diag(1.0 / rho[idx])
            nu = _wrap_nearest(model, np.asarray(ys[t], dtype=np.float64) - xm)[idx]
            nis_dx += float(2.0 * np.abs(np.linalg.solve(S, nu)) @ np.maximum(1.0, np.abs(xm[idx])))
            xf, P, n = update(orc, model, xm, Pm, ys[t], rho, dtype)
            x, nis = np.asarray(xf, dtype=np.float64), nis + n
        else:
            x, P = xm, Pm                       # nothing measured: the prediction, untouched
        xs[t], Ps[t], Pms[t] = x, P, Pm
    return dict(xs=xs, Ps=Ps, Pms=Pms, nis=float(nis), nis_dx=nis_dx)


def run_batch(orc, model, params, dt, x0, P0, us, ys, w, q, om=None, fext=None, dtype=np.float64, update=joint_update):
    """x0 [nx, B], P0 [nx, nx, B], us [T, B], ys [T, nx, B], om [T, B] or None, params np numbers or [np, B], fext None, 4 shared
    numbers or [4, B] -> dict xs [T, nx, B], Ps / Pms [T, nx, nx, B], nis [B], nis_dx [B], x_final, P_final"""
    nx, nb = x0.shape
    T = us.shape[0]
    out = dict(xs=np.zeros((T, nx, nb)), Ps=np.zeros((T, nx, nx, nb)), Pms=np.zeros((T, nx, nx, nb)), nis=np.zeros(nb),
               nis_dx=np.zeros(nb))
    for b in range(nb):
        r = run(orc, model, sr._params(params, b), dt, x0[:, b], P0[:, :, b], us[:, b], ys[:, :, b], w, q,
                None if om is None else om[:, b], sr._lane(fext, b), dtype, update)
        out["xs"][:, :, b], out["Ps"][..., b], out["Pms"][..., b], out["nis"][b] = r["xs"], r["Ps"], r["Pms"], r["nis"]
        out["nis_dx"][b] = r["nis_dx"]
    out["x_final"], out["P_final"] = out["xs"][-1], out["Ps"][-1]
    return out


def constant_state(x0, p0_diag, ys, w, om=None):
    """dt = 0, diagonal P0, q = 0, one problem: ys [T, nx], om [T] or None -> the mean [nx] and the variances [nx] of
    P = (P0^-1 + sum_t om_t W)^-1, mean = P (P0^-1 x0 + sum_t om_t W y_t).  (No wrap: the draws keep every difference small.)"""
    T = len(ys)
    om = np.ones(T) if om is None else np.asarray(om, dtype=np.float64)
    info = 1.0 / np.asarray(p0_diag, dtype=np.float64) + om.sum() * np.asarray(w, dtype=np.float64)
    rhs = np.asarray(x0) / np.asarray(p0_diag) + np.einsum("t,q,tq->q", om, np.asarray(w, dtype=np.float64), np.asarray(ys))
    return rhs / info, 1.0 / info


def window_prior_estimates(orc, model, params, dt, guess, us, ys, window, w=None, iterations=2, prior_cov=None, q=None):
    """The twin of WindowEstimator for one problem: push(us[t], ys[t]) then estimate(iterations) for every tick t.  Without
    prior_cov it IS sim_rollout_gn_x0_ref.window_estimates.  With prior_cov [nx, nx] the prior mean starts as `guess`, and
    whenever a full window drops its oldest tick, mean and covariance move over the dropped (u, y) by one filter tick; every
    estimate carries the arrival cost (mean, covariance^-1).  -> the current-state estimates [len(us), nx]"""
    if prior_cov is None:
        return gx.window_estimates(orc, model, params, dt, guess, us, ys, window, w, iterations)
    nx = sj.NX[model]
    wv = np.ones(nx) if w is None else np.asarray(w, dtype=np.float64)
    qv = np.zeros(nx) if q is None else np.asarray(q, dtype=np.float64)
    x0 = np.array(guess, dtype=np.float64)
    mean, cov = x0.copy(), np.array(prior_cov, dtype=np.float64)
    out = np.zeros((len(us), nx))
    for t in range(len(us)):
        lo = max(0, t + 1 - window)
        if t + 1 > window:
            r = run(orc, model, params, dt, mean, cov, us[lo - 1:lo], ys[lo - 1:lo], wv, qv)
            mean, cov = r["xs"][-1], r["Ps"][-1]
            x0 = sr.rollout(orc, model, params, dt, x0, us[lo - 1:lo])[-1]
        its, out[t] = gx.estimate(orc, model, params, dt, x0, us[lo:t + 1], ys[lo:t + 1], w, iterations=iterations,
                                  prior=mean, prior_info=np.linalg.inv(cov))
        x0 = its[-1]
    return out


# ---- the cases of tests/test_gpu_sim_ekf.py ---------------------------------------------------------------------------------
B = 130
DT_T = ((0.0105, 5), (0.02, 3), (0.001, 8), (0.0, 3))
# (model, dt, T, kind): kind None; "dyn" per-problem parameters; "tw" per-sample weights in [0, 2] with exact zeros; "shared" /
# "per" external forces (4-state model: the reference has forces for it alone); "w0" nothing measured
CASES = [(m, dt, nt, None) for m in ("single", "double") for dt, nt in DT_T] + \
        [("single", 0.0105, 5, "dyn"), ("double", 0.0105, 5, "dyn"), ("single", 0.0105, 5, "tw"), ("double", 0.0105, 5, "tw"),
         ("single", 0.0105, 5, "shared"), ("single", 0.0105, 5, "per"), ("single", 0.0105, 1, None), ("double", 0.0105, 2, None),
         ("single", 0.0105, 5, "w0"), ("double", 0.0105, 5, "w0")]
IDS = ["%s-%g-%d-%s" % c for c in CASES]
SHARED_F = ((1.5, 0.0), (-2.0, 1.0))
SIGMA = 0.01                      # the encoders' noise: weights 1 / SIGMA^2 on the positions, 0 on the velocities
Q_VELOCITY = 1e-6                 # process noise: variances added per tick to the velocities


def weights(model, kind=None):
    nq = sj.NX[model] // 2
    return np.array([0.0 if kind == "w0" else 1.0 / SIGMA ** 2] * nq + [0.0] * nq)


def process_noise(model):
    nq = sj.NX[model] // 2
    return np.array([0.0] * nq + [Q_VELOCITY] * nq)


def covariances(model, nb, seed=47):
    """P0 [nx, nx, nb] = D + 0.1 (a random correlation matrix scaled into D), D = diag(1e-2 on positions, 4e-2 on velocities)"""
    nx = sj.NX[model]
    nq = nx // 2
    rng = np.random.default_rng(seed + nx)
    d = np.sqrt(np.array([1e-2] * nq + [4e-2] * nq))
    P = np.zeros((nx, nx, nb))
    for b in range(nb):
        G = rng.normal(size=(nx, nx))
        S = G @ G.T
        c = 1.0 / np.sqrt(np.diag(S))
        P[:, :, b] = np.diag(d * d) + 0.1 * (S * c[:, None] * c[None, :]) * d[:, None] * d[None, :]
    return P


_IN = {}


def inputs(orc, case, nb=B):
    """numpy inputs of a case, made once and left unchanged: dict x0 [nx, nb], P0 [nx, nx, nb], us [T, nb], ys [T, nx, nb] (the
    oracle's rollout from x0 plus noise of +- 2 SIGMA), f (None, 4 shared numbers or [4, nb]), prm (np numbers or [np, nb]),
    w [nx], q [nx], om (None or [T, nb])"""
    key = (case, nb)
    if key not in _IN:
        model, dt, nt, kind = case
        nx = sj.NX[model]
        x, _ = sj.states(model, nb)
        rng = np.random.default_rng(53)
        us = rng.uniform(-20.0, 20.0, (nt, nb))
        noise = rng.uniform(-2 * SIGMA, 2 * SIGMA, (nt, nx, nb))
        f = None
        if kind == "shared":
            f = np.array([SHARED_F[0][0], SHARED_F[0][1], SHARED_F[1][0], SHARED_F[1][1]])
        elif kind == "per":
            f = np.random.default_rng(21).uniform(-3.0, 3.0, (4, nb))
        prm = np.array(sj.DYN[model])
        if kind == "dyn":
            prm = np.tile(prm[:, None], (1, nb)) * np.random.default_rng(43).uniform(0.8, 1.2, (len(prm), nb))
        om = None
        if kind == "tw":
            om = np.random.default_rng(45).uniform(0.0, 2.0, (nt, nb))
            om[np.random.default_rng(46).uniform(size=(nt, nb)) < 0.25] = 0.0
        ys = sr.rollout_batch(orc, model, prm, dt, x, us, f) + noise
        _IN[key] = dict(x0=x, P0=covariances(model, nb), us=us, ys=ys, f=f, prm=prm, w=weights(model, kind),
                        q=process_noise(model), om=om)
        for a in _IN[key].values():
            if a is not None:
                a.setflags(write=False)
    return _IN[key]


def reference(orc, case, nb=B, dtype=np.float64, arrays=None):
    """run_batch on the case's inputs, or on `arrays` (the same dict with the values a float tensor holds) -> its dict"""
    i = inputs(orc, case, nb) if arrays is None else arrays
    return run_batch(orc, case[0], i["prm"], case[1], i["x0"], i["P0"], i["us"], i["ys"], i["w"], i["q"], i["om"], i["f"],
                     dtype=dtype)


# StateFilter and WindowEstimator(prior_cov=...) against their twins: fp64, positions only
FILTER_B, FILTER_TICKS = 64, 12
WINDOW_B, WINDOW_TICKS, WINDOW_T, WINDOW_ITERATIONS = 64, 12, 4, 2


def twin_draws(model="single", nb=FILTER_B, ticks=FILTER_TICKS, seed=31):
    """-> truth x0 [nx, nb], the first guess [nx, nb] (the truth perturbed as the estimation tests perturb it), us [ticks, nb]"""
    return gx.estimation_draws(model, nb, ticks, seed)


def prior_covariance(model):
    """the diagonal prior covariance of the twins' first guess: the squares of the perturbation"""
    return gx.perturbation(model) ** 2
