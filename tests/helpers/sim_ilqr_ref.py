"""Numpy reference for one iteration of iterative LQR on the plant's tick map and for the loop above it (include/cpmpc.h:
cpmpc_sim_ilqr_backward_batch, cpmpc_sim_ilqr_forward_batch; batch.py: sim_ilqr), formulated differently from the kernels on
purpose.  Built on sim_lqr_ref.trajectory, closed_loop and wrap_nearest.  TEST INFRASTRUCTURE ONLY.

  cost            J = sum_t (e_t^T diag(q) e_t + r (u_t - uref_t)^2) + e_T^T P_T e_T of one problem, e_t = wrap(x_t - xref_t)
  backward        the value recursion in the TEXTBOOK form Q_x, Q_u, Q_xx, Q_ux, Q_uu (halved gradients: J has no factor 1/2),
                      k = clamp(u - Q_u / (Q_uu + mu)) - u,  K = clamped ? 0 : -Q_ux / (Q_uu + mu),
                      V_x = Q_x + K Q_uu k + K Q_u + Q_ux k,  V_xx = Q_xx + K Q_uu K^T + K Q_ux^T + Q_ux K^T
                  -> dict K [T, nx], kff [T], dV [2], P0, g0, hmax, un [T] (the unclamped controls).  `dtype`: the type the
                  algebra runs in; np.float32 redoes ONLY the recursion in float32, on the float64 Phi, gamma and residuals
  dense_step      the linearised problem stacked as ONE least-squares system in the T control changes -> the minimiser du [T]
                  and the model's cost change
  policy_rollout  the linearised system from dx_0 = 0 under du = kff + K dx -> du [T]
  forward         the forward pass through the oracle's step: u = clamp(u_nom + alpha kff + K . wrap(x - x_nom)) -> xs, us, J
  loop            sim_ilqr's loop for one problem
  *_batch         the same over [.., B] arrays
  CASES / inputs  the cases of tests/test_gpu_sim_ilqr.py and their draws; LOOP_* the loop test's, pinned as admissible by
                  tests/test_sim_ilqr_ref.py"""
import json
import os

import numpy as np

from helpers import sim_jac_ref as sj
from helpers import sim_lqr_ref as lq
from helpers import sim_rollout_ref as sr

ARMIJO = 1e-4


def residuals(model, x0, xs, xref):
    """e [T + 1, nx]: wrap(x_t - xref_t), x_0 = x0, x_t = xs[t - 1]"""
    x = np.concatenate([np.asarray(x0, dtype=np.float64)[None], xs])
    return np.stack([lq.wrap_nearest(model, x[t] - xref[t]) for t in range(len(x))])


def cost(model, x0, xs, us, xref, uref, q, r, PT):
    e = residuals(model, x0, xs, xref)
    du = np.asarray(us, dtype=np.float64) - uref
    return float((e[:-1] ** 2 * np.asarray(q)).sum() + r * (du ** 2).sum() + e[-1] @ PT @ e[-1])


def backward(Phi, gam, e, us, uref, q, r, PT, mu=0.0, u_limit=np.inf, dtype=np.float64):
    T, nx = gam.shape
    f = dtype
    Q = np.diag(np.asarray(q, dtype=np.float64)).astype(f)
    Vxx = np.asarray(PT, dtype=np.float64).astype(f)
    Vx = Vxx @ e[T].astype(f)
    K, kff, un = np.zeros((T, nx), dtype=f), np.zeros(T, dtype=f), np.zeros(T, dtype=f)
    dV1 = dV2 = hmax = f(0)
    for t in range(T - 1, -1, -1):
        A, b = Phi[t].astype(f), gam[t].astype(f)
        u, du = f(us[t]), f(us[t]) - f(uref[t])
        Qx = Q @ e[t].astype(f) + A.T @ Vx
        Qu = f(r) * du + b @ Vx
        Qxx = Q + A.T @ Vxx @ A
        Qux = A.T @ (Vxx @ b)
        Quu = f(r) + b @ Vxx @ b
        Qr = Quu + f(mu)
        un[t] = u - Qu / Qr
        uc = min(max(un[t], f(-u_limit)), f(u_limit))
        k = uc - u
        Kt = np.zeros(nx, dtype=f) if uc != un[t] else -Qux / Qr
        dV1, dV2, hmax = dV1 + 2 * k * Qu, dV2 + k * k * Quu, max(hmax, abs(k) * Qr)
        Vx = Qx + Kt * (Quu * k) + Kt * Qu + Qux * k
        Vxx = Qxx + Quu * np.outer(Kt, Kt) + np.outer(Kt, Qux) + np.outer(Qux, Kt)
        Vxx = (Vxx + Vxx.T) / f(2)
        K[t], kff[t] = Kt, k
    d = np.float64
    return dict(K=K.astype(d), kff=kff.astype(d), dV=np.array([dV1, dV2], dtype=d), P0=Vxx.astype(d), g0=Vx.astype(d),
                hmax=float(hmax), un=un.astype(d))


def dense_step(Phi, gam, e, us, uref, q, r, PT):
    """min over du of sum_t |Q^1/2 (e_t + dx_t)|^2 + r (u_t - uref_t + du_t)^2 + |P_T^1/2 (e_T + dx_T)|^2 with dx_0 = 0,
    dx_{t+1} = Phi_t dx_t + gamma_t du_t, as one least-squares system -> du [T], the cost change of the model"""
    T, nx = gam.shape
    sq, sr_, sT = np.diag(np.sqrt(np.asarray(q, dtype=np.float64))), np.sqrt(r), lq._sqrt_psd(PT)
    G = [np.zeros((nx, T))]          # dx_t = G[t] du
    for t in range(T):
        g = Phi[t] @ G[-1]
        g[:, t] += gam[t]
        G.append(g)
    rows, rhs = [], []
    for t in range(T):
        rows.append(sq @ G[t])
        rhs.append(sq @ e[t])
        row = np.zeros((1, T))
        row[0, t] = sr_
        rows.append(row)
        rhs.append(np.array([sr_ * (us[t] - uref[t])]))
    rows.append(sT @ G[T])
    rhs.append(sT @ e[T])
    Mu, c = np.vstack(rows), np.concatenate(rhs)
    du = -np.linalg.lstsq(Mu, c, rcond=None)[0]
    res = c + Mu @ du
    return du, float(res @ res - c @ c)


def policy_rollout(Phi, gam, K, kff):
    T, nx = gam.shape
    dx, du = np.zeros(nx), np.zeros(T)
    for t in range(T):
        du[t] = kff[t] + K[t] @ dx
        dx = Phi[t] @ dx + gam[t] * du[t]
    return du


def forward(orc, model, params, dt, x0, u_nom, kff, K, x0_nom, xs_nom, alpha, u_limit, xref, uref, q, r, PT, fext=None):
    """through closed_loop: alpha kff is folded into the nominal controls it is given"""
    base = np.asarray(u_nom, dtype=np.float64) + (0.0 if kff is None else alpha * np.asarray(kff, dtype=np.float64))
    xs, us = lq.closed_loop(orc, model, params, dt, x0, base, K, x0_nom, xs_nom, u_limit, fext)
    return xs, us, cost(model, x0, xs, us, xref, uref, q, r, PT)


def linearise(orc, model, params, dt, x0, us, fext=None):
    return lq.trajectory(orc, model, params, dt, x0, us, fext)


def loop(orc, model, params, dt, x0, u_init, xref, uref, q, r, PT, u_limit=np.inf, iterations=10, trials=6, mu_init=0.0, fext=None):
    """sim_ilqr's loop for one problem -> dict u, xs, cost, cost_history [iterations + 1], mu, accepted [iterations], hmax (of
    the returned trajectory, with the returned mu), K"""
    args = (xref, uref, q, r, PT)
    xs, us, J = forward(orc, model, params, dt, x0, u_init, None, None, None, None, 1.0, u_limit, *args, fext=fext)
    mu, hist, acc = float(mu_init), [J], []
    for _ in range(iterations):
        _, Phi, gam = linearise(orc, model, params, dt, x0, us, fext)
        bw = backward(Phi, gam, residuals(model, x0, xs, xref), us, uref, q, r, PT, mu, u_limit)
        alpha, done = 1.0, False
        for _ in range(trials):
            if not done:
                _, _, J_try = forward(orc, model, params, dt, x0, us, bw["kff"], bw["K"], x0, xs, alpha, u_limit, *args, fext=fext)
                pred = bw["dV"][0] * alpha + bw["dV"][1] * alpha * alpha
                done = bool(pred < 0 and J_try - J <= ARMIJO * pred)
                if not done:
                    alpha *= 0.5
        if done:
            xs, us, J = forward(orc, model, params, dt, x0, us, bw["kff"], bw["K"], x0, xs, alpha, u_limit, *args, fext=fext)
            mu = mu / 10.0
            mu = 0.0 if mu < 1e-6 else mu
        else:
            mu = max(10.0 * mu, 1e-3)
        hist.append(J)
        acc.append(done)
    _, Phi, gam = linearise(orc, model, params, dt, x0, us, fext)
    last = backward(Phi, gam, residuals(model, x0, xs, xref), us, uref, q, r, PT, mu, u_limit)
    return dict(u=us, xs=xs, cost=J, cost_history=np.array(hist), mu=mu, accepted=np.array(acc, dtype=bool), hmax=last["hmax"],
                K=last["K"])


# ---- batches -----------------------------------------------------------------------------------------------------------------
def _terminal(q, terminal, b):
    term = terminal[:, :, b] if isinstance(terminal, np.ndarray) and terminal.ndim == 3 else terminal
    return lq.terminal_matrix(q, term)


def expand_ref(x_ref, T, nx, nb):
    """x_ref [T + 1, nx, nb], [nx, nb] or [nx] -> [T + 1, nx, nb]"""
    x_ref = np.asarray(x_ref, dtype=np.float64)
    if x_ref.ndim == 1:
        x_ref = x_ref[:, None] * np.ones((1, nb))
    if x_ref.ndim == 2:
        x_ref = np.tile(x_ref[None], (T + 1, 1, 1))
    assert x_ref.shape == (T + 1, nx, nb)
    return x_ref


def backward_batch(orc, model, params, dt, x0, us, x_ref, u_ref, q, r, terminal=None, mu=None, u_limit=np.inf, fext=None,
                   dtype=np.float64):
    """x0 [nx, B], us [T, B], x_ref (expand_ref's forms), u_ref [T, B] or None, mu [B] or None -> dict xs [T, nx, B] (the
    oracle's trajectory), K [T, nx, B], kff [T, B], dV [2, B], P0 [nx, nx, B], g0 [nx, B], hmax [B], un [T, B]"""
    nx, nb = x0.shape
    T = us.shape[0]
    xr = expand_ref(x_ref, T, nx, nb)
    out = dict(xs=np.zeros((T, nx, nb)), K=np.zeros((T, nx, nb)), kff=np.zeros((T, nb)), dV=np.zeros((2, nb)),
               P0=np.zeros((nx, nx, nb)), g0=np.zeros((nx, nb)), hmax=np.zeros(nb), un=np.zeros((T, nb)))
    for b in range(nb):
        xs, Phi, gam = lq.trajectory(orc, model, sr._params(params, b), dt, x0[:, b], us[:, b], sr._lane(fext, b))
        e = residuals(model, x0[:, b], xs, xr[:, :, b])
        bw = backward(Phi, gam, e, us[:, b], np.zeros(T) if u_ref is None else u_ref[:, b], q, r, _terminal(q, terminal, b),
                      0.0 if mu is None else float(mu[b]), u_limit, dtype)
        out["xs"][:, :, b] = xs
        for n in ("K", "kff", "dV", "P0", "g0", "hmax", "un"):
            out[n][..., b] = bw[n]
    return out


def forward_batch(orc, model, params, dt, x0, u_nom, kff, K, x0_nom, xs_nom, alpha, x_ref, u_ref, q, r, terminal=None,
                  u_limit=np.inf, fext=None):
    """-> xs [T, nx, B], us [T, B], cost [B]"""
    nx, nb = x0.shape
    T = u_nom.shape[0]
    xr = expand_ref(x_ref, T, nx, nb)
    xs, us, J = np.zeros((T, nx, nb)), np.zeros((T, nb)), np.zeros(nb)
    for b in range(nb):
        xs[:, :, b], us[:, b], J[b] = forward(
            orc, model, sr._params(params, b), dt, x0[:, b], u_nom[:, b], None if kff is None else kff[:, b],
            None if K is None else K[:, :, b], None if K is None else x0_nom[:, b], None if K is None else xs_nom[:, :, b],
            1.0 if alpha is None else float(alpha[b]), u_limit, xr[:, :, b], np.zeros(T) if u_ref is None else u_ref[:, b], q, r,
            _terminal(q, terminal, b), sr._lane(fext, b))
    return xs, us, J


def cost_batch(model, x0, xs, us, x_ref, u_ref, q, r, terminal=None):
    nx, nb = x0.shape
    T = us.shape[0]
    xr = expand_ref(x_ref, T, nx, nb)
    return np.array([cost(model, x0[:, b], xs[:, :, b], us[:, b], xr[:, :, b], np.zeros(T) if u_ref is None else u_ref[:, b], q, r,
                          _terminal(q, terminal, b)) for b in range(nb)])


def loop_batch(orc, model, params, dt, x0, u_init, x_ref, q, r, terminal=None, u_ref=None, u_limit=np.inf, iterations=10, trials=6,
               mu_init=0.0):
    nx, nb = x0.shape
    T = u_init.shape[0]
    xr = expand_ref(x_ref, T, nx, nb)
    runs = [loop(orc, model, sr._params(params, b), dt, x0[:, b], u_init[:, b], xr[:, :, b],
                 np.zeros(T) if u_ref is None else u_ref[:, b], q, r, _terminal(q, terminal, b), u_limit, iterations, trials, mu_init)
            for b in range(nb)]
    return {n: np.stack([np.asarray(run[n]) for run in runs], axis=-1) for n in runs[0]}


# ---- the cases of tests/test_gpu_sim_ilqr.py ----------------------------------------------------------------------------------
B = lq.B
Q, R = lq.Q, lq.R
DT_T = ((0.0105, 5), (0.001, 8), (0.0, 3), (0.0105, 1), (0.01, 12))
# (model, dt, T, kind): kind None; "dyn" per-problem parameters; "per" per-problem forces (4-state model); "PT" a tensor terminal
# cost; "mu" a regularisation per lane; "limit" a limit that binds: LIMIT, with the trajectory's controls drawn inside it (the
# unclamped minimiser has a median near 1.3 N here); every other kind draws them from +-U_MAX.
CASES = [(m, dt, nt, None) for m in ("single", "double") for dt, nt in DT_T] + \
        [(m, 0.0105, 5, k) for m in ("single", "double") for k in ("dyn", "PT", "mu", "limit")] + [("single", 0.0105, 5, "per")]
IDS = ["%s-%g-%d-%s" % c for c in CASES]
U_MAX, LIMIT = 20.0, 2.0


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


_IN = {}


def inputs(orc, case, nb=B):
    """numpy inputs of a case, made once and left unchanged: dict x0 [nx, nb] (sim_lqr_ref's states: lanes at the +-pi cut and
    beyond the bumpers), us [T, nb], x_ref [T + 1, nx, nb] (the upright, the cart at a per-lane place, moved a little per tick),
    u_ref [T, nb], f, prm, q, r, PT, mu (None or [nb]), u_limit"""
    key = (case, nb)
    if key not in _IN:
        model, dt, nt, kind = case
        nx, nq = sj.NX[model], sj.NX[model] // 2
        x, _ = sj.states(model, nb)
        rng = np.random.default_rng(97 + nx)
        us = rng.uniform(-U_MAX, U_MAX, (nt, nb)) * (LIMIT / U_MAX if kind == "limit" else 1.0)
        f, prm = lq._plant_draws(model, kind, nb)
        x_ref = np.zeros((nt + 1, nx, nb))
        x_ref[:, 0] = rng.uniform(-0.3, 0.3, (1, nb))
        x_ref[:, 1:nq] = np.pi / 2
        x_ref += rng.uniform(-0.05, 0.05, (nt + 1, nx, nb))
        u_ref = rng.uniform(-1.0, 1.0, (nt, nb))
        mu = rng.choice([0.0, 1e-3, 0.1, 10.0], nb) if kind == "mu" else None
        _IN[key] = _freeze(dict(x0=x, us=us, x_ref=x_ref, u_ref=u_ref, f=f, prm=prm, q=np.array(Q[model]), r=R,
                                PT=lq.terminal_costs(model, nb) if kind == "PT" else None, mu=mu,
                                u_limit=LIMIT if kind == "limit" else np.inf))
    return _IN[key]


def reference(orc, case, nb=B, dtype=np.float64, arrays=None):
    """backward_batch on the case's inputs, or on `arrays` (the same dict with the values a float tensor holds)"""
    i = inputs(orc, case, nb) if arrays is None else arrays
    return backward_batch(orc, case[0], i["prm"], case[1], i["x0"], i["us"], i["x_ref"], i["u_ref"], i["q"], i["r"], i["PT"],
                          i["mu"], i["u_limit"], i["f"], dtype)


# ---- the loop test: T = 30, dt = 0.01, sim_lqr_ref's Q and R, terminal 10 q, starts around the upright ------------------------
LOOP_DT, LOOP_T, LOOP_NB, LOOP_ITERS, LOOP_TRIALS = 0.01, 30, 32, 12, 6
# the 4-state model with the prototype's +-0.3 and 4 N; the 6-state one with smaller starts and a looser limit, as it converges
# more slowly and does not finish under 4 N
LOOP_SPREAD = {"single": 0.3, "double": 0.1}
LOOP_LIMIT = {"single": 4.0, "double": 8.0}


def loop_draws(model, nb=LOOP_NB, seed=131):
    """-> x0 [nx, nb] (b_x and the angles off the upright by up to LOOP_SPREAD, at rest), u_init [T, nb] zeros, the target [nx]
    (the upright at b_x = 0), the terminal weights 10 q.  The draws are those of LOOP_NB lanes whatever nb is."""
    nx, nq = sj.NX[model], sj.NX[model] // 2
    rng = np.random.default_rng(seed + nx)
    s = LOOP_SPREAD[model]
    x = np.zeros((nx, LOOP_NB))
    x[0] = rng.uniform(-s, s, LOOP_NB)
    x[1:nq] = np.pi / 2 + rng.uniform(-s, s, (nq - 1, LOOP_NB))
    target = np.zeros(nx)
    target[1:nq] = np.pi / 2
    return x[:, :nb].copy(), np.zeros((LOOP_T, nb)), target, [10.0 * v for v in Q[model]]


# The reference loop's converged costs on all LOOP_NB lanes take a minute to compute, so the GPU test reads them from
# tests/golden/sim_ilqr_loop_costs.json: entry "<model>_<free|clamped>" [LOOP_NB], loop_batch's cost after LOOP_ITERS iterations.
# tests/test_sim_ilqr_ref.py recomputes the first lanes and holds the file to them; write_loop_golden() remakes it.
LOOP_GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "sim_ilqr_loop_costs.json")


def loop_limit(model, clamped):
    return LOOP_LIMIT[model] if clamped else np.inf


def loop_reference(orc, model, clamped, nb=LOOP_NB, iterations=LOOP_ITERS):
    x0, u0, target, qf = loop_draws(model, nb)
    return loop_batch(orc, model, sj.DYN[model], LOOP_DT, x0, u0, target, Q[model], R, qf, None, loop_limit(model, clamped),
                      iterations, LOOP_TRIALS)


def loop_golden():
    with open(LOOP_GOLDEN) as fh:
        return {k: np.array(v) for k, v in json.load(fh).items()}


def write_loop_golden(orc):
    with open(LOOP_GOLDEN, "w") as fh:
        json.dump({"%s_%s" % (m, "clamped" if c else "free"): [float(v) for v in loop_reference(orc, m, c)["cost"]]
                   for m in ("single", "double") for c in (False, True)}, fh, indent=0)
