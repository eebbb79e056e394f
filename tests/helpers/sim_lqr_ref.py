"""Numpy reference for the time-varying LQR gains along a plant trajectory and for the plant under an affine feedback law
(include/cpmpc.h: cpmpc_sim_lqr_batch, cpmpc_sim_rollout_fb_batch), formulated differently from the kernels on purpose.  Built
on the CPU oracle through sim_jac_ref.step_ref.  TEST INFRASTRUCTURE ONLY.

  trajectory      xs [T, nx], Phi [T, nx, nx], gamma [T, nx] of one problem: the ticks' x+, A and Bu chained from x0
  riccati         the TEXTBOOK recursion P = Q + Phi^T P Phi - Phi^T P gamma (r + gamma^T P gamma)^-1 gamma^T P Phi with
                  k = -(r + gamma^T P gamma)^-1 gamma^T P Phi -> K [T, nx], P0 [nx, nx].  `dtype` is the type the algebra runs in:
                  np.float32 redoes ONLY the recursion in float32, on the float64 Phi and gamma
  dense_lqr       the T-step problem stacked and solved as ONE least-squares system in the T control deviations -> K_0, P0
  closed_loop     the feedback rollout through step_ref: d = wrap(x - x_nom), u = clamp(u_nom + K . d) -> xs [T, nx], us [T]
  lqr_batch / closed_loop_batch   the same for [nx, B] states
  CASES / inputs, FB_CASES / fb_inputs   the cases of tests/test_gpu_sim_lqr.py and their draws, pinned as admissible by
                  tests/test_sim_lqr_ref.py
  tracking_draws  the tracking test's nominal trajectories near the upright and the perturbed starts"""
import numpy as np

from helpers import sim_jac_ref as sj
from helpers import sim_rollout_ref as sr


def wrap_nearest(model, d):
    """a difference of states, its pole angles to the nearest multiple of 2 pi"""
    d = np.array(d, dtype=np.float64)
    nq = sj.NX[model] // 2
    d[1:nq] = d[1:nq] - 2 * np.pi * np.round(d[1:nq] / (2 * np.pi))
    return d


def trajectory(orc, model, params, dt, x0, us, fext=None):
    nx, T = sj.NX[model], len(us)
    fb, fm = (None, None) if fext is None else (fext[:2], fext[2:])
    xs, Phi, gam = np.zeros((T, nx)), np.zeros((T, nx, nx)), np.zeros((T, nx))
    x = np.asarray(x0, dtype=np.float64)
    for t in range(T):
        x, Phi[t], gam[t] = sj.step_ref(orc, model, params, dt, x, float(us[t]), fb, fm)
        xs[t] = x
    return xs, Phi, gam


def terminal_matrix(q, terminal):
    """P_T of a case: None -> diag(q), nx numbers -> their diagonal, a matrix -> its lower triangle mirrored"""
    if terminal is None:
        return np.diag(np.asarray(q, dtype=np.float64))
    t = np.asarray(terminal, dtype=np.float64)
    if t.ndim == 1:
        return np.diag(t)
    L = np.tril(t)
    return L + L.T - np.diag(np.diag(L))


def riccati(Phi, gam, q, r, PT, dtype=np.float64):
    T, nx = gam.shape
    Q = np.diag(np.asarray(q, dtype=np.float64)).astype(dtype)
    P = np.asarray(PT, dtype=np.float64).astype(dtype)
    K = np.zeros((T, nx), dtype=dtype)
    for t in range(T - 1, -1, -1):
        A, g = Phi[t].astype(dtype), gam[t].astype(dtype)
        s = dtype(r) + g @ P @ g
        gPA = g @ P @ A
        K[t] = -gPA / s
        P = Q + A.T @ P @ A - np.outer(gPA, gPA) / s
        P = (P + P.T) / dtype(2)
    return K.astype(np.float64), P.astype(np.float64)


def _sqrt_psd(M):
    w, V = np.linalg.eigh(M)
    return (V * np.sqrt(np.maximum(w, 0.0))) @ V.T


def dense_lqr(Phi, gam, q, r, PT):
    """min over du_0 .. du_{T-1} of sum_t |Q^1/2 d_t|^2 + r du_t^2 + |P_T^1/2 d_T|^2 with d_{t+1} = Phi_t d_t + gamma_t du_t, as
    one least-squares system per unit start d_0 = e_i: the minimiser is linear in d_0, du = G d_0 -> K_0 = G[0], and the
    optimal cost d_0^T P0 d_0."""
    T, nx = gam.shape
    sq, sr_, sT = np.diag(np.sqrt(np.asarray(q, dtype=np.float64))), np.sqrt(r), _sqrt_psd(PT)
    # d_t = F[t] d_0 + sum_s G_[t][s] du_s
    F = [np.eye(nx)]
    Gm = [np.zeros((nx, T))]
    for t in range(T):
        F.append(Phi[t] @ F[-1])
        g = Phi[t] @ Gm[-1]
        g[:, t] += gam[t]
        Gm.append(g)
    rows_u, rows_0 = [], []
    for t in range(T):
        rows_u.append(sq @ Gm[t])
        rows_0.append(sq @ F[t])
        e = np.zeros((1, T))
        e[0, t] = sr_
        rows_u.append(e)
        rows_0.append(np.zeros((1, nx)))
    rows_u.append(sT @ Gm[T])
    rows_0.append(sT @ F[T])
    Mu, M0 = np.vstack(rows_u), np.vstack(rows_0)
    G = -np.linalg.lstsq(Mu, M0, rcond=None)[0]
    R0 = M0 + Mu @ G
    return G[0], R0.T @ R0


def closed_loop(orc, model, params, dt, x0, u_nom, K, x0_nom, xs_nom, u_limit=np.inf, fext=None):
    nx, T = sj.NX[model], len(u_nom)
    fb, fm = (None, None) if fext is None else (fext[:2], fext[2:])
    x = np.asarray(x0, dtype=np.float64)
    xs, us = np.zeros((T, nx)), np.zeros(T)
    for t in range(T):
        u = float(u_nom[t])
        if K is not None:
            xn = x0_nom if t == 0 else xs_nom[t - 1]
            u += float(np.asarray(K[t], dtype=np.float64) @ wrap_nearest(model, x - np.asarray(xn, dtype=np.float64)))
        u = min(max(u, -u_limit), u_limit)
        x, _, _ = sj.step_ref(orc, model, params, dt, x, u, fb, fm)
        xs[t], us[t] = x, u
    return xs, us


def lqr_batch(orc, model, params, dt, x0, us, q, r, terminal=None, fext=None, dtype=np.float64, dense=False):
    """x0 [nx, B], us [T, B], terminal None, nx numbers or [nx, nx, B], params np numbers or [np, B], fext None, 4 shared numbers
    or [4, B] -> dict xs [T, nx, B], K [T, nx, B], P0 [nx, nx, B], gam_max [T, B] (the ticks' largest |gamma| entry), and with
    `dense` K0_dense [nx, B], P0_dense [nx, nx, B]"""
    nx, nb = x0.shape
    T = us.shape[0]
    out = dict(xs=np.zeros((T, nx, nb)), K=np.zeros((T, nx, nb)), P0=np.zeros((nx, nx, nb)), gam_max=np.zeros((T, nb)))
    if dense:
        out.update(K0_dense=np.zeros((nx, nb)), P0_dense=np.zeros((nx, nx, nb)))
    for b in range(nb):
        xs, Phi, gam = trajectory(orc, model, sr._params(params, b), dt, x0[:, b], us[:, b], sr._lane(fext, b))
        term = terminal[:, :, b] if isinstance(terminal, np.ndarray) and terminal.ndim == 3 else terminal
        PT = terminal_matrix(q, term)
        out["xs"][:, :, b], out["gam_max"][:, b] = xs, np.abs(gam).max(axis=1)
        out["K"][:, :, b], out["P0"][:, :, b] = riccati(Phi, gam, q, r, PT, dtype)
        if dense:
            out["K0_dense"][:, b], out["P0_dense"][:, :, b] = dense_lqr(Phi, gam, q, r, PT)
    return out


def closed_loop_batch(orc, model, params, dt, x0, u_nom, K, x0_nom, xs_nom, u_limit=np.inf, fext=None):
    nx, nb = x0.shape
    T = u_nom.shape[0]
    xs, us = np.zeros((T, nx, nb)), np.zeros((T, nb))
    for b in range(nb):
        xs[:, :, b], us[:, b] = closed_loop(orc, model, sr._params(params, b), dt, x0[:, b], u_nom[:, b],
                                            None if K is None else K[:, :, b], None if K is None else x0_nom[:, b],
                                            None if K is None else xs_nom[:, :, b], u_limit, sr._lane(fext, b))
    return xs, us


# ---- the cases of tests/test_gpu_sim_lqr.py ---------------------------------------------------------------------------------
B = 130
DT_T = ((0.0105, 5), (0.02, 3), (0.001, 8), (0.0, 3), (0.01, 12))
# (model, dt, T, kind): kind None; "dyn" per-problem parameters; "shared" / "per" external forces (4-state model: the reference
# has forces for it alone); "PT" a tensor terminal cost
CASES = [(m, dt, nt, None) for m in ("single", "double") for dt, nt in DT_T] + \
        [("single", 0.0105, 5, "dyn"), ("double", 0.0105, 5, "dyn"), ("single", 0.0105, 5, "shared"), ("single", 0.0105, 5, "per"),
         ("single", 0.0105, 5, "PT"), ("double", 0.0105, 5, "PT"), ("single", 0.0105, 1, None), ("double", 0.0105, 1, None)]
IDS = ["%s-%g-%d-%s" % c for c in CASES]
SHARED_F = ((1.5, 0.0), (-2.0, 1.0))
Q = {"single": (1.0, 10.0, 0.1, 0.1), "double": (1.0, 10.0, 10.0, 0.1, 0.1, 0.1)}
R = 0.01


def terminal_costs(model, nb, seed=61):
    """PT [nx, nx, nb]: diag(10 q) plus a tenth of a random correlation matrix scaled into it -- positive definite, not diagonal"""
    nx = sj.NX[model]
    rng = np.random.default_rng(seed + nx)
    d = np.sqrt(10.0 * np.array(Q[model]))
    P = np.zeros((nx, nx, nb))
    for b in range(nb):
        G = rng.normal(size=(nx, nx))
        S = G @ G.T
        c = 1.0 / np.sqrt(np.diag(S))
        M = np.diag(d * d) + 0.1 * (S * c[:, None] * c[None, :]) * d[:, None] * d[None, :]
        P[:, :, b] = (M + M.T) / 2     # symmetric to the bit: the calls read the lower triangle and mirror it
    return P


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _plant_draws(model, kind, nb):
    f = None
    if kind == "shared":
        f = np.array([SHARED_F[0][0], SHARED_F[0][1], SHARED_F[1][0], SHARED_F[1][1]])
    elif kind == "per":
        f = np.random.default_rng(21).uniform(-3.0, 3.0, (4, nb))
    prm = np.array(sj.DYN[model])
    if kind == "dyn":
        prm = np.tile(prm[:, None], (1, nb)) * np.random.default_rng(43).uniform(0.8, 1.2, (len(prm), nb))
    return f, prm


_IN, _FB = {}, {}


def inputs(orc, case, nb=B):
    """numpy inputs of a case, made once and left unchanged: dict x0 [nx, nb], us [T, nb], f (None, 4 shared numbers or [4, nb]),
    prm (np numbers or [np, nb]), q [nx], r, PT (None or [nx, nx, nb])"""
    key = (case, nb)
    if key not in _IN:
        model, dt, nt, kind = case
        x, _ = sj.states(model, nb)
        us = np.random.default_rng(53).uniform(-20.0, 20.0, (nt, nb))
        f, prm = _plant_draws(model, kind, nb)
        _IN[key] = _freeze(dict(x0=x, us=us, f=f, prm=prm, q=np.array(Q[model]), r=R,
                                PT=terminal_costs(model, nb) if kind == "PT" else None))
    return _IN[key]


def reference(orc, case, nb=B, dtype=np.float64, arrays=None, dense=False):
    """lqr_batch on the case's inputs, or on `arrays` (the same dict with the values a float tensor holds) -> its dict"""
    i = inputs(orc, case, nb) if arrays is None else arrays
    return lqr_batch(orc, case[0], i["prm"], case[1], i["x0"], i["us"], i["q"], i["r"], i["PT"], i["f"], dtype=dtype, dense=dense)


# The feedback rollout's cases (model, dt, T, kind): kind None -- the plant is the nominal's, no clamp; "clamp" -- u_limit =
# FB_LIMIT; "mismatch" -- the plant's parameters are per problem, 0.9 .. 1.1 of the nominal's; "per" -- forces on the plant that
# the nominal never saw; "noK" -- K is None
FB_LIMIT = 10.0
FB_CASES = [(m, dt, nt, None) for m in ("single", "double") for dt, nt in ((0.0105, 5), (0.001, 8), (0.0, 3), (0.0105, 1))] + \
           [(m, 0.0105, 5, k) for m in ("single", "double") for k in ("clamp", "mismatch", "noK")] + [("single", 0.0105, 5, "per")]
FB_IDS = ["%s-%g-%d-%s" % c for c in FB_CASES]


def fb_inputs(orc, case, nb=B):
    """numpy inputs of a feedback case, made once and left unchanged: dict x0 [nx, nb] (the nominal start moved by up to 0.05 a
    state and wrapped; lanes 0 and 1 pushed over the +-pi cut), u_nom [T, nb], K [T, nx, nb] (the reference's gains along the
    nominal; None for "noK"), x0_nom, xs_nom, prm (the PLANT's), f (the plant's forces), u_limit"""
    key = (case, nb)
    if key not in _FB:
        model, dt, nt, kind = case
        nx, nq = sj.NX[model], sj.NX[model] // 2
        x_nom, _ = sj.states(model, nb)
        u_nom = np.random.default_rng(53).uniform(-20.0, 20.0, (nt, nb))
        nom = lqr_batch(orc, model, sj.DYN[model], dt, x_nom, u_nom, Q[model], R)
        d = np.random.default_rng(67).uniform(-0.05, 0.05, (nx, nb))
        if nb >= 8:
            d[1:nq, :2] = 0.001          # 3.1414 + 0.001 lies beyond pi: the state is on the other side of the cut
        x0 = x_nom + d
        for b in range(nb):
            x0[:, b] = sj._wrap(orc, model, x0[:, b])
        prm = np.array(sj.DYN[model])
        if kind == "mismatch":
            prm = np.tile(prm[:, None], (1, nb)) * np.random.default_rng(71).uniform(0.9, 1.1, (len(prm), nb))
        f = np.random.default_rng(21).uniform(-3.0, 3.0, (4, nb)) if kind == "per" else None
        _FB[key] = _freeze(dict(x0=x0, u_nom=u_nom, K=None if kind == "noK" else nom["K"], x0_nom=x_nom, xs_nom=nom["xs"],
                                prm=prm, f=f, u_limit=FB_LIMIT if kind == "clamp" else np.inf, gam_max=nom["gam_max"]))
    return _FB[key]


def fb_reference(orc, case, nb=B, arrays=None):
    i = fb_inputs(orc, case, nb) if arrays is None else arrays
    return closed_loop_batch(orc, case[0], i["prm"], case[1], i["x0"], i["u_nom"], i["K"], i["x0_nom"], i["xs_nom"],
                             i["u_limit"], i["f"])


# ---- tracking: a nominal trajectory near the upright, 60 ticks of 10 ms, the start moved by 1e-2 ----------------------------------
TRACK_DT, TRACK_T, TRACK_DELTA, TRACK_RATIO = 0.01, 60, 1e-2, 0.25
TRACK_GROWTH = 4.0   # the premise: on every lane the open loop ends at least this many times further off than it began


def tracking_draws(model, nb=B, seed=73):
    """-> the nominal start [nx, nb] (b_x +-0.3, angles pi/2 +-0.05, velocities +-0.2), u_nom [60, nb] (+-2), the perturbed
    start, the terminal weights 10 q.  The start is moved by |delta| = 1e-2 in a random DIAGONAL direction: every state by
    1e-2 / sqrt(nx) with a random sign.  The condition compares the closed loop with the open loop's divergence, so it says
    something only where the open loop does diverge: a direction drawn uniformly from the sphere has, on a lane in fifty, next
    to no component along the unstable modes, and there both loops merely stay where they started; with every state moved the
    angles always are (tests/test_sim_lqr_ref.py asserts the open loop's growth).  The draws are those of B lanes whatever nb
    is: the first nb of them."""
    nx, nq = sj.NX[model], sj.NX[model] // 2
    rng = np.random.default_rng(seed + nx)
    x = np.concatenate([rng.uniform(-0.3, 0.3, (1, B)), np.pi / 2 + rng.uniform(-0.05, 0.05, (nq - 1, B)),
                        rng.uniform(-0.2, 0.2, (nq, B))])
    u = rng.uniform(-2.0, 2.0, (TRACK_T, B))
    d = rng.choice([-1.0, 1.0], (nx, B)) * TRACK_DELTA / np.sqrt(nx)
    return x[:, :nb].copy(), u[:, :nb].copy(), (x + d)[:, :nb].copy(), [10.0 * v for v in Q[model]]


def deviation(model, x, x_nom):
    """per lane, the Euclidean norm of x - x_nom [nx, B], pole angles wrapped"""
    d = x - x_nom
    nq = sj.NX[model] // 2
    d[1:nq] = d[1:nq] - 2 * np.pi * np.round(d[1:nq] / (2 * np.pi))
    return np.linalg.norm(d, axis=0)
