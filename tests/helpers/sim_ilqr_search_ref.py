"""Numpy reference of the line search of one iLQR iteration (include/cpmpc.h: cpmpc_sim_ilqr_search_batch; batch.py:
sim_ilqr_search), built on sim_ilqr_ref.forward and nothing else of the kernels.  TEST INFRASTRUCTURE ONLY.

  search            one problem's trial ladder from its nominal: alpha = 1, halved until the rolled cost passes the Armijo test
                    against cost_nom and dV, at most `trials` times -> dict xs, us, cost, alpha (0: no step, the nominal by
                    copy), rolls (the forward passes it took: 1 where alpha = 1 is accepted, `trials` where nothing is)
  loop_with_search  sim_ilqr_ref.loop with search() in the ladder's place -> loop's dict, and "alpha" [iterations]: the step
                    of every iteration, and "rolls" [iterations]
  LOOP_LANES        the lanes of the loop configurations the tests use: the first 8 (4-state) and the first 4 (6-state)"""
import numpy as np

from helpers import sim_ilqr_ref as il

LOOP_LANES = {"single": 8, "double": 4}
RUNGS = tuple(0.5 ** j for j in range(il.LOOP_TRIALS))


def search(orc, model, params, dt, x0, u_nom, xs_nom, cost_nom, kff, K, dV, u_limit, xref, uref, q, r, PT, trials=6,
           armijo=il.ARMIJO, fext=None):
    alpha = 1.0
    for j in range(trials):
        xs, us, J = il.forward(orc, model, params, dt, x0, u_nom, kff, K, x0, xs_nom, alpha, u_limit, xref, uref, q, r, PT,
                               fext=fext)
        pred = dV[0] * alpha + dV[1] * alpha * alpha
        if pred < 0 and J - cost_nom <= armijo * pred:
            return dict(xs=xs, us=us, cost=J, alpha=alpha, rolls=j + 1)
        alpha *= 0.5
    return dict(xs=np.array(xs_nom, dtype=np.float64), us=np.array(u_nom, dtype=np.float64), cost=cost_nom, alpha=0.0,
                rolls=trials)


def loop_with_search(orc, model, params, dt, x0, u_init, xref, uref, q, r, PT, u_limit=np.inf, iterations=10, trials=6,
                     mu_init=0.0, fext=None):
    args = (xref, uref, q, r, PT)
    xs, us, J = il.forward(orc, model, params, dt, x0, u_init, None, None, None, None, 1.0, u_limit, *args, fext=fext)
    mu, hist, acc, alphas, rolls = float(mu_init), [J], [], [], []
    for _ in range(iterations):
        _, Phi, gam = il.linearise(orc, model, params, dt, x0, us, fext)
        bw = il.backward(Phi, gam, il.residuals(model, x0, xs, xref), us, uref, q, r, PT, mu, u_limit)
        s = search(orc, model, params, dt, x0, us, xs, J, bw["kff"], bw["K"], bw["dV"], u_limit, *args, trials=trials, fext=fext)
        xs, us, J = s["xs"], s["us"], s["cost"]
        done = s["alpha"] > 0
        if done:
            mu = mu / 10.0
            mu = 0.0 if mu < 1e-6 else mu
        else:
            mu = max(10.0 * mu, 1e-3)
        hist.append(J)
        acc.append(done)
        alphas.append(s["alpha"])
        rolls.append(s["rolls"])
    _, Phi, gam = il.linearise(orc, model, params, dt, x0, us, fext)
    last = il.backward(Phi, gam, il.residuals(model, x0, xs, xref), us, uref, q, r, PT, mu, u_limit)
    return dict(u=us, xs=xs, cost=J, cost_history=np.array(hist), mu=mu, accepted=np.array(acc, dtype=bool), hmax=last["hmax"],
                K=last["K"], alpha=np.array(alphas), rolls=np.array(rolls))
