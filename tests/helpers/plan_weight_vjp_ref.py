"""Numpy references for the gradients of a loss on the planned controls with respect to the COST WEIGHTS (include/cpmpc.h:
cpmpc_plan_weight_vjp_batch): for a cotangent gbar = dL/du+ on the controls u+ = u + du of the undamped, unclamped Gauss-Newton
QP at z,
    g_tw [NX] (the terminal weights, state order),  g_wu (u_cost_weight),  g_wdu (u_derivative_cost_weight),
and the primal QP step du itself.  Built on tests/helpers/feedback_ref.py, plan_sensitivity_ref.py, plan_vjp_ref.py and the
CPU oracle's problem functions.  TEST INFRASTRUCTURE ONLY.

  dense_weight_vjp      two solves of the symmetric KKT system [[J^T J, A^T], [A, 0]]: the primal [dz; nu] = KKT^-1 [-J^T r; -c]
                        and the adjoint [y; mu] = KKT^-1 [E gbar; 0]; with rho = r + J dz the gradient with respect to the
                        weight of cost row i is -(2 / w_i) (J_i y) rho_i.  The rows of a weight are found as the rows of J that
                        move when the weight moves.  Also returns du and `scale`
  scale                 per output the sum of |2 / w_i . J_i y . rho_i| over that output's rows: cancellation-free, non-zero for
                        any cost row with a positive weight.  Every relative error of a gradient is |g - g_ref| / scale
  fd_weight_vjp         central differences of gbar . du through params_for, u_cost_weight and u_derivative_cost_weight, per
                        weight FIELD (the 6-state model's poles share theirs): see by_field
  condensed_weight_vjp  the kernel's recurrences (csrc/plan_weight_vjp_kernels.hpp), `lin` the precision of Phi, Gamma, Psi, w_k
                        and of what travels through the workspace, as in the sibling helpers
  golden                tests/golden/plan_weight_vjp_sample.json
Gradients are packed as one vector [g_tw (NX), g_wu, g_wdu] per problem."""
import json
import os

import numpy as np

from helpers import feedback_ref as fr
from helpers import plan_sensitivity_ref as ps
from helpers import plan_vjp_ref as pv

GOLDEN_PATH = os.path.join(fr.ROOT, "tests", "golden", "plan_weight_vjp_sample.json")
COTANGENTS = pv.COTANGENTS
X0_SHIFT, SET_POINT, U_PREV = 0.01, 0.3, 0.7   # the sample: x0 = the sample state + 0.01, so that dz and rho are generic
TERMINAL_FIELDS = ("b_x_final_cost_weight", "th_final_cost_weight", "b_x_dot_final_cost_weight", "th_dot_final_cost_weight")
FIELDS = TERMINAL_FIELDS + ("u_cost_weight", "u_derivative_cost_weight")


def _copy(p):
    return type(p).from_buffer_copy(p)


def _field_of_state(t, nx):
    nq = nx // 2
    return 0 if t == 0 else (1 if t < nq else (2 if t == nq else 3))


def terminal_weights_of(p, nx):
    """The NX terminal weights of p in state order (negative: an equality row)."""
    return np.array([getattr(p, TERMINAL_FIELDS[_field_of_state(t, nx)]) for t in range(nx)], dtype=np.float64)


def by_field(g, nx):
    """[6]: the packed gradient summed over the states that share a weight field (FIELDS order)."""
    out = np.zeros(6)
    for t in range(nx):
        out[_field_of_state(t, nx)] += g[t]
    out[4], out[5] = g[nx], g[nx + 1]
    return out


def _wrap(v):
    return v - 2.0 * np.pi * np.round(v / (2.0 * np.pi))


def _primal(orc, model, p, dyn, z, x0, set_point, u_prev):
    r, c, J, A = fr.problem_eval(orc, model, p, dyn, x0, set_point, u_prev, z)
    kkt = ps._kkt(J, A)
    dz = np.linalg.solve(kkt, np.concatenate([-J.T @ r, -c]))[:A.shape[1]]
    return r, J, A, kkt, dz


def dense_weight_vjp(orc, p, dyn, z, x0, gbar, set_point=SET_POINT, u_prev=U_PREV, terminal_weights=None, model="single"):
    """(g [NX + 2], du [N], scale [NX + 2]).  An equality row (weight < 0), a zero weight and an absent control row (weight
    <= 0) give exactly 0, with scale 0."""
    nx, N, sp, S = fr._shape(orc, model, p)
    if terminal_weights is not None:
        p = fr.params_for(orc, model, sp, terminal_weights)
    z = np.asarray(z, dtype=np.float64)
    r, J, A, kkt, dz = _primal(orc, model, p, dyn, z, x0, set_point, u_prev)
    dim, n_eq = A.shape[1], A.shape[0]
    rhs = np.zeros(dim + n_eq)
    rhs[nx * S:dim] = pv._padded(gbar, N)
    y = np.linalg.solve(kkt, rhs)[:dim]
    rho, Jy = r + J @ dz, J @ y
    g, scale = np.zeros(nx + 2), np.zeros(nx + 2)
    for f, name in enumerate(FIELDS):
        w = float(getattr(p, name))
        if not w > 0.0:
            continue
        p2 = _copy(p)
        setattr(p2, name, w + 1.0)
        _, _, J2, _ = fr.problem_eval(orc, model, p2, dyn, x0, set_point, u_prev, z)
        assert J2.shape == J.shape
        for i in np.flatnonzero(np.any(J2 != J, axis=1)):
            if f < 4:   # a terminal row touches one state of the last node
                cols = np.flatnonzero(J2[i])
                assert cols.size == 1 and nx * (S - 1) <= cols[0] < nx * S
                out = int(cols[0]) - nx * (S - 1)
                assert _field_of_state(out, nx) == f
            else:
                out = nx + f - 4
            term = (2.0 / w) * Jy[i] * rho[i]
            g[out] -= term
            scale[out] += abs(term)
    return g, dz[nx * S:], scale


def _loss(orc, model, p, dyn, z, x0, set_point, u_prev, gbar, nx, N, S):
    return float(pv._padded(gbar, N) @ _primal(orc, model, p, dyn, z, x0, set_point, u_prev)[4][nx * S:])


def fd_weight_vjp(orc, p, dyn, z, x0, gbar, set_point=SET_POINT, u_prev=U_PREV, model="single", h=1e-5):
    """[6] in FIELDS order: central differences of gbar . du in each weight field; 0 for a field whose weight is not positive
    (an equality row, or a row that does not exist)."""
    nx, N, sp, S = fr._shape(orc, model, p)
    out = np.zeros(6)
    for f, name in enumerate(FIELDS):
        w = float(getattr(p, name))
        if not w > 0.0:
            continue
        L = []
        for sgn in (1.0, -1.0):
            p2 = _copy(p)
            setattr(p2, name, w + sgn * h)
            L.append(_loss(orc, model, p2, dyn, np.asarray(z, dtype=np.float64), x0, set_point, u_prev, gbar, nx, N, S))
        out[f] = (L[0] - L[1]) / (2.0 * h)
    return out


def condensed_weight_vjp(Phi, Gam, cs, tw, wu, wd, sp, ci, e_term, u, u_prev, gbar, lin=np.float64):
    """(g [NX + 2], du [N]) in the kernel's recurrences.  tw: the NX terminal weights (negative: equality); cs [S - 1, NX] the
    shooting defects, ci = wrap(z_0 - x0), e_term = wrap(z_{S-1} - target).  `lin`: the type Phi, Gamma, Psi, w_k, upsilon,
    1 / d, the controls, the control-cost gradient and everything that travels through Wk / Tk ((U^-1 g)_k, eta_k) are carried
    in; S, rho, a, eta's recurrence, the free response, the LDL^T, both solves and the ascending pass stay in double."""
    N, nx = Gam.shape
    S1 = Phi.shape[0]
    gb = pv._padded(gbar, N)
    tw = np.asarray(tw, dtype=np.float64)
    Rw, Dg = np.where(tw >= 0, tw, 1.0).astype(lin), (tw >= 0).astype(np.float64)
    Phi, Gam, cs, u = Phi.astype(lin), Gam.astype(lin), cs.astype(lin), np.asarray(u).astype(lin)
    ci, e_term, u_prev = np.asarray(ci).astype(lin), np.asarray(e_term).astype(lin), lin(u_prev)
    wu2, wd2 = lin(wu) * lin(wu), lin(wd) * lin(wd)
    Psi = np.diag(Rw)
    Wm = np.zeros((N, nx), dtype=lin)
    ups, inv_d, gws, etas = (np.zeros(N, dtype=lin) for _ in range(4))
    Sm, rho, av, ha = np.zeros((nx, nx)), np.zeros(nx), np.zeros(nx), np.zeros(nx)
    wk, d_next, gw, eta = np.zeros(nx, dtype=lin), lin(1), lin(0), 0.0
    for s in range(S1 - 1, -1, -1):
        for k in range(sp * (s + 1) - 1, sp * s - 1, -1):
            u_lo = u[k - 1] if k > 0 else u_prev
            g = wu2 * u[k] + wd2 * (u[k] - u_lo)
            if k < N - 1:
                g = g + wd2 * (u[k] - u[k + 1])
            nd = lin(2) if k < N - 1 else lin(1)
            ups[k] = -wd2 / d_next if k < N - 1 else lin(0)
            dk = (wu2 + wd2 * nd) + wd2 * ups[k]
            assert dk > 0
            inv_d[k] = lin(1) / dk
            d_next = dk
            wk = Psi @ Gam[k] - ups[k] * wk
            gw = lin(g - ups[k] * gw)
            eta = gb[k] - np.float64(ups[k]) * eta
            Wm[k], gws[k], etas[k] = wk, gw, lin(eta)
            wi = wk.astype(np.float64) * np.float64(inv_d[k])
            rho += wi * np.float64(gw)
            av += wi * eta
            Sm += np.outer(wi, wk.astype(np.float64))
        ha += Psi.astype(np.float64) @ cs[s].astype(np.float64)
        Psi = (Psi @ Phi[s]).astype(lin)
    hv = Rw.astype(np.float64) * e_term.astype(np.float64) + ha - Psi.astype(np.float64) @ ci.astype(np.float64)
    Sm = Sm + np.diag(Dg)
    L, d = np.eye(nx), np.zeros(nx)   # LDL^T without pivoting, as the kernel
    for j in range(nx):
        d[j] = Sm[j, j] - np.sum(L[j, :j] ** 2 * d[:j])
        assert d[j] > 0
        for i in range(j + 1, nx):
            L[i, j] = (Sm[i, j] - np.sum(L[i, :j] * L[j, :j] * d[:j])) / d[j]

    def solve(b):
        return np.linalg.solve(L.T, np.linalg.solve(L, b) / d)
    qp, qa = solve(hv - rho), solve(av)
    out = np.zeros(nx + 2)
    for t in range(nx):   # a cost row's multiplier IS its linearised residual: q_p = w (e + dx), q_a = w yx
        if tw[t] > 0:
            out[t] = -2.0 * qa[t] * qp[t] / np.float64(Rw[t])
    W64, id64, ups64 = Wm.astype(np.float64), inv_d.astype(np.float64), ups.astype(np.float64)
    du = np.zeros(N)
    du_prev = y_prev = ups_prev = 0.0
    v_prev, s_u, s_d = np.float64(u_prev), 0.0, 0.0
    for k in range(N):
        du[k] = -(np.float64(gws[k]) + W64[k] @ qp) * id64[k] - ups_prev * du_prev
        yk = (np.float64(etas[k]) - W64[k] @ qa) * id64[k] - ups_prev * y_prev
        v = np.float64(u[k]) + du[k]
        s_u += yk * v
        s_d += (y_prev - yk) * (v_prev - v)
        du_prev, y_prev, v_prev, ups_prev = du[k], yk, v, ups64[k]
    out[nx] = -2.0 * np.float64(lin(wu)) * s_u
    out[nx + 1] = -2.0 * np.float64(lin(wd)) * s_d
    return out, du


def targets(nx, set_point):
    nq = nx // 2
    return np.array([set_point] + [np.pi / 2] * (nq - 1) + [0.0] * nq)


def condensed_ref(orc, p, dyn, z, x0, gbar, set_point=SET_POINT, u_prev=U_PREV, terminal_weights=None, model="single",
                  lin=np.float64, blocks=None):
    """(g, du) of the condensed form from the blocks of the oracle's A and its defects at z.  blocks: (Phi, Gam) to use
    instead of the oracle's (tests/helpers/plan_shapes.py perturbs them, or takes the single-precision oracle's)."""
    nx, N, sp, S = fr._shape(orc, model, p)
    nq = nx // 2
    z = np.asarray(z, dtype=np.float64)
    Phi, Gam = fr.blocks_of(orc, p, dyn, z, model) if blocks is None else blocks
    _, c, _, _ = fr.problem_eval(orc, model, p, dyn, x0, set_point, u_prev, z)
    cs = c[:nx * (S - 1)].reshape(S - 1, nx)
    ci = z[:nx] - np.asarray(x0, dtype=np.float64)
    e_term = z[nx * (S - 1):nx * S] - targets(nx, set_point)
    ci[1:nq], e_term[1:nq] = _wrap(ci[1:nq]), _wrap(e_term[1:nq])
    tw = terminal_weights_of(p, nx) if terminal_weights is None else np.asarray(terminal_weights, dtype=np.float64)
    return condensed_weight_vjp(Phi, Gam, cs, tw, max(p.u_cost_weight, 0.0), max(p.u_derivative_cost_weight, 0.0), sp, ci,
                                e_term, z[nx * S:], u_prev, gbar, lin=lin)


def rel_err(g, g_ref, scale):
    """max over the outputs with a non-zero scale of |g - g_ref| / scale; an output whose scale is 0 (an equality row, a zero
    weight) must be exactly 0."""
    g, live = np.asarray(g, dtype=np.float64), scale > 0
    assert np.all(g[~live] == 0.0), g[~live]
    return float((np.abs(g - g_ref)[live] / scale[live]).max())


def rel_err_du(du, du_ref):
    n = len(du)
    return float(np.abs(np.asarray(du, dtype=np.float64) - du_ref[:n]).max() / np.abs(du_ref).max())


def sample_inputs(x0_sample):
    """The states the weight-gradient sample is evaluated at: the gain sample's + 0.01 (z stays that sample's solution)."""
    return np.asarray(x0_sample, dtype=np.float64) + X0_SHIFT


# ---- the golden file ---------------------------------------------------------------------------------------------
def make_golden(orc):
    out = {"about": "gradients of gbar . du+ with respect to the cost weights, [g_tw (NX), g_wu, g_wdu], and the primal QP step "
                    "du: per configuration (the seeds, and so the z, of feedback_gain_sample.json; x0 = the sample state + %g, "
                    "set-point %g, u_prev %g) and per cotangent of plan_vjp_sample.json the worst difference between the "
                    "condensed form and the dense KKT solves over the %d-lane sample -- gradients relative to `scale` "
                    "(sum |2 / w_i . J_i y . rho_i| over an output's rows), du relative to max |du_ref| -- and the dense "
                    "[g (NX + 2), du_0, du_1] of %d lanes (12 digits) (tests/helpers/plan_weight_vjp_ref.py)"
                    % (X0_SHIFT, SET_POINT, U_PREV, fr.SAMPLE_LANES, fr.GOLDEN_LANES),
           "configs": {}}
    for model, sp, mix in fr.configs():
        p, tw, xs, z = fr.solve_sample(orc, model, sp, mix, fr.SAMPLE_LANES)
        x0 = sample_inputs(xs)
        cots = pv.cotangents(model, sp, mix, fr.SAMPLE_LANES, int(p.window_length))
        cfg = {"seed": fr.config_seed(model, sp, mix), "sample_lanes": fr.SAMPLE_LANES}
        for name in COTANGENTS:
            worst, worst_du, rows = 0.0, 0.0, []
            for b in range(fr.SAMPLE_LANES):
                gd, dud, sc = dense_weight_vjp(orc, p, fr.DYN[model], z[:, b], x0[:, b], cots[name][:, b], model=model)
                gc, duc = condensed_ref(orc, p, fr.DYN[model], z[:, b], x0[:, b], cots[name][:, b], model=model)
                worst, worst_du = max(worst, rel_err(gc, gd, sc)), max(worst_du, rel_err_du(duc, dud))
                if b < fr.GOLDEN_LANES:
                    rows.append(fr._rounded(np.concatenate([gd, dud[:2]]), 12))
            cfg["worst_rel_" + name], cfg["worst_rel_du_" + name] = worst, worst_du
            cfg["dense_" + name] = rows
        cfg["condensed_vs_dense_worst_rel"] = max(max(cfg["worst_rel_" + n], cfg["worst_rel_du_" + n]) for n in COTANGENTS)
        out["configs"][fr.config_key(model, sp, mix)] = cfg
    return out


def dump_golden(data, path=GOLDEN_PATH):
    """One lane per line: a diff of the file shows which lane of which configuration moved."""
    lines = ["{", ' "about": %s,' % json.dumps(data["about"]), ' "configs": {']
    keys = list(data["configs"])
    arrays = ["dense_" + n for n in COTANGENTS]
    for key in keys:
        cfg = data["configs"][key]
        lines.append("  %s: {" % json.dumps(key))
        for name in ["seed", "sample_lanes"] + ["worst_rel_" + n for n in COTANGENTS] + [
                "worst_rel_du_" + n for n in COTANGENTS] + ["condensed_vs_dense_worst_rel"]:
            lines.append("   %s: %s," % (json.dumps(name), json.dumps(cfg[name])))
        for name in arrays:
            lines.append("   %s: [" % json.dumps(name))
            lines += ["    %s%s" % (json.dumps(row, separators=(",", ":")), "," if i + 1 < len(cfg[name]) else "")
                      for i, row in enumerate(cfg[name])]
            lines.append("   ]%s" % ("," if name != arrays[-1] else ""))
        lines.append("  }%s" % ("," if key != keys[-1] else ""))
    lines += [" }", "}"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def load_golden():
    with open(GOLDEN_PATH) as fh:
        return json.load(fh)
