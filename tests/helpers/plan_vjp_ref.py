"""Numpy references for the reverse mode of the plan's sensitivities (include/cpmpc.h: cpmpc_plan_vjp_batch): a cotangent gbar
on the planned controls pulled back to x0, the set-point and u_prev,
    g_x0 = K^T gbar [NX],  g_sp = k_sp^T gbar,  g_up = k_up^T gbar,
built on tests/helpers/feedback_ref.py, tests/helpers/plan_sensitivity_ref.py and the CPU oracle's problem functions.  TEST
INFRASTRUCTURE ONLY.

  dense_vjp        ONE solve of the symmetric KKT system [[J^T J, A^T], [A, 0]] of the undamped QP at z with gbar in the
                   control rows; the solution dotted with the right-hand sides that feedback_ref.feedback_gain_ref (unit
                   vectors in the initial-state rows) and plan_sensitivity_ref.sensitivity_ref (-(J^T dr, dc) for the
                   set-point and for u_prev) solve for
  condensed_vjp    the closed forms in the kernel's recurrences (csrc/plan_vjp_kernels.hpp), the precision of the
                   linearisation selectable as in plan_sensitivity_ref.condensed_sensitivities
  cotangents       the two seeded cotangents of a configuration: uniform in [-1, 1]^N per lane from the configuration's
                   seed + 1, and e_0
  golden           tests/golden/plan_vjp_sample.json: per configuration of feedback_ref.configs() -- the seeds, and therefore
                   the x0 and z, of feedback_gain_sample.json -- the worst condensed-vs-dense difference over the 64-lane
                   sample and the dense outputs of 16 lanes
Outputs are packed as one vector [g_x0 (NX), g_sp, g_up] per problem."""
import json
import os

import numpy as np

from helpers import feedback_ref as fr
from helpers import plan_sensitivity_ref as ps

GOLDEN_PATH = os.path.join(fr.ROOT, "tests", "golden", "plan_vjp_sample.json")
COTANGENTS = ("uniform", "e0")
GOLDEN_GBAR_LANES = 2   # lanes whose uniform cotangent is stored: it is regenerated from the seed, these pin the generator


def _padded(gbar, N):
    g = np.zeros(N)
    g[:len(gbar)] = np.asarray(gbar, dtype=np.float64)
    return g


def dense_vjp(orc, p, dyn, z, gbar, terminal_weights=None, model="single"):
    """[g_x0, g_sp, g_up] (NX + 2) from one KKT solve; gbar holds the leading rows, the others are zero."""
    nx, N, sp, S = fr._shape(orc, model, p)
    if terminal_weights is not None:
        p = fr.params_for(orc, model, sp, terminal_weights)
    z = np.asarray(z, dtype=np.float64)
    r0, c0, J, A = fr.problem_eval(orc, model, p, dyn, z[:nx], 0.0, 0.0, z)
    r1, c1, _, _ = fr.problem_eval(orc, model, p, dyn, z[:nx], 1.0, 0.0, z)
    r2, c2, _, _ = fr.problem_eval(orc, model, p, dyn, z[:nx], 0.0, 1.0, z)
    dim, n_eq = A.shape[1], A.shape[0]
    kkt = ps._kkt(J, A)
    rhs = np.zeros(dim + n_eq)
    rhs[nx * S:dim] = _padded(gbar, N)
    y = np.linalg.solve(kkt, rhs)   # KKT is symmetric: y^T b = gbar^T (KKT^-1 b)[controls] for every right-hand side b
    out = np.zeros(nx + 2)
    out[:nx] = y[dim + nx * (S - 1):dim + nx * S]   # feedback_gain_ref's unit right-hand sides
    out[nx] = y @ np.concatenate([-J.T @ (r1 - r0), -(c1 - c0)])        # sensitivity_ref's, set-point
    out[nx + 1] = y @ np.concatenate([-J.T @ (r2 - r0), -(c2 - c0)])    # and u_prev
    return out


def condensed_vjp(Phi, Gam, Rw, Dg, wu, wd, sp, gbar, lin=np.float64):
    """[g_x0, g_sp, g_up] in the kernel's recurrences: next to sweep 1
        eta_k = gbar_k - upsilon_k eta_{k+1},  a += w_k eta_k / d_k,
    then q = (S + Dg)^-1 a,  g_x0 = - Psi_0^T q,  g_sp = Rw[0] q_0,  g_up = (wd^2 / d_0) (eta_0 - w_0 . q).
    `lin`: the type Phi, Gamma, Psi, w_k, upsilon and 1 / d are carried in (float32: the float kernels' precision split --
    S, eta, a, the LDL^T, the solve and the products stay in double), as condensed_sensitivities."""
    N, nx = Gam.shape
    S1 = Phi.shape[0]
    g = _padded(gbar, N)
    Phi, Gam = Phi.astype(lin), Gam.astype(lin)
    wu2, wd2 = lin(wu) * lin(wu), lin(wd) * lin(wd)
    Psi = np.diag(Rw.astype(lin))
    Sm = np.zeros((nx, nx))
    wk, d_next, inv_d = np.zeros(nx, dtype=lin), lin(1), lin(0)
    eta, av = 0.0, np.zeros(nx)
    for s in range(S1 - 1, -1, -1):
        for k in range(sp * (s + 1) - 1, sp * s - 1, -1):
            nd = lin(2) if k < N - 1 else lin(1)
            ups = -wd2 / d_next if k < N - 1 else lin(0)
            dk = (wu2 + wd2 * nd) + wd2 * ups
            assert dk > 0
            inv_d = lin(1) / dk
            d_next = dk
            wk = Psi @ Gam[k] - ups * wk
            w64 = wk.astype(np.float64)
            eta = g[k] - np.float64(ups) * eta
            av += w64 * (eta * np.float64(inv_d))
            Sm += np.outer(w64 * np.float64(inv_d), w64)
        Psi = (Psi @ Phi[s]).astype(lin)
    Sm = Sm + np.diag(Dg)
    L, d = np.eye(nx), np.zeros(nx)   # LDL^T without pivoting, as the kernel
    for j in range(nx):
        d[j] = Sm[j, j] - np.sum(L[j, :j] ** 2 * d[:j])
        assert d[j] > 0
        for i in range(j + 1, nx):
            L[i, j] = (Sm[i, j] - np.sum(L[i, :j] * L[j, :j] * d[:j])) / d[j]
    q = np.linalg.solve(L.T, np.linalg.solve(L, av) / d)
    out = np.zeros(nx + 2)
    out[:nx] = -(Psi.astype(np.float64).T @ q)
    out[nx] = np.float64(Rw.astype(lin)[0]) * q[0]
    out[nx + 1] = np.float64(wd2) * np.float64(inv_d) * (eta - wk.astype(np.float64) @ q)
    return out


def condensed_ref(orc, p, dyn, z, gbar, terminal_weights=None, model="single", lin=np.float64):
    """[g_x0, g_sp, g_up] of the condensed closed forms from the blocks of the oracle's A at z."""
    nx, N, sp, S = fr._shape(orc, model, p)
    Phi, Gam = fr.blocks_of(orc, p, dyn, z, model)
    Rw, Dg = fr.terminal_rows(orc, p, model, terminal_weights)
    return condensed_vjp(Phi, Gam, Rw, Dg, max(p.u_cost_weight, 0.0), max(p.u_derivative_cost_weight, 0.0), sp, gbar, lin=lin)


def rel_err(g, g_ref):
    """max |g - g_ref| / max |g_ref| of one problem over its NX + 2 outputs."""
    return float(np.abs(np.asarray(g) - g_ref).max() / np.abs(g_ref).max())


def cotangents(model, sp, mix, lanes, N=40):
    """{"uniform": [N, lanes] uniform in [-1, 1] from the configuration's seed + 1 (lane by lane: a lane's cotangent does not
    depend on how many lanes are drawn), "e0": [N, lanes] the first unit vector}."""
    rng = np.random.default_rng(fr.config_seed(model, sp, mix) + 1)
    e0 = np.zeros((N, lanes))
    e0[0] = 1.0
    return {"uniform": np.ascontiguousarray(rng.uniform(-1.0, 1.0, (lanes, N)).T), "e0": e0}


# ---- the golden file ---------------------------------------------------------------------------------------------
def make_golden(orc):
    out = {"about": "reverse mode of the plan's sensitivities, [g_x0 (NX), g_sp, g_up] = [K, k_sp, k_up]^T gbar: per "
                    "configuration (the seeds, and so the x0 and z, of feedback_gain_sample.json) and per cotangent -- "
                    "'uniform' in [-1, 1]^N from the seed + 1, stored for the first %d lanes as [lane][N], and 'e0' -- the "
                    "worst relative difference, max |.| / max |ref| per problem over the NX + 2 outputs, between the condensed "
                    "closed forms and the dense KKT solve over the %d-lane sample, and the dense outputs of %d lanes as "
                    "[lane][NX + 2] (12 digits) (tests/helpers/plan_vjp_ref.py)"
                    % (GOLDEN_GBAR_LANES, fr.SAMPLE_LANES, fr.GOLDEN_LANES),
           "configs": {}}
    for model, sp, mix in fr.configs():
        p, tw, x0, z = fr.solve_sample(orc, model, sp, mix, fr.SAMPLE_LANES)
        cots = cotangents(model, sp, mix, fr.SAMPLE_LANES, int(p.window_length))
        cfg = {"seed": fr.config_seed(model, sp, mix), "gbar_seed": fr.config_seed(model, sp, mix) + 1,
               "sample_lanes": fr.SAMPLE_LANES,
               "gbar_uniform": [[float(v) for v in cots["uniform"][:, b]] for b in range(GOLDEN_GBAR_LANES)]}
        for name in COTANGENTS:
            worst, rows = 0.0, []
            for b in range(fr.SAMPLE_LANES):
                gd = dense_vjp(orc, p, fr.DYN[model], z[:, b], cots[name][:, b], model=model)
                gc = condensed_ref(orc, p, fr.DYN[model], z[:, b], cots[name][:, b], model=model)
                worst = max(worst, rel_err(gc, gd))
                if b < fr.GOLDEN_LANES:
                    rows.append(fr._rounded(gd, 12))
            cfg["worst_rel_" + name] = worst
            cfg["dense_" + name] = rows
        cfg["condensed_vs_dense_worst_rel"] = max(cfg["worst_rel_" + n] for n in COTANGENTS)
        out["configs"][fr.config_key(model, sp, mix)] = cfg
    return out


def dump_golden(data, path=GOLDEN_PATH):
    """One lane per line: a diff of the file shows which lane of which configuration moved."""
    lines = ["{", ' "about": %s,' % json.dumps(data["about"]), ' "configs": {']
    keys = list(data["configs"])
    arrays = ["gbar_uniform"] + ["dense_" + n for n in COTANGENTS]
    for key in keys:
        cfg = data["configs"][key]
        lines.append("  %s: {" % json.dumps(key))
        for name in ["seed", "gbar_seed", "sample_lanes"] + ["worst_rel_" + n for n in COTANGENTS] + [
                "condensed_vs_dense_worst_rel"]:
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
