"""Numpy references for the sensitivities of the MPC plan to the set-point and to u_prev, k_sp = du / dset_point and
k_up = du / du_prev (include/cpmpc.h: cpmpc_plan_sensitivity_batch), built on tests/helpers/feedback_ref.py and the CPU
oracle's problem functions.  TEST INFRASTRUCTURE ONLY.

  sensitivity_ref         dense: the KKT system [[J^T J, A^T], [A, 0]] of the undamped QP at z, right-hand sides
                          -(J^T dr, dc) with (dr, dc) the difference of the oracle's residuals (r, c) at set-point 1 / 0 and
                          at u_prev 1 / 0 -- both enter linearly, so the difference is the exact derivative
  sensitivity_qp_diff     differences of two orc.qp_solve calls, at set-point 0 / 1 and at u_prev 0 / 1
  condensed_sensitivities the closed forms (and K) in the kernel's recurrences, the precision of each part selectable
  golden                  tests/golden/plan_sensitivity_sample.json: per configuration of feedback_ref.configs() -- the seeds,
                          and therefore the x0 and z, of feedback_gain_sample.json -- the worst condensed-vs-dense difference
                          and rows 0..1 of both sensitivities on 16 lanes
"""
import json
import os

import numpy as np

from helpers import feedback_ref as fr

GOLDEN_PATH = os.path.join(fr.ROOT, "tests", "golden", "plan_sensitivity_sample.json")


def _kkt(J, A):
    dim, n_eq = A.shape[1], A.shape[0]
    kkt = np.zeros((dim + n_eq, dim + n_eq))
    kkt[:dim, :dim] = J.T @ J
    kkt[:dim, dim:] = A.T
    kkt[dim:, :dim] = A
    return kkt


def sensitivity_ref(orc, p, dyn, z, terminal_weights=None, model="single", want_cond=False):
    """Dense reference (k_sp [N], k_up [N]): min |r + J dz|^2 s.t. c + A dz = 0, so d(dz) = KKT^-1 (-J^T dr, -dc)."""
    nx, N, sp, S = fr._shape(orc, model, p)
    if terminal_weights is not None:
        p = fr.params_for(orc, model, sp, terminal_weights)
    z = np.asarray(z, dtype=np.float64)
    r0, c0, J, A = fr.problem_eval(orc, model, p, dyn, z[:nx], 0.0, 0.0, z)
    r1, c1, J1, A1 = fr.problem_eval(orc, model, p, dyn, z[:nx], 1.0, 0.0, z)
    r2, c2, J2, A2 = fr.problem_eval(orc, model, p, dyn, z[:nx], 0.0, 1.0, z)
    assert np.array_equal(J, J1) and np.array_equal(J, J2) and np.array_equal(A, A1) and np.array_equal(A, A2)
    dim = A.shape[1]
    kkt = _kkt(J, A)
    rhs = np.stack([np.concatenate([-J.T @ (r1 - r0), -(c1 - c0)]), np.concatenate([-J.T @ (r2 - r0), -(c2 - c0)])], axis=1)
    k = np.linalg.solve(kkt, rhs)[nx * S:dim]
    return (k[:, 0], k[:, 1], float(np.linalg.cond(kkt))) if want_cond else (k[:, 0], k[:, 1])


def sensitivity_qp_diff(orc, p, dyn, z, model="single"):
    """(k_sp, k_up, return codes, max |dz| of the base solve) from differences of orc.qp_solve."""
    nx, N, sp, S = fr._shape(orc, model, p)
    z = np.asarray(z, dtype=np.float64)
    r, c, J, A = fr.problem_eval(orc, model, p, dyn, z[:nx], 0.0, 0.0, z)
    rc0, dz0 = orc.qp_solve(J, r, A, c, N, 0.0)
    codes, out = [rc0], []
    for set_point, u_prev in ((1.0, 0.0), (0.0, 1.0)):
        r1, c1, _, _ = fr.problem_eval(orc, model, p, dyn, z[:nx], set_point, u_prev, z)
        rc, dz = orc.qp_solve(J, r1, A, c1, N, 0.0)
        codes.append(rc)
        out.append((dz - dz0)[nx * S:])
    return out[0], out[1], codes, float(np.abs(dz0).max())


def condensed_sensitivities(Phi, Gam, Rw, Dg, wu, wd, sp, lin=np.float64, n_rows=None):
    """(K [n_rows, NX], k_sp [n_rows], k_up [n_rows]) in the kernel's recurrences (csrc/plan_sensitivity_kernels.hpp):
        K = - op((S + Dg)^-1 Psi_0),  k_sp = + op((S + Dg)^-1 Rw[0] e_0),  k_up = U^-T D^-1 (wd^2 e_0 - W dq),
        dq = (wd^2 / d_0) (S + Dg)^-1 w_0,  op(v)_k = (w_k . v) / d_k - upsilon_{k-1} op(v)_{k-1}.
    `lin`: the type Phi, Gamma, Psi, w_k, upsilon and 1 / d are carried in (float32: the float kernels' precision split -- S,
    its LDL^T, the solves and the ascending pass stay in double), as feedback_ref.condensed_gain."""
    N, nx = Gam.shape
    S1 = Phi.shape[0]
    n_rows = N if n_rows is None else n_rows
    Phi, Gam = Phi.astype(lin), Gam.astype(lin)
    wu2, wd2 = lin(wu) * lin(wu), lin(wd) * lin(wd)
    Psi = np.diag(Rw.astype(lin))
    Wm = np.zeros((N, nx), dtype=lin)
    ups, inv_d = np.zeros(N, dtype=lin), np.zeros(N, dtype=lin)
    Sm = np.zeros((nx, nx))
    wprev, d_next = np.zeros(nx, dtype=lin), lin(1)
    for s in range(S1 - 1, -1, -1):
        for k in range(sp * (s + 1) - 1, sp * s - 1, -1):
            nd = lin(2) if k < N - 1 else lin(1)
            ups[k] = -wd2 / d_next if k < N - 1 else lin(0)
            dk = (wu2 + wd2 * nd) + wd2 * ups[k]
            assert dk > 0
            inv_d[k] = lin(1) / dk
            d_next = dk
            Wm[k] = Psi @ Gam[k] - ups[k] * wprev
            w64 = Wm[k].astype(np.float64)
            Sm += np.outer(w64 * np.float64(inv_d[k]), w64)
            wprev = Wm[k]
        Psi = (Psi @ Phi[s]).astype(lin)
    Sm = Sm + np.diag(Dg)
    L, d = np.eye(nx), np.zeros(nx)   # LDL^T without pivoting, as the kernel
    for j in range(nx):
        d[j] = Sm[j, j] - np.sum(L[j, :j] ** 2 * d[:j])
        assert d[j] > 0
        for i in range(j + 1, nx):
            L[i, j] = (Sm[i, j] - np.sum(L[i, :j] * L[j, :j] * d[:j])) / d[j]

    def solve(b):
        return np.linalg.solve(L.T, np.linalg.solve(L, b) / (d[:, None] if b.ndim == 2 else d))
    W64, id64, ups64 = Wm.astype(np.float64), inv_d.astype(np.float64), ups.astype(np.float64)
    Q = solve(Psi.astype(np.float64))
    e0 = np.zeros(nx)
    e0[0] = np.float64(Rw.astype(lin)[0])
    q_sp = solve(e0)
    dq = solve(np.float64(wd2) * id64[0] * W64[0])
    y = np.zeros((N, nx + 2))   # the right-hand sides of U^T x = D^-1 y, column by column
    for k in range(N):   # row by row: the gain columns are feedback_ref.condensed_gain's to the bit
        y[k, :nx] = -(W64[k] @ Q)
    y[:, nx] = W64 @ q_sp
    y[:, nx + 1] = -(W64 @ dq)
    y[0, nx + 1] += np.float64(wd2)
    out = np.zeros((n_rows, nx + 2))
    prev, ups_prev = np.zeros(nx + 2), 0.0
    for k in range(n_rows):
        out[k] = y[k] * id64[k] - ups_prev * prev
        prev, ups_prev = out[k], ups64[k]
    return out[:, :nx], out[:, nx], out[:, nx + 1]


def condensed_ref(orc, p, dyn, z, terminal_weights=None, model="single", lin=np.float64):
    """(K, k_sp, k_up) of the condensed closed forms from the blocks of the oracle's A at z."""
    nx, N, sp, S = fr._shape(orc, model, p)
    Phi, Gam = fr.blocks_of(orc, p, dyn, z, model)
    Rw, Dg = fr.terminal_rows(orc, p, model, terminal_weights)
    return condensed_sensitivities(Phi, Gam, Rw, Dg, max(p.u_cost_weight, 0.0), max(p.u_derivative_cost_weight, 0.0), sp,
                                   lin=lin)


def rel_err(k, k_ref):
    """max |k - k_ref| / max |k_ref| of one problem."""
    return float(np.abs(np.asarray(k) - k_ref).max() / np.abs(k_ref).max())


# ---- the golden file ---------------------------------------------------------------------------------------------
def make_golden(orc):
    out = {"about": "sensitivities of the plan, k_sp = du/dset_point and k_up = du/du_prev: per configuration (the seeds, and "
                    "so the x0 and z, of feedback_gain_sample.json) the worst relative difference between the condensed closed "
                    "forms and the dense KKT solve over the %d-lane sample, for each and for both, and the dense reference's "
                    "rows k_sp[0..1], k_up[0..1] of %d lanes as [lane][4] (9 digits) (tests/helpers/plan_sensitivity_ref.py)"
                    % (fr.SAMPLE_LANES, fr.GOLDEN_LANES),
           "configs": {}}
    for model, sp, mix in fr.configs():
        p, tw, x0, z = fr.solve_sample(orc, model, sp, mix, fr.SAMPLE_LANES)
        w_sp, w_up, rows = 0.0, 0.0, []
        for b in range(fr.SAMPLE_LANES):
            sd, ud = sensitivity_ref(orc, p, fr.DYN[model], z[:, b], model=model)
            _, sc, uc = condensed_ref(orc, p, fr.DYN[model], z[:, b], model=model)
            w_sp, w_up = max(w_sp, rel_err(sc, sd)), max(w_up, rel_err(uc, ud))
            if b < fr.GOLDEN_LANES:
                rows.append(fr._rounded(np.concatenate([sd[:2], ud[:2]]), 9))
        out["configs"][fr.config_key(model, sp, mix)] = {
            "seed": fr.config_seed(model, sp, mix), "sample_lanes": fr.SAMPLE_LANES, "k_sp_worst_rel": w_sp,
            "k_up_worst_rel": w_up, "condensed_vs_dense_worst_rel": max(w_sp, w_up), "k01": rows}
    return out


def dump_golden(data, path=GOLDEN_PATH):
    """One lane per line: a diff of the file shows which lane of which configuration moved."""
    lines = ["{", ' "about": %s,' % json.dumps(data["about"]), ' "configs": {']
    keys = list(data["configs"])
    for key in keys:
        cfg = data["configs"][key]
        lines.append("  %s: {" % json.dumps(key))
        for name in ("seed", "sample_lanes", "k_sp_worst_rel", "k_up_worst_rel", "condensed_vs_dense_worst_rel"):
            lines.append("   %s: %s," % (json.dumps(name), json.dumps(cfg[name])))
        lines.append('   "k01": [')
        lines += ["    %s%s" % (json.dumps(row, separators=(",", ":")), "," if i + 1 < len(cfg["k01"]) else "")
                  for i, row in enumerate(cfg["k01"])]
        lines.append("   ]")
        lines.append("  }%s" % ("," if key != keys[-1] else ""))
    lines += [" }", "}"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def load_golden():
    with open(GOLDEN_PATH) as fh:
        return json.load(fh)
