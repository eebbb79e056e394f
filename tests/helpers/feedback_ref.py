"""Numpy references for the feedback gains K = du / dx0 of the MPC plan (include/cpmpc.h: cpmpc_feedback_gain_batch), built
on the CPU oracle's problem functions.  TEST INFRASTRUCTURE ONLY.

  feedback_gain_ref      dense: the KKT system [[J^T J, A^T], [A, 0]] of the undamped QP at z with unit right-hand sides in
                         the initial-state rows NX (S - 1) + j (layout: tests/test_oracle_problem.py)
  feedback_gain_qp_diff  differences of two orc.qp_solve calls, the initial-state row of c lowered by one
  condensed_gain         the closed form  K = - U^-T D^-1 W (S + Dg)^-1 Psi_0  from the blocks of A, in the recurrences the
                         kernel uses ("Feedback gains"), with the precision of each part selectable
  sample / golden        the seeded test sample and the file tests/golden/feedback_gain_sample.json made from it
"""
import ctypes as C
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "feedback_gain_sample.json")

DYN = {"single": [1.0, 0.1, 0.25, 9.81, 0.05, 0.1, 0.02, 0.8, 100.0],   # viz/src/application.ts:61-71 (conftest.DYN_UI)
       "double": [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]}                       # tests/test_gpu_double.py
# terminal rows in state order (>= 0: cost row with that weight, < 0: equality row); None = the default parameters'
TERMINAL_MIXES = {"default": None,
                  "mix": {"single": [40.0, -1.0, 3.0, -1.0], "double": [40.0, -1.0, -1.0, 3.0, 0.5, 0.5]}}
SPACINGS = (5, 10, 20)
SAMPLE_LANES = 64     # lanes of the CPU sample per configuration (the recorded figure is their worst)
GOLDEN_LANES = 16     # lanes whose inputs and K[0..1] are stored
GOLDEN_Z_LANES = 2    # of those, the lanes whose solution z is stored as well: every z is regenerated from the seed and the
                      # stored ones pin the generator; with all sixteen the file is 235 KB (309 KB at full precision)
_dp = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def params_for(orc, model, sp, terminal_weights=None, **over):
    """Default OptimizationParams at state_spacing sp, the four terminal weights replaced by terminal_weights (state order;
    the 6-state model's two poles share th_final / th_dot_final, as in the oracle and the kernels' shared parameters)."""
    p = orc.default_opt_params(state_spacing=sp, **over)
    if terminal_weights is not None:
        w = [float(v) for v in terminal_weights]
        nq = len(w) // 2
        assert all(v == w[1] for v in w[1:nq]) and all(v == w[nq + 1] for v in w[nq + 1:]), "poles share their weights"
        p.b_x_final_cost_weight, p.th_final_cost_weight = w[0], w[1]
        p.b_x_dot_final_cost_weight, p.th_dot_final_cost_weight = w[nq], w[nq + 1]
    return p


def problem_eval(orc, model, p, dyn, x_current, set_point, u_prev, z):
    """orc_problem_eval_model: (r, c, J, A) for either model."""
    L = orc.lib()
    m = orc.MODELS[model]
    L.orc_problem_eval_model.argtypes = [C.c_int, C.POINTER(orc.OptParams), _dp, _dp, C.c_double, C.c_double, _dp, _dp,
                                         _dp, _dp, _dp]
    L.orc_problem_eval_model.restype = None
    dim, n_eq, n_cost = orc.problem_shape_model(model, p)
    dyn = np.ascontiguousarray(dyn, dtype=np.float64)
    x_current = np.ascontiguousarray(x_current, dtype=np.float64)
    z = np.ascontiguousarray(z, dtype=np.float64)
    assert z.size == dim and x_current.size == orc.model_nx(m) and dyn.size == orc.model_np(m)
    r, c = np.zeros(max(n_cost, 1)), np.zeros(n_eq)
    J, A = np.zeros((max(n_cost, 1), dim)), np.zeros((n_eq, dim))
    L.orc_problem_eval_model(m, C.byref(p), _ptr(dyn), _ptr(x_current), float(set_point), float(u_prev), _ptr(z), _ptr(r),
                             _ptr(c), _ptr(J), _ptr(A))
    return r[:n_cost], c, J[:n_cost], A


def _shape(orc, model, p):
    nx = orc.model_nx(orc.MODELS[model])
    N, sp = int(p.window_length), int(p.state_spacing)
    return nx, N, sp, N // sp + 1


def feedback_gain_ref(orc, p, dyn, z, terminal_weights=None, model="single", want_cond=False):
    """Dense reference K [N, NX]: column j is the u-part of the KKT solve with a unit right-hand side in initial-state row j."""
    nx, N, sp, S = _shape(orc, model, p)
    if terminal_weights is not None:
        p = params_for(orc, model, sp, terminal_weights)
    z = np.asarray(z, dtype=np.float64)
    _, _, J, A = problem_eval(orc, model, p, dyn, z[:nx], 0.0, 0.0, z)
    dim, n_eq = A.shape[1], A.shape[0]
    kkt = np.zeros((dim + n_eq, dim + n_eq))
    kkt[:dim, :dim] = J.T @ J
    kkt[:dim, dim:] = A.T
    kkt[dim:, :dim] = A
    rhs = np.zeros((dim + n_eq, nx))
    for j in range(nx):
        rhs[dim + nx * (S - 1) + j, j] = 1.0   # c_init = z_0 - x0: d(-c)/d x0_j = +e_j
    K = np.linalg.solve(kkt, rhs)[nx * S:dim]
    return (K, float(np.linalg.cond(kkt))) if want_cond else K


def feedback_gain_qp_diff(orc, p, dyn, z, model="single"):
    """K [N, NX] from differences of orc.qp_solve: initial-state row NX (S - 1) + j of c lowered by one.  Returns (K, the
    return codes of every qp_solve, max |dz| of the base solve)."""
    nx, N, sp, S = _shape(orc, model, p)
    z = np.asarray(z, dtype=np.float64)
    r, c, J, A = problem_eval(orc, model, p, dyn, z[:nx], 0.0, 0.0, z)
    rc0, dz0 = orc.qp_solve(J, r, A, c, N, 0.0)
    codes = [rc0]
    K = np.zeros((N, nx))
    for j in range(nx):
        c1 = c.copy()
        c1[nx * (S - 1) + j] -= 1.0
        rc, dz = orc.qp_solve(J, r, A, c1, N, 0.0)
        codes.append(rc)
        K[:, j] = (dz - dz0)[nx * S:]
    return K, codes, float(np.abs(dz0).max())


def blocks_of(orc, p, dyn, z, model="single", precision="f64"):
    """(Phi [S-1, NX, NX], Gam [N, NX]) read from the shooting rows of the oracle's A at z.  precision="f32": of the
    single-precision oracle's A (orc.problem_eval_f32: the linearisation itself computed in float, not the double blocks
    rounded)."""
    nx, N, sp, S = _shape(orc, model, p)
    z = np.asarray(z, dtype=np.float64)
    assert precision in ("f64", "f32"), precision
    if precision == "f32":
        _, _, _, A = orc.problem_eval_f32(model, p, dyn, z[:nx], 0.0, 0.0, z)
    else:
        _, _, _, A = problem_eval(orc, model, p, dyn, z[:nx], 0.0, 0.0, z)
    Phi = np.stack([A[nx * s:nx * s + nx, nx * s:nx * s + nx] for s in range(S - 1)])
    Gam = np.stack([A[nx * (k // sp):nx * (k // sp) + nx, nx * S + k] for k in range(N)])
    return Phi, Gam


def terminal_rows(orc, p, model="single", terminal_weights=None):
    """(Rw, Dg) of load_terminal: residual weight (1 on an equality row), 1 / 0 for cost / equality rows."""
    nx = orc.model_nx(orc.MODELS[model])
    nq = nx // 2
    if terminal_weights is None:
        terminal_weights = ([p.b_x_final_cost_weight] + [p.th_final_cost_weight] * (nq - 1)
                            + [p.b_x_dot_final_cost_weight] + [p.th_dot_final_cost_weight] * (nq - 1))
    w = np.asarray(terminal_weights, dtype=np.float64)
    return np.where(w >= 0, w, 1.0), (w >= 0).astype(np.float64)


def condensed_gain(Phi, Gam, Rw, Dg, wu, wd, sp, lin=np.float64, n_rows=None):
    """K = - U^-T D^-1 W (S + Dg)^-1 Psi_0 in the kernel's recurrences.  `lin`: the type Phi, Gamma, Psi, w_k, upsilon and
    1 / d are carried in (float32: the float kernels' precision split -- S, its LDL^T, the NX solves and the ascending pass
    stay in double)."""
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
    # LDL^T without pivoting, as the kernel
    L, d = np.eye(nx), np.zeros(nx)
    for j in range(nx):
        d[j] = Sm[j, j] - np.sum(L[j, :j] ** 2 * d[:j])
        assert d[j] > 0
        for i in range(j + 1, nx):
            L[i, j] = (Sm[i, j] - np.sum(L[i, :j] * L[j, :j] * d[:j])) / d[j]
    Y = np.linalg.solve(L, Psi.astype(np.float64))
    Q = np.linalg.solve(L.T, Y / d[:, None])
    K = np.zeros((n_rows, nx))
    prev, ups_prev = np.zeros(nx), 0.0
    for k in range(n_rows):
        K[k] = -(Wm[k].astype(np.float64) @ Q) * np.float64(inv_d[k]) - ups_prev * prev
        prev, ups_prev = K[k], np.float64(ups[k])
    return K


def condensed_gain_ref(orc, p, dyn, z, terminal_weights=None, model="single", lin=np.float64):
    nx, N, sp, S = _shape(orc, model, p)
    Phi, Gam = blocks_of(orc, p, dyn, z, model)
    Rw, Dg = terminal_rows(orc, p, model, terminal_weights)
    return condensed_gain(Phi, Gam, Rw, Dg, max(p.u_cost_weight, 0.0), max(p.u_derivative_cost_weight, 0.0), sp, lin=lin)


def rel_err(K, K_ref):
    """max |K - K_ref| / max |K_ref| of one problem."""
    return float(np.abs(K - K_ref).max() / np.abs(K_ref).max())


# ---- the sample --------------------------------------------------------------------------------------------------
def sample_states(model, seed, lanes):
    """b_x and the velocities uniform +-0.5, pole angles within 0.3 rad of upright: [NX, lanes]."""
    rng = np.random.default_rng(seed)
    nq = 2 if model == "single" else 3
    rows = [rng.uniform(-0.5, 0.5, lanes)]
    rows += [np.pi / 2 + rng.uniform(-0.3, 0.3, lanes) for _ in range(nq - 1)]
    rows += [rng.uniform(-0.5, 0.5, lanes) for _ in range(nq)]
    return np.stack(rows)


def config_seed(model, sp, mix):
    return 20260000 + 1000 * (model == "double") + 10 * sp + (mix == "mix")


def config_key(model, sp, mix):
    return "%s/sp%d/%s" % (model, sp, mix)


def configs():
    return [(m, sp, mix) for m in ("single", "double") for sp in SPACINGS for mix in TERMINAL_MIXES]


def solve_sample(orc, model, sp, mix, lanes, window_length=None, u_cost_weight=None, u_derivative_cost_weight=None,
                 terminal_weights=None, seed=None):
    """The sample of one configuration: states x0 [NX, lanes] and the oracle's solutions z [dim, lanes] (Optimization.step
    from a cold start, default parameters at this spacing and these terminal rows).  window_length, the two control-cost
    weights, an explicit list of terminal rows (state order, instead of the mix) and the seed of the states may be given;
    left out, they are the default parameters', the mix's and config_seed's."""
    if terminal_weights is None:
        tw = TERMINAL_MIXES[mix]
        tw = None if tw is None else tw[model]
    else:
        tw = [float(v) for v in terminal_weights]
    over = {k: v for k, v in (("window_length", window_length), ("u_cost_weight", u_cost_weight),
                              ("u_derivative_cost_weight", u_derivative_cost_weight)) if v is not None}
    p = params_for(orc, model, sp, tw, **over)
    x0 = sample_states(model, config_seed(model, sp, mix) if seed is None else seed, lanes)
    z = np.stack([orc.Optimization(p, model=model).step(x0[:, b], DYN[model], 0.0).z for b in range(lanes)], axis=1)
    return p, tw, x0, z


def _rounded(a, digits):
    return [float("%.*g" % (digits, v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def make_golden(orc):
    out = {"about": "feedback gains K = du/dx0 of the plan: per configuration the seed, the inputs x0 [lane][NX] and the dense "
                    "reference's rows K[0..1] [lane][2 NX] of %d lanes (12 / 9 digits), the oracle's solution z [lane][dim] of "
                    "the first %d of them, and the worst relative difference between the condensed closed form and the dense "
                    "KKT solve over the %d-lane sample (tests/helpers/feedback_ref.py)"
                    % (GOLDEN_LANES, GOLDEN_Z_LANES, SAMPLE_LANES),
           "configs": {}}
    for model, sp, mix in configs():
        p, tw, x0, z = solve_sample(orc, model, sp, mix, SAMPLE_LANES)
        worst, K01 = 0.0, []
        for b in range(SAMPLE_LANES):
            Kd = feedback_gain_ref(orc, p, DYN[model], z[:, b], model=model)
            Kc = condensed_gain_ref(orc, p, DYN[model], z[:, b], model=model)
            worst = max(worst, rel_err(Kc, Kd))
            if b < GOLDEN_LANES:
                K01.append(_rounded(Kd[:2], 9))
        out["configs"][config_key(model, sp, mix)] = {
            "seed": config_seed(model, sp, mix), "dyn": DYN[model], "terminal_weights": tw, "sample_lanes": SAMPLE_LANES,
            "condensed_vs_dense_worst_rel": worst,
            "x0": [_rounded(x0[:, b], 12) for b in range(GOLDEN_LANES)],
            "z": [_rounded(z[:, b], 12) for b in range(GOLDEN_Z_LANES)], "K01": K01}
    return out


def dump_golden(data, path=GOLDEN_PATH):
    """One array (a lane's x0, z or K[0..1]) per line: a diff of the file shows which lane of which configuration moved."""
    lines = ["{", ' "about": %s,' % json.dumps(data["about"]), ' "configs": {']
    keys = list(data["configs"])
    for key in keys:
        cfg = data["configs"][key]
        lines.append("  %s: {" % json.dumps(key))
        for name in ("seed", "dyn", "terminal_weights", "sample_lanes", "condensed_vs_dense_worst_rel"):
            lines.append("   %s: %s," % (json.dumps(name), json.dumps(cfg[name])))
        for name in ("x0", "z", "K01"):
            lines.append("   %s: [" % json.dumps(name))
            lines += ["    %s%s" % (json.dumps(row, separators=(",", ":")), "," if i + 1 < len(cfg[name]) else "")
                      for i, row in enumerate(cfg[name])]
            lines.append("   ]%s" % ("," if name != "K01" else ""))
        lines.append("  }%s" % ("," if key != keys[-1] else ""))
    lines += [" }", "}"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def load_golden():
    with open(GOLDEN_PATH) as fh:
        return json.load(fh)
