"""The four plan-derivative calls (feedback gains, plan sensitivities, their reverse mode, the weight gradients) off the
default shape: horizons other than N = 40, spacings the linearisation has no specialisation for, single-interval and
one-control-per-interval walks, and control-cost weights other than 0.1 / 0.1 -- the cases, their seeded samples and, per
(case, call), the REFERENCE FIGURE that the GPU tests' bounds are made of.  TEST INFRASTRUCTURE ONLY.

Why the cases carry soft terminal rows (every row a cost row): with the default rows (one cost row, the others
equalities) the dense KKT reference itself runs out of digits off 40/10 -- the condensed form and the dense solve differ by
1e-9 ... 4e-3 in the 6-state model -- and a bound made of such a figure tests nothing.  With soft rows the two agree to
1e-15 ... 4e-13 and a relative perturbation of 1e-12 of Phi and Gamma moves the outputs by 1e-12 ... 1e-10: that is where a
subtly wrong kernel shows.  Default rows are kept where the reference still carries digits (grid C).

  cases()            grids A (soft rows, default weights, every shape), B (soft rows, the other weight sets) and C (default rows)
  sample             x0, the oracle's cold-start z and the inputs of the calls on LANES lanes, seeded per case
  dense / condensed  one call's dense reference / numpy condensed form on one lane, as dicts of named outputs
  errors             a call's outputs against a reference in that call's own rel_err, per named part
  reference_figures  per call the larger of (a) condensed vs dense and (b) the condensed form's change under a relative
                     perturbation of 1e-12 of every entry of Phi and Gamma, each the worst over the lanes
  float_emulation    per call and part the median / 99th percentile of the float emulation's error (lin = float32, Phi and
                     Gamma from the single-precision oracle) against the fp64 dense reference at z rounded to float
  golden             tests/golden/plan_derivative_shapes.json (tests/golden/gen_plan_derivative_shapes.py makes it)
"""
import collections
import json
import os

import numpy as np

from helpers import feedback_ref as fr
from helpers import plan_sensitivity_ref as ps
from helpers import plan_vjp_ref as pv
from helpers import plan_weight_vjp_ref as pw

GOLDEN_PATH = os.path.join(fr.ROOT, "tests", "golden", "plan_derivative_shapes.json")
LANES = 70            # one full wave and a ragged second
PERTURBATION = 1e-12  # three digits above double rounding: another sincos, another summation order in the linearisation
CAP = {"soft": 1e-9, "default": 1e-7}   # a reference figure above its cap admits no bound worth having
CALLS = ("gain", "sensitivity", "vjp", "weight_vjp")
PARTS = {"gain": ("K",), "sensitivity": ("k_sp", "k_up"), "vjp": ("g",), "weight_vjp": ("g", "g_tw_angle", "du")}

# terminal rows in state order; all >= 0: every row is a cost row.  The poles share their weights (fr.params_for)
SOFT = {"single": [40.0, 3.0, 3.0, 0.5], "double": [40.0, 3.0, 3.0, 3.0, 0.5, 0.5]}
WEIGHTS = collections.OrderedDict([("D", (0.1, 0.1)), ("wd0", (0.1, 0.0)), ("wu0", (0.0, 0.1)), ("wu3", (3.0, 1e-3)),
                                   ("wd1", (1e-3, 1.0))])   # (u_cost_weight, u_derivative_cost_weight)
OTHER_WEIGHTS = tuple(w for w in WEIGHTS if w != "D")
SHAPES = ((6, 1), (8, 8), (12, 4), (16, 1), (21, 7), (30, 3), (64, 4), (80, 5), (100, 10))   # (N, state_spacing)

Case = collections.namedtuple("Case", "model N sp rows weights")


def case_key(c):
    return "%s/%dx%d/%s/%s" % (c.model, c.N, c.sp, c.rows, c.weights)


def case_seed(c):
    return (30000000 + 5000000 * (c.model == "double") + 10000 * c.N + 100 * c.sp + 10 * list(WEIGHTS).index(c.weights)
            + (c.rows == "default"))


def grid_a():
    """Soft rows, the default weights, both models, every shape -- but double 100/10, whose reference is at 5e-8."""
    return [Case(m, N, sp, "soft", "D") for m in ("single", "double") for N, sp in SHAPES
            if not (m == "double" and (N, sp) == (100, 10))]


def grid_b():
    """Soft rows, the four other weight sets, both models, 12/4 and 40/10."""
    return [Case(m, N, sp, "soft", w) for m in ("single", "double") for N, sp in ((12, 4), (40, 10)) for w in OTHER_WEIGHTS]


def grid_c():
    """Default rows, where the dense reference still carries digits."""
    out = [Case("single", N, sp, "default", "D") for N, sp in ((8, 8), (21, 7), (30, 3), (100, 10))]
    out += [Case("single", 80, 5, "default", w) for w in WEIGHTS]
    out += [Case("single", 40, 10, "default", w) for w in OTHER_WEIGHTS]
    out += [Case("double", 40, 10, "default", "wd0")]
    return out


def cases():
    return grid_a() + grid_b() + grid_c()


def n_rows_of(c):
    """The row counts at which a cut can go wrong: 1, one interval, one control into the second, all but one, all."""
    out = []
    for n in (1, c.sp, c.sp + 1, c.N - 1, c.N):
        if 1 <= n <= c.N and n not in out:
            out.append(n)
    return out


# ---- the sample ------------------------------------------------------------------------------------------------------
Sample = collections.namedtuple("Sample", "p tw x0 z")
Inputs = collections.namedtuple("Inputs", "x0 set_point u_prev gbar")
_samples = {}


def oracle_params(orc, c):
    wu, wd = WEIGHTS[c.weights]
    tw = SOFT[c.model] if c.rows == "soft" else None
    return fr.params_for(orc, c.model, c.sp, tw, window_length=c.N, u_cost_weight=wu, u_derivative_cost_weight=wd), tw


def handle_params(pkg, orc, c, weights=None):
    """The handle's parameters of a case: the oracle's, field by field.  weights: (u_cost_weight, u_derivative_cost_weight)
    instead of the case's."""
    po, _ = oracle_params(orc, c)
    wu, wd = (po.u_cost_weight, po.u_derivative_cost_weight) if weights is None else weights
    return pkg.default_params(window_length=c.N, state_spacing=c.sp, u_cost_weight=wu, u_derivative_cost_weight=wd,
                              b_x_final_cost_weight=po.b_x_final_cost_weight, th_final_cost_weight=po.th_final_cost_weight,
                              b_x_dot_final_cost_weight=po.b_x_dot_final_cost_weight,
                              th_dot_final_cost_weight=po.th_dot_final_cost_weight)


def sample(orc, c, lanes=LANES):
    """Sample(p, tw, x0 [NX, lanes], z [dim, lanes]): fr.solve_sample at the case's shape, weights, rows and seed; computed
    once per process and shared (read-only)."""
    key = (c, lanes)
    if key not in _samples:
        wu, wd = WEIGHTS[c.weights]
        p, tw, x0, z = fr.solve_sample(orc, c.model, c.sp, "default", lanes, window_length=c.N, u_cost_weight=wu,
                                       u_derivative_cost_weight=wd,
                                       terminal_weights=SOFT[c.model] if c.rows == "soft" else None, seed=case_seed(c))
        for a in (x0, z):
            a.setflags(write=False)
        _samples[key] = Sample(p, tw, x0, z)
    return _samples[key]


def inputs(c, x0_sample, dtype=np.float64):
    """The inputs of the calls beside z, as float64 arrays holding values of `dtype` (what a kernel of that type reads): the
    weight gradients' x0 = the sample states + 0.01, set-point 0.3, u_prev 0.7 (plan_weight_vjp_ref's sample), and one
    cotangent per lane, uniform in [-1, 1]^N from the case's seed + 1."""
    lanes = x0_sample.shape[1]
    gbar = np.random.default_rng(case_seed(c) + 1).uniform(-1.0, 1.0, (lanes, c.N)).T

    def rounded(a):
        return np.ascontiguousarray(np.asarray(a, dtype=dtype).astype(np.float64))
    return Inputs(rounded(pw.sample_inputs(x0_sample)), float(dtype(pw.SET_POINT)), float(dtype(pw.U_PREV)), rounded(gbar))


# ---- one call on one lane --------------------------------------------------------------------------------------------
def dense(orc, c, p, call, z, inp, b):
    """The call's dense KKT reference on lane b at z [dim]: a dict of its named outputs (weight_vjp: with `scale`)."""
    dyn = fr.DYN[c.model]
    if call == "gain":
        return {"K": fr.feedback_gain_ref(orc, p, dyn, z, model=c.model)}
    if call == "sensitivity":
        sd, ud = ps.sensitivity_ref(orc, p, dyn, z, model=c.model)
        return {"k_sp": sd, "k_up": ud}
    if call == "vjp":
        return {"g": pv.dense_vjp(orc, p, dyn, z, inp.gbar[:, b], model=c.model)}
    g, du, scale = pw.dense_weight_vjp(orc, p, dyn, z, inp.x0[:, b], inp.gbar[:, b], set_point=inp.set_point,
                                       u_prev=inp.u_prev, model=c.model)
    return {"g": g, "du": du, "scale": scale}


def condensed(orc, c, p, call, z, inp, b, blocks, lin=np.float64):
    """The call's numpy condensed form on lane b from the blocks (Phi, Gam)."""
    Phi, Gam = blocks
    Rw, Dg = fr.terminal_rows(orc, p, c.model)
    wu, wd = max(p.u_cost_weight, 0.0), max(p.u_derivative_cost_weight, 0.0)
    if call == "gain":
        return {"K": fr.condensed_gain(Phi, Gam, Rw, Dg, wu, wd, c.sp, lin=lin)}
    if call == "sensitivity":
        _, sc, uc = ps.condensed_sensitivities(Phi, Gam, Rw, Dg, wu, wd, c.sp, lin=lin)
        return {"k_sp": sc, "k_up": uc}
    if call == "vjp":
        return {"g": pv.condensed_vjp(Phi, Gam, Rw, Dg, wu, wd, c.sp, inp.gbar[:, b], lin=lin)}
    g, du = pw.condensed_ref(orc, p, fr.DYN[c.model], z, inp.x0[:, b], inp.gbar[:, b], set_point=inp.set_point,
                             u_prev=inp.u_prev, model=c.model, lin=lin, blocks=blocks)
    return {"g": g, "du": du}


def _rel_or_exact(k, k_ref):
    """ps.rel_err; a reference that is identically zero (k_up without a derivative row) asks for exactly zero."""
    if not np.any(k_ref):
        assert not np.any(k), k
        return 0.0
    return ps.rel_err(k, k_ref)


def errors(call, got, ref, scale=None):
    """{part: error} of a call's outputs against a reference in the call's own measure.  weight_vjp: `scale` is the dense
    reference's (ref["scale"] unless given)."""
    if call == "gain":
        return {"K": fr.rel_err(got["K"], ref["K"])}
    if call == "sensitivity":
        return {n: _rel_or_exact(got[n], ref[n]) for n in ("k_sp", "k_up")}
    if call == "vjp":
        return {"g": pv.rel_err(got["g"], ref["g"])}
    scale = ref["scale"] if scale is None else scale
    return {"g": pw.rel_err(got["g"], ref["g"], scale), "g_tw_angle": _angle_rows_err(got["g"], ref["g"], scale),
            "du": pw.rel_err_du(got["du"], ref["du"])}


def _angle_rows_err(g, g_ref, scale):
    """pw.rel_err over g_tw of the pole-angle rows alone (states 1 .. NQ - 1; 0 where none of them is a cost row).  g_tw of a
    row is proportional to that row's terminal residual, so these outputs alone show an error in the angle residuals that
    the maximum over all NX + 2 outputs hides behind the worst-conditioned one."""
    nq = (len(g_ref) - 2) // 2
    rows = [t for t in range(1, nq) if scale[t] > 0]
    return max([abs(float(g[t]) - g_ref[t]) / scale[t] for t in rows], default=0.0)


# ---- the figures -----------------------------------------------------------------------------------------------------
def reference_figures(orc, c, lanes=LANES):
    """{call: {"condensed_vs_dense", "perturbation", "figure"}}: each part the worst over the lanes, the figure the larger."""
    smp = sample(orc, c, lanes)
    inp = inputs(c, smp.x0)
    rng = np.random.default_rng(case_seed(c) + 2)
    out = {call: {"condensed_vs_dense": 0.0, "perturbation": 0.0} for call in CALLS}
    for b in range(lanes):
        z = smp.z[:, b]
        Phi, Gam = fr.blocks_of(orc, smp.p, fr.DYN[c.model], z, c.model)
        moved = (Phi * (1.0 + PERTURBATION * rng.choice([-1.0, 1.0], Phi.shape)),
                 Gam * (1.0 + PERTURBATION * rng.choice([-1.0, 1.0], Gam.shape)))
        for call in CALLS:
            ref = dense(orc, c, smp.p, call, z, inp, b)
            con = condensed(orc, c, smp.p, call, z, inp, b, (Phi, Gam))
            per = condensed(orc, c, smp.p, call, z, inp, b, moved)
            o = out[call]
            o["condensed_vs_dense"] = max(o["condensed_vs_dense"], max(errors(call, con, ref).values()))
            o["perturbation"] = max(o["perturbation"], max(errors(call, per, con, scale=ref.get("scale")).values()))
    for o in out.values():
        o["figure"] = max(o["condensed_vs_dense"], o["perturbation"])
    return out


def float_lane_errors(orc, c, call, z32, inp32, got=None):
    """({part: [lanes]} of the float emulation, the same of `got` or None): errors against the fp64 dense reference at z32 (z
    as a float kernel reads it).  got: a function lane -> the call's outputs."""
    p = oracle_params(orc, c)[0]
    emu, res = {n: [] for n in PARTS[call]}, {n: [] for n in PARTS[call]}
    for b in range(z32.shape[1]):
        z = z32[:, b]
        ref = dense(orc, c, p, call, z, inp32, b)
        blocks = fr.blocks_of(orc, p, fr.DYN[c.model], z, c.model, precision="f32")
        for n, e in errors(call, condensed(orc, c, p, call, z, inp32, b, blocks, lin=np.float32), ref).items():
            emu[n].append(e)
        if got is not None:
            for n, e in errors(call, got(b), ref).items():
                res[n].append(e)
    as_arrays = lambda d: {n: np.array(v) for n, v in d.items()}   # noqa: E731
    return as_arrays(emu), (as_arrays(res) if got is not None else None)


def float_sample(orc, c, lanes=LANES):
    """(z32, inputs32): the oracle's z and the calls' inputs rounded to float."""
    smp = sample(orc, c, lanes)
    return smp.z.astype(np.float32).astype(np.float64), inputs(c, smp.x0, np.float32)


def float_emulation(orc, c, lanes=LANES):
    """{call: {part: [median, 99th percentile]}} of the float emulation's per-lane error."""
    z32, inp32 = float_sample(orc, c, lanes)
    out = {}
    for call in CALLS:
        errs, _ = float_lane_errors(orc, c, call, z32, inp32)
        out[call] = {n: [float(np.percentile(e, 50)), float(np.percentile(e, 99))] for n, e in errs.items()}
    return out


# ---- the golden file -------------------------------------------------------------------------------------------------
def make_golden(orc, progress=None):
    data = {"about": "plan-derivative calls off the default shape (tests/helpers/plan_shapes.py): per case "
                     "model/NxSP/rows/weights and per call the reference figure on %d lanes -- the larger of the worst "
                     "difference between the numpy condensed form and the dense KKT solve and the worst change of the "
                     "condensed form under a relative perturbation of %g of every entry of Phi and Gamma -- and, for the "
                     "cases of grid A, the float emulation's [median, 99th percentile] per output.  'excluded': the (case, "
                     "call) pairs whose figure is above the cap (%g soft rows, %g default rows)"
                     % (LANES, PERTURBATION, CAP["soft"], CAP["default"]),
            "lanes": LANES, "cases": {}, "excluded": []}
    emulated = set(grid_a())
    for c in cases():
        figs = reference_figures(orc, c)
        emu = float_emulation(orc, c) if c in emulated else None
        entry = {"seed": case_seed(c), "calls": {}}
        for call in CALLS:
            entry["calls"][call] = dict(figs[call])
            if emu is not None:
                entry["calls"][call]["emulation"] = emu[call]
            if figs[call]["figure"] > CAP[c.rows]:
                data["excluded"].append({"case": case_key(c), "call": call, "figure": figs[call]["figure"]})
        data["cases"][case_key(c)] = entry
        if progress is not None:
            progress(c, entry)
    return data


def dump_golden(data, path=GOLDEN_PATH):
    """One call per line: a diff of the file shows which figure of which case moved."""
    lines = ["{", ' "about": %s,' % json.dumps(data["about"]), ' "lanes": %d,' % data["lanes"], ' "cases": {']
    keys = list(data["cases"])
    for key in keys:
        entry = data["cases"][key]
        lines.append('  %s: {"seed": %d, "calls": {' % (json.dumps(key), entry["seed"]))
        lines += ["   %s: %s%s" % (json.dumps(call), json.dumps(entry["calls"][call]), "," if call != CALLS[-1] else "")
                  for call in CALLS]
        lines.append("  }}%s" % ("," if key != keys[-1] else ""))
    lines.append(" },")
    lines.append(' "excluded": [')
    lines += ["  %s%s" % (json.dumps(e), "," if i + 1 < len(data["excluded"]) else "") for i, e in enumerate(data["excluded"])]
    lines += [" ]", "}"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def load_golden():
    with open(GOLDEN_PATH) as fh:
        return json.load(fh)


def excluded_pairs(golden):
    return {(e["case"], e["call"]) for e in golden["excluded"]}
