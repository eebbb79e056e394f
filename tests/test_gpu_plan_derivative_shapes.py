"""The four plan-derivative calls on the GPU (feedback_gain, plan_sensitivity, plan_vjp, plan_weight_vjp) off the default
shape: the cases of tests/helpers/plan_shapes.py -- horizons from 6 to 100 controls, single-interval and one-control
intervals, spacings served by the run-time-spacing linearisation, control-cost weights with either term absent -- every one
of 70 lanes (one full wave and a ragged second) against the dense KKT references of the call's own helper.

fp64: every lane and every output within 100 x the REFERENCE FIGURE of that (case, call) in
tests/golden/plan_derivative_shapes.json, at the oracle's z given explicitly and at the handle's own solution after one step.
The rule and the factor are tests/test_gpu_feedback.py's: the kernel is the condensed arithmetic in another order on another
linearisation.  The figure is admitted on the CPU (tests/test_plan_derivative_shapes_ref.py): at most 1e-9 with soft terminal
rows and 1e-7 with the default rows, so the bound is at most 1e-7 / 1e-5.  A pair whose figure is above the cap is listed as
excluded there: it is called and checked for ok and finiteness, and carries no bound.
fp32 (grid A, wide_qp off and on): median and 99th percentile of the per-lane error against the fp64 dense reference within
4 x those of the numpy float emulation on the same lanes, whose Phi and Gamma are the single-precision oracle's; one test per
(case, form, call).  The weight gradients are held in three parts: all outputs (`g`), g_tw of the pole-angle rows alone
(`g_tw_angle`) and `du`.  The second is what pins the angle wrap of plan_weight_vjp_kernel: with the
wrap that sent in-range negative angles through + 2 pi - 2 pi the median of g_tw_angle was 4.9 x the emulation's at single 8/8
and 6.7 x at double 8/8, measured on the MI355X.
Two pairs stay as strict expected failures, XFAIL below: the weight gradients at 16/1 in both models, in the tail of `g`.
Every test prints its figures before it asserts; DESIGN.md, "Feedback gains", records them."""
import numpy as np
import pytest

from helpers import feedback_ref as fr
from helpers import plan_shapes as sh

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = sh.LANES
CASES = sh.cases()
GRID_A = sh.grid_a()


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def golden():
    return sh.load_golden()


class Calls:
    """The four calls of one handle at one z (None: the handle's own solution), all rows, with ok."""

    def __init__(self, opt, case, inp, dtype, z=None):
        dyn = fr.DYN[case.model]
        gbar = T(inp.gbar, dtype)
        u_prev = torch.full((B,), inp.u_prev, dtype=dtype, device=DEV)
        K, ok = opt.feedback_gain(dyn, n_rows=case.N, z=z, want_ok=True)
        sens = opt.plan_sensitivity(dyn, n_rows=case.N, z=z, want_ok=True)
        vjp = opt.plan_vjp(dyn, gbar, z=z, want_ok=True)
        wv = opt.plan_weight_vjp(T(inp.x0, dtype), dyn, gbar, set_point=inp.set_point, u_prev=u_prev, z=z, want_du=True,
                                 want_ok=True)
        assert tuple(K.shape) == (case.N, opt.nx, B) and tuple(sens["k_sp"].shape) == tuple(sens["k_up"].shape) == (case.N, B)
        assert tuple(vjp["x0"].shape) == tuple(wv["terminal"].shape) == (opt.nx, B) and tuple(wv["du"].shape) == (case.N, B)
        self.ok = {"gain": ok, "sensitivity": sens["ok"], "vjp": vjp["ok"], "weight_vjp": wv["ok"]}
        self.tensors = {"gain": [K], "sensitivity": [sens["K"], sens["k_sp"], sens["k_up"]],
                        "vjp": [vjp["x0"], vjp["set_point"], vjp["u_prev"]],
                        "weight_vjp": [wv["terminal"], wv["u"], wv["du_dt"], wv["du"]]}
        self.K, self.sens_K = K, sens["K"]
        Kn, ksp, kup, du = N_(K), N_(sens["k_sp"]), N_(sens["k_up"]), N_(wv["du"])
        gv = np.concatenate([N_(vjp["x0"]), N_(vjp["set_point"])[None], N_(vjp["u_prev"])[None]]).T
        gw = np.concatenate([N_(wv["terminal"]), N_(wv["u"])[None], N_(wv["du_dt"])[None]]).T
        self.lane = {"gain": lambda b: {"K": Kn[:, :, b]},
                     "sensitivity": lambda b: {"k_sp": ksp[:, b], "k_up": kup[:, b]},
                     "vjp": lambda b: {"g": gv[b]},
                     "weight_vjp": lambda b: {"g": gw[b], "du": du[:, b]}}

    def assert_ok_and_finite(self):
        for call in sh.CALLS:
            assert N_(self.ok[call]).all(), (call, "ok", np.flatnonzero(N_(self.ok[call]) == 0))
            for t in self.tensors[call]:
                assert torch.isfinite(t).all(), call

    def worst(self, orc, case, p, z, inp):
        """{call: (worst error over the lanes and the call's parts, its lane)} against the dense references at z [dim, B]."""
        out = {}
        for call in sh.CALLS:
            errs = np.array([max(sh.errors(call, self.lane[call](b), sh.dense(orc, case, p, call, z[:, b], inp, b)).values())
                             for b in range(B)])
            out[call] = (float(errs.max()), int(errs.argmax()))
        return out


@pytest.mark.parametrize("case", CASES, ids=[sh.case_key(c) for c in CASES])
def test_fp64_every_call_matches_the_dense_reference(pkg, orc, golden, case):
    key = sh.case_key(case)
    stored, excluded = golden["cases"][key]["calls"], sh.excluded_pairs(golden)
    smp = sh.sample(orc, case)
    inp = sh.inputs(case, smp.x0)
    opt = pkg.BatchOptimization(sh.handle_params(pkg, orc, case), max_batch=B, dtype=torch.float64, device=0, model=case.model)
    assert (opt.N, opt.S, opt.dim) == (case.N, case.N // case.sp + 1, smp.z.shape[0])
    dyn = fr.DYN[case.model]
    # the oracle's z, explicitly, before any step; then the handle's own solution after one
    at_z = Calls(opt, case, inp, torch.float64, z=T(smp.z))
    assert not opt.has_previous_solution()
    e_z = at_z.worst(orc, case, smp.p, smp.z, inp)
    opt.step(T(smp.x0), dyn, 0.0)
    z_own = N_(opt.get_solution(B))
    own = Calls(opt, case, inp, torch.float64)
    e_own = own.worst(orc, case, smp.p, z_own, inp)
    for call in sh.CALLS:
        bound = 100.0 * stored[call]["figure"]
        print("SHAPES fp64 %s %s: worst error, explicit z %.3e, own solution %.3e, bound %.3e%s (pipeline %s)"
              % (key, call, e_z[call][0], e_own[call][0], bound, " [excluded]" if (key, call) in excluded else "",
                 opt.pipeline()))
    at_z.assert_ok_and_finite()
    own.assert_ok_and_finite()
    for call in sh.CALLS:
        if (key, call) in excluded:
            continue
        bound = 100.0 * stored[call]["figure"]
        assert bound <= 100.0 * sh.CAP[case.rows]
        assert e_z[call][0] <= bound, (call, "explicit z", e_z[call], bound)
        assert e_own[call][0] <= bound, (call, "own solution", e_own[call], bound)
    # a cut of the rows -- inside the first interval, at its end, one control into the next, all but the last -- is the
    # leading rows of all of them, bitwise
    for n in sh.n_rows_of(case):
        assert torch.equal(opt.feedback_gain(dyn, n_rows=n), own.K[:n]), n
        assert torch.equal(opt.feedback_gain(dyn, n_rows=n, z=T(smp.z)), at_z.K[:n]), n
        for z_t, whole in ((None, own.tensors["sensitivity"]), (T(smp.z), at_z.tensors["sensitivity"])):
            part = opt.plan_sensitivity(dyn, n_rows=n, z=z_t)
            for name, full in zip(("K", "k_sp", "k_up"), whole):
                assert part[name].shape[0] == n and torch.equal(part[name], full[:n]), (name, n, z_t is None)
    opt.close()


# (case, form, call) that miss the fp32 rule and stay as strict expected failures: two (case, call) pairs, the weight gradients
# at 16/1 in both models.  Measured on the MI355X, 99th percentile of `g`, GPU against 4 x the emulation's.  The emulation is
# handed the shooting defects of the DOUBLE oracle rounded to float; the kernel evaluates them in float, at a solved z a
# difference of nearly equal numbers that is off by as much as it is large, and 16/1 has sixteen defect rows.  With the
# single-precision oracle's defects in the emulation the same figures are within 1.0 x / 2.0 x / 2.2 x of it.
XFAIL = {("single/16x1/soft/D", False, "weight_vjp"): "g p99 3.03e-4 against 4 x 6.75e-5 (4.5 x the emulation)",
         ("double/16x1/soft/D", False, "weight_vjp"): "g p99 3.61e-4 against 4 x 4.74e-5 (7.6 x the emulation)",
         ("double/16x1/soft/D", True, "weight_vjp"): "g p99 4.15e-4 against 4 x 4.74e-5 (8.8 x the emulation)"}
# g_tw_angle is held in the median only.  It is there for a systematic error: the float wrap cost half an ulp of 2 pi on
# every lane whose angle residual is negative, about half of them, so it moved the median (4.9 x / 6.7 x the emulation at 8/8;
# 1.0 ... 3.0 x over grid A without it).  The 99th percentile of 70 lanes is the worst lane or two, where the conditioning
# of that lane and the float-evaluated defects decide; those outputs are in the tail of `g`, which is held by the rule above.
# The tail of g_tw_angle is printed: it is beyond 4 x at 16/1 (both models), double 6/1 and double 30/3 (4.6 ... 9.7 x).
MEDIAN_ONLY = ("g_tw_angle",)
FP32 = [pytest.param(c, wide, call, id="%s-%s-%s" % (sh.case_key(c), "wide" if wide else "plain", call),
                     marks=[pytest.mark.xfail(strict=True, reason=XFAIL[(sh.case_key(c), wide, call)])]
                     if (sh.case_key(c), wide, call) in XFAIL else [])
        for c in GRID_A for wide in (False, True) for call in sh.CALLS]


@pytest.mark.parametrize("case,wide,call", FP32)
def test_fp32_within_4x_of_the_float_emulation(pkg, orc, case, wide, call):
    key = sh.case_key(case)
    z32, inp = sh.float_sample(orc, case)
    opt = pkg.BatchOptimization(sh.handle_params(pkg, orc, case), max_batch=B, dtype=torch.float32, device=0, model=case.model,
                                wide_qp=wide)
    assert opt.wide_qp == wide
    res = Calls(opt, case, inp, torch.float32, z=T(z32, torch.float32))
    opt.close()
    emu, gpu = sh.float_lane_errors(orc, case, call, z32, inp, got=res.lane[call])
    figures = []
    for part in sh.PARTS[call]:
        g50, g99 = np.percentile(gpu[part], 50), np.percentile(gpu[part], 99)
        m50, m99 = np.percentile(emu[part], 50), np.percentile(emu[part], 99)
        print("SHAPES fp32 %s wide_qp=%s %s %s: GPU median %.3e p99 %.3e; emulation median %.3e p99 %.3e"
              % (key, wide, call, part, g50, g99, m50, m99))
        figures.append((part, g50, g99, m50, m99))
    res.assert_ok_and_finite()
    for part, g50, g99, m50, m99 in figures:
        assert g50 <= 4.0 * m50, (call, part, g50, m50)
        if part not in MEDIAN_ONLY:
            assert g99 <= 4.0 * m99, (call, part, g99, m99)


@pytest.mark.parametrize("dtype,wide", [(torch.float64, None), (torch.float32, False), (torch.float32, True)],
                         ids=["f64", "f32-plain", "f32-wide"])
@pytest.mark.parametrize("model", ["single", "double"])
def test_both_control_weights_zero_report_ok_0_and_nan(pkg, orc, model, dtype, wide):
    """u_cost_weight = u_derivative_cost_weight = 0 is a handle the library accepts; the control-cost Hessian is then zero,
    d_k <= 0 on every control, and the contract of a pivot that is not positive holds on every lane: ok = 0 and NaN in every
    output.  A handle with the default weights made afterwards gives the bits one made before gave."""
    case = sh.Case(model, 12, 4, "soft", "D")
    smp = sh.sample(orc, case)
    inp = sh.inputs(case, smp.x0, np.float64 if dtype == torch.float64 else np.float32)
    z = T(smp.z, dtype)

    def handle(weights=None):
        return pkg.BatchOptimization(sh.handle_params(pkg, orc, case, weights), max_batch=B, dtype=dtype, device=0, model=model,
                                     wide_qp=wide)
    first = handle()
    before = Calls(first, case, inp, dtype, z=z)
    before.assert_ok_and_finite()
    first.close()
    zero = handle((0.0, 0.0))
    got = Calls(zero, case, inp, dtype, z=z)
    for call in sh.CALLS:
        assert not N_(got.ok[call]).any(), call
        for t in got.tensors[call]:
            assert torch.isnan(t).all(), call
    second = handle()
    after = Calls(second, case, inp, dtype, z=z)
    for call in sh.CALLS:
        assert torch.equal(after.ok[call], before.ok[call])
        for a, b in zip(after.tensors[call], before.tensors[call]):
            assert torch.equal(a, b), call
    zero.close()
    second.close()
