"""The gradients of the plan with respect to the cost weights on the GPU (cpmpc_plan_weight_vjp_batch,
BatchOptimization.plan_weight_vjp and step_differentiable(weight_grad=True)) against the numpy references of
tests/helpers/plan_weight_vjp_ref.py.

Shapes: N = 40, B = 130 -- two full waves and a 2-lane tail.  z is the handle's own solution after one cold-start step from
the configuration's seeded states; the call's inputs are the sample's: x0 = those states + 0.01, set-point 0.3, u_prev 0.7.
fp64: every configuration of feedback_ref.configs() (state_spacing 20 puts the 6-state handle on the split pipeline), both
golden cotangents, every lane: g_tw, g_wu, g_wdu relative to `scale` and du relative to max |du_ref| within 100 x the worst
condensed-vs-dense figure that the CPU sample of the SAME configuration recorded (tests/golden/plan_weight_vjp_sample.json) --
the rule and the margin of tests/test_gpu_feedback.py, for its reason: the GPU's linearisation differs from the oracle's by
rounding, amplified by the same conditioning.
fp32: the GPU's median and 99th-percentile error against the fp64 dense reference are held to 4 x those of the numpy condensed
form with lin=np.float32 on the same lanes (the existing fp32 rule).
Every test prints its figures before it asserts; DESIGN.md section 5d is where they are recorded."""
import ctypes as C

import numpy as np
import pytest

from helpers import feedback_ref as fr
from helpers import plan_vjp_ref as pv
from helpers import plan_weight_vjp_ref as pw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = 130
ALL = ("terminal", "u", "du_dt")


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def packed(res):
    """[B, NX + 2]: the helper's layout."""
    return np.concatenate([N_(res["terminal"]), N_(res["u"])[None], N_(res["du_dt"])[None]]).astype(np.float64).T


@pytest.fixture(scope="module")
def golden():
    return pw.load_golden()


def _params(pkg, orc, model, sp, mix):
    tw = fr.TERMINAL_MIXES[mix]
    tw = None if tw is None else tw[model]
    po = fr.params_for(orc, model, sp, tw)
    pg = pkg.default_params(state_spacing=sp, b_x_final_cost_weight=po.b_x_final_cost_weight,
                            th_final_cost_weight=po.th_final_cost_weight,
                            b_x_dot_final_cost_weight=po.b_x_dot_final_cost_weight,
                            th_dot_final_cost_weight=po.th_dot_final_cost_weight)
    return po, pg


class Case:
    """A handle after one cold-start step from the configuration's seeded states, and the sample's inputs of the call."""

    def __init__(self, pkg, pg, model, sp, mix, dtype, wide=None, pipeline=None):
        self.model, self.dtype, self.dyn = model, dtype, fr.DYN[model]
        self.opt = pkg.BatchOptimization(pg, max_batch=B, dtype=dtype, device=0, model=model, wide_qp=wide)
        if pipeline is not None:
            self.opt.set_pipeline(pipeline)
        xs = fr.sample_states(model, fr.config_seed(model, sp, mix), B)
        self.opt.step(T(xs, dtype), self.dyn, 0.0)
        self.z = N_(self.opt.get_solution(B)).astype(np.float64)
        self.x0_t = T(pw.sample_inputs(xs), dtype)
        self.x0 = N_(self.x0_t).astype(np.float64)   # as the kernel reads it
        self.u_prev_t = torch.full((B,), pw.U_PREV, dtype=dtype, device=DEV)
        self.u_prev = float(N_(self.u_prev_t)[0])
        self.set_point = float(np.asarray(pw.SET_POINT, dtype=N_(self.u_prev_t).dtype))
        self.gbar = {k: T(v, dtype) for k, v in pv.cotangents(model, sp, mix, B, self.opt.N).items()}

    def call(self, gbar, **kw):
        kw.setdefault("set_point", pw.SET_POINT)
        kw.setdefault("u_prev", self.u_prev_t)
        return self.opt.plan_weight_vjp(self.x0_t, kw.pop("dyn", self.dyn), gbar, **kw)

    def dense(self, orc, po, b, gbar_np, **kw):
        return pw.dense_weight_vjp(orc, po, self.dyn, self.z[:, b], self.x0[:, b], gbar_np[:, b], set_point=self.set_point,
                                   u_prev=self.u_prev, model=self.model, **kw)


def _check_bitwise_properties(case, gbar, full, **kw):
    """Each output asked for alone is the output asked for with the others; n_rows = 1 and 3 are n_rows = N with the
    cotangent padded with zeros; two consecutive calls agree: all bitwise, as include/cpmpc.h states."""
    again = case.call(gbar, want_du=True, want_ok=True, **kw)
    for name in ALL + ("du", "ok"):
        assert torch.equal(again[name], full[name]), name
    for name in ALL:
        alone = case.call(gbar, want=(name,), **kw)
        assert list(alone) == [name] and torch.equal(alone[name], full[name]), name
    du_alone = case.call(None, want=(), want_du=True, **kw)
    assert list(du_alone) == ["du"] and torch.equal(du_alone["du"], full["du"])
    pair = case.call(gbar, want=("u", "du_dt"), **kw)
    assert torch.equal(pair["u"], full["u"]) and torch.equal(pair["du_dt"], full["du_dt"])
    for n in (1, 3):
        padded = torch.zeros_like(gbar)
        padded[:n] = gbar[:n]
        part = case.call(gbar[:n].contiguous(), want_du=True, **kw)
        whole = case.call(padded, want_du=True, **kw)
        for name in ALL:
            assert torch.equal(part[name], whole[name]), (name, n)
        assert tuple(part["du"].shape) == (n, B) and torch.equal(part["du"], full["du"][:n])
        assert torch.equal(whole["du"], full["du"])   # the primal step does not depend on the cotangent
        assert not torch.equal(part["u"], full["u"])   # the rows beyond n do count


@pytest.mark.parametrize("model,sp,mix", fr.configs(), ids=[fr.config_key(*c) for c in fr.configs()])
def test_fp64_matches_dense_reference(pkg, orc, golden, model, sp, mix):
    po, pg = _params(pkg, orc, model, sp, mix)
    bound = 100.0 * golden["configs"][fr.config_key(model, sp, mix)]["condensed_vs_dense_worst_rel"]
    case = Case(pkg, pg, model, sp, mix, torch.float64)
    opt = case.opt
    if model == "double" and sp == 20:
        assert opt.pipeline() == "split"
    for name in pw.COTANGENTS:
        gbar = case.gbar[name]
        full = case.call(gbar, want_du=True, want_ok=True)
        assert tuple(full["terminal"].shape) == (opt.nx, B) and tuple(full["u"].shape) == tuple(full["du_dt"].shape) == (B,)
        assert tuple(full["du"].shape) == (opt.N, B) and N_(full["ok"]).all()
        got, du = packed(full), N_(full["du"])
        g_np = N_(gbar)
        err, err_du = np.zeros(B), np.zeros(B)
        for b in range(B):
            gd, dud, sc = case.dense(orc, po, b, g_np)
            err[b], err_du[b] = pw.rel_err(got[b], gd, sc), pw.rel_err_du(du[:, b], dud)
        print("%s fp64 %s: worst error of the gradients / scale %.3e, of du / max |du| %.3e, bound %.3e (pipeline %s)"
              % (fr.config_key(model, sp, mix), name, err.max(), err_du.max(), bound, opt.pipeline()))
        assert err.max() <= bound, (name, err.max(), bound, int(err.argmax()))
        assert err_du.max() <= bound, (name, err_du.max(), bound, int(err_du.argmax()))
        if name == "uniform":
            _check_bitwise_properties(case, gbar, full)
    opt.close()


@pytest.mark.parametrize("model,wide", [("single", False), ("single", True), ("double", False), ("double", True)])
def test_fp32_within_4x_of_the_float_emulation(pkg, orc, model, wide):
    sp, mix = 10, "default"
    po, pg = _params(pkg, orc, model, sp, mix)
    case = Case(pkg, pg, model, sp, mix, torch.float32, wide=wide)
    assert case.opt.wide_qp == wide
    for name in pw.COTANGENTS:
        gbar = case.gbar[name]
        g_used = N_(gbar).astype(np.float64)   # the cotangent as the float kernel reads it
        full = case.call(gbar, want_du=True, want_ok=True)
        assert N_(full["ok"]).all()
        got, du = packed(full), N_(full["du"]).astype(np.float64)
        assert np.isfinite(got).all() and np.isfinite(du).all()
        e_gpu, e_emu, d_gpu, d_emu = [], [], [], []
        for b in range(B):
            gd, dud, sc = case.dense(orc, po, b, g_used)
            ge, due = pw.condensed_ref(orc, po, case.dyn, case.z[:, b], case.x0[:, b], g_used[:, b], set_point=case.set_point,
                                       u_prev=case.u_prev, model=model, lin=np.float32)
            e_gpu.append(pw.rel_err(got[b], gd, sc))
            e_emu.append(pw.rel_err(ge, gd, sc))
            d_gpu.append(pw.rel_err_du(du[:, b], dud))
            d_emu.append(pw.rel_err_du(due, dud))
        for what, eg, ee in (("gradients", e_gpu, e_emu), ("du", d_gpu, d_emu)):
            g50, g99 = np.percentile(eg, 50), np.percentile(eg, 99)
            m50, m99 = np.percentile(ee, 50), np.percentile(ee, 99)
            print("%s fp32 wide_qp=%s %s %s: GPU median %.3e p99 %.3e; emulation median %.3e p99 %.3e"
                  % (model, wide, name, what, g50, g99, m50, m99))
            assert g50 <= 4.0 * m50 and g99 <= 4.0 * m99, (name, what, g50, g99, m50, m99)
        if name == "uniform":
            _check_bitwise_properties(case, gbar, full)
    case.opt.close()


@pytest.mark.parametrize("model,dtype,wide", [("single", torch.float64, None), ("single", torch.float32, False),
                                              ("single", torch.float32, True), ("double", torch.float64, None),
                                              ("double", torch.float32, False), ("double", torch.float32, True)])
def test_poisoned_lane_reports_ok_0_and_disturbs_nobody(pkg, model, dtype, wide):
    """Every instantiation a handle can reach: both models, fp64, fp32 plain and wide."""
    sp = 10
    case = Case(pkg, pkg.default_params(state_spacing=sp), model, sp, "default", dtype, wide=wide)
    if wide is not None:
        assert case.opt.wide_qp == wide
    gbar = case.gbar["uniform"]
    dyn = np.tile(np.array(fr.DYN[model])[:, None], (1, B))
    clean = case.call(gbar, dyn=T(dyn, dtype), want_du=True, want_ok=True)
    bad = 70
    dyn[1, bad] = np.nan
    got = case.call(gbar, dyn=T(dyn, dtype), want_du=True, want_ok=True)
    assert N_(clean["ok"]).all()
    assert N_(got["ok"])[bad] == 0 and N_(got["ok"]).sum() == B - 1
    keep = [b for b in range(B) if b != bad]
    for name in ALL + ("du",):
        assert torch.isnan(got[name][..., bad]).all(), name
        assert torch.isfinite(clean[name]).all(), name
        assert torch.equal(got[name][..., keep], clean[name][..., keep]), name
    only = case.call(gbar[:2].contiguous(), dyn=T(dyn, dtype), want=("du_dt",), want_ok=True)   # one output alone: NaN too
    assert torch.isnan(only["du_dt"][bad]) and N_(only["ok"])[bad] == 0
    case.opt.close()


@pytest.mark.parametrize("model,dtype,wide", [("single", torch.float64, None), ("single", torch.float32, False),
                                              ("single", torch.float32, True), ("double", torch.float64, None),
                                              ("double", torch.float32, False), ("double", torch.float32, True)])
def test_equality_rows_and_a_zero_weight_give_exactly_zero(pkg, model, dtype, wide):
    """Per-problem terminal rows: lanes alternate between an equality-heavy mix and one with a zero weight."""
    sp = 10
    case = Case(pkg, pkg.default_params(state_spacing=sp), model, sp, "default", dtype, wide=wide)
    nx = case.opt.nx
    rows = {"single": ([40.0, -1.0, 0.0, 2.0], [150.0, -1.0, -1.0, -1.0]),
            "double": ([40.0, -1.0, 3.0, 0.0, 0.5, 0.0], [150.0, -1.0, -1.0, -1.0, -1.0, 2.0])}[model]
    tw = np.stack([np.array(rows[b % 2]) for b in range(B)], axis=1)
    res = case.call(case.gbar["uniform"], terminal_weights=T(tw, dtype), want_ok=True)
    assert N_(res["ok"]).all() and torch.isfinite(res["terminal"]).all()
    g = N_(res["terminal"])
    assert g.shape == (nx, B)
    assert (g[tw <= 0] == 0.0).all()          # exactly: equality rows and zero weights
    assert (g[tw > 0] != 0.0).all()           # and only those
    case.opt.close()


@pytest.mark.parametrize("model,dtype,pipeline,wide", [
    ("single", torch.float64, "auto", None), ("single", torch.float32, "auto", True), ("single", torch.float32, "auto", False),
    ("single", torch.float32, "split", False), ("double", torch.float64, "split", None),
    ("double", torch.float32, "auto", True), ("double", torch.float32, "auto", False)])
def test_calls_leave_the_solver_untouched(pkg, model, dtype, pipeline, wide):
    """A step after weight-gradient calls is bitwise the step of a twin handle that never made them: every instantiation a
    handle can reach (fp64 of both models, fp32 plain and wide of both models), and the split pipeline."""
    sp = 10
    x0 = fr.sample_states(model, 5, B)
    x1 = x0 + np.random.default_rng(6).normal(0, 0.01, x0.shape)
    twins = [pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=dtype, device=0, model=model,
                                   wide_qp=wide) for _ in range(2)]
    for o in twins:
        o.set_pipeline(pipeline)
        o.step(T(x0, dtype), fr.DYN[model], 0.0)
    a, b = twins
    if wide is not None:
        assert a.wide_qp == wide
    gbar = T(pv.cotangents(model, sp, "default", B, a.N)["uniform"], dtype)
    a.plan_weight_vjp(T(x1, dtype), fr.DYN[model], gbar, set_point=0.3, want_du=True)
    a.plan_weight_vjp(T(x1, dtype), fr.DYN[model], gbar[:1].contiguous(), want=("terminal",), z=b.get_solution(B) * 0.5)
    assert a.previous_solution_batch() == b.previous_solution_batch() == B
    assert torch.equal(a.get_solution(B), b.get_solution(B))
    ra = a.step(T(x1, dtype), fr.DYN[model], 0.0, want_guess=True)
    rb = b.step(T(x1, dtype), fr.DYN[model], 0.0, want_guess=True)
    for name in ("u", "predicted_states", "status", "iterations", "ls_evals", "final_cost", "final_eq_l1", "guess"):
        assert torch.equal(getattr(ra, name), getattr(rb, name)), name
    assert torch.equal(a.get_solution(B), b.get_solution(B))
    for o in twins:
        o.close()


def test_du_is_the_step_of_one_split_pipeline_iteration(pkg):
    """du at n_rows = N against u_after - u_before of one split-pipeline iteration from the same linearisation point, on a
    handle with max_iterations = 1 and lambda = 0, on the lanes where that iteration took the full step unclamped (one merit
    evaluation, the controls moved, none at the limit).  Warm-started from a converged twin's solution so that the full step
    is the rule; asserted only where at least 90 % of the lanes qualify.  Tolerance: the fp64 parity tests' 1e-5 on u.
    The two are not bitwise alike by construction: the solver wraps c_init and the terminal error with wrap_angles, the weight
    kernel leaves an angle already in (-pi, pi] as it is (wrap_angles_in_place), half an ulp of 2 pi apart (4.4e-16 here)."""
    model, sp, dtype = "single", 10, torch.float64
    dyn = fr.DYN[model]
    xs = fr.sample_states(model, fr.config_seed(model, sp, "default"), B)
    conv = pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=dtype, device=0)
    conv.step(T(xs), dyn, 0.0)
    z_conv = conv.get_solution(B)
    opts = pkg.default_solver_opts(lambda_initial=0.0)
    one = pkg.BatchOptimization(pkg.default_params(state_spacing=sp, max_iterations=1), max_batch=B, dtype=dtype, device=0,
                                opts=opts)
    one.set_pipeline("split")
    one.set_previous_solution(z_conv)
    x0 = T(pw.sample_inputs(xs))
    o = one.step(x0, dyn, pw.SET_POINT, want_guess=True)
    nxS = one.nx * one.S
    u_before, u_after = N_(o.guess)[nxS:], N_(o.u)
    u_prev = z_conv[nxS].clone()   # what the step's row w_du (u_0 - u_prev) saw: control 0 of the previous solution
    res = one.plan_weight_vjp(x0, dyn, None, set_point=pw.SET_POINT, u_prev=u_prev, z=o.guess.contiguous(), want=(),
                              want_du=True, want_ok=True)
    du = N_(res["du"])
    moved = np.abs(u_after - u_before).max(axis=0) > 0
    inside = np.abs(u_after).max(axis=0) < float(opts.u_limit)
    ok = (N_(o.ls_evals) == 1) & moved & inside & (N_(res["ok"]) != 0)
    diff = np.abs(du - (u_after - u_before)).max(axis=0)
    assert ok.any(), "no lane took the full step unclamped: the comparison would be vacuous"
    print("one split iteration: %d of %d lanes (%.0f %%) took the full step unclamped; max |du - (u_after - u_before)| on "
          "them %.3e; asserted: %s" % (ok.sum(), B, 100.0 * ok.sum() / B, diff[ok].max(), ok.sum() >= 0.9 * B))
    if ok.sum() >= 0.9 * B:
        assert diff[ok].max() <= 1e-5
    for h in (conv, one):
        h.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_step_differentiable_weight_grad(pkg, dtype):
    model, sp = "single", 10
    dyn = fr.DYN[model]
    x0_np = fr.sample_states(model, fr.config_seed(model, sp, "default"), B)
    sp_np = np.random.default_rng(8).uniform(-0.2, 0.2, B)
    tw_np = np.tile(np.array([40.0, -1.0, 3.0, 2.0])[:, None], (1, B))
    opt, twin = (pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=dtype, device=0)
                 for _ in range(2))
    G = T(pv.cotangents(model, sp, "default", B, opt.N)["uniform"], dtype)
    # weight_grad=False: outputs and the x0 / set-point gradients are bitwise the existing function's, whose own test
    # pins them to plan_vjp at the step's solution
    x0a, spa = T(x0_np, dtype).requires_grad_(), T(sp_np, dtype).requires_grad_()
    ua, oa = opt.step_differentiable(x0a, dyn, spa, terminal_weights=T(tw_np, dtype))
    ref = twin.step(T(x0_np, dtype), dyn, T(sp_np, dtype), terminal_weights=T(tw_np, dtype))
    z0 = twin.get_solution(B)
    assert torch.equal(oa.u, ref.u) and torch.equal(ua.detach(), ref.u)
    gx, gs = torch.autograd.grad((ua * G).sum(), (x0a, spa))
    want = twin.plan_vjp(dyn, G, z=z0, terminal_weights=T(tw_np, dtype), want=("x0", "set_point"))
    assert torch.equal(gx, want["x0"]) and torch.equal(gs, want["set_point"])
    # weight_grad=True on the warm handle: the same x0 / set-point gradients, and g_tw at the u_prev the step saw
    x1_np = x0_np + 0.01
    x0b, spb = T(x1_np, dtype).requires_grad_(), T(sp_np, dtype).requires_grad_()
    twb = T(tw_np, dtype).requires_grad_()
    with pytest.raises(ValueError):
        opt.step_differentiable(x0b, dyn, spb, weight_grad=True)   # no terminal_weights tensor
    u_prev = opt.get_solution(B)[opt.nx * opt.S].clone()
    ub, ob = opt.step_differentiable(x0b, dyn, spb, terminal_weights=twb, weight_grad=True)
    rb = twin.step(T(x1_np, dtype), dyn, T(sp_np, dtype), terminal_weights=T(tw_np, dtype))
    assert torch.equal(ob.u, rb.u) and torch.equal(ub.detach(), rb.u)
    z1 = opt.get_solution(B)
    opt.step(T(x0_np, dtype), dyn, 0.0)   # a later step on the handle before backward: the graph holds its own copies
    gx, gs, gt = torch.autograd.grad((ub * G).sum(), (x0b, spb, twb))
    want = twin.plan_vjp(dyn, G, z=z1, terminal_weights=T(tw_np, dtype), want=("x0", "set_point"))
    assert torch.equal(gx, want["x0"]) and torch.equal(gs, want["set_point"])
    wt = twin.plan_weight_vjp(T(x1_np, dtype), dyn, G, set_point=T(sp_np, dtype), u_prev=u_prev, z=z1,
                              terminal_weights=T(tw_np, dtype), want="terminal", want_ok=True)
    assert N_(wt["ok"]).all() and torch.isfinite(gt).all() and gt.abs().max() > 0
    assert torch.equal(gt, wt["terminal"])
    assert (gt[1] == 0).all()   # the equality row
    # cold start: u_prev is 0
    twin.reset()
    x0c, twc = T(x0_np, dtype), T(tw_np, dtype).requires_grad_()
    uc, _ = twin.step_differentiable(x0c, dyn, 0.1, n_rows=3, terminal_weights=twc, weight_grad=True)
    zc = twin.get_solution(B)
    (uc * G[:3]).sum().backward()
    wc = opt.plan_weight_vjp(x0c, dyn, G[:3].contiguous(), set_point=0.1, u_prev=None, z=zc, terminal_weights=T(tw_np, dtype),
                             want="terminal")
    assert torch.equal(twc.grad, wc["terminal"])
    for h in (opt, twin):
        h.close()


def test_argument_checks_with_a_handle(pkg):
    capi = pkg.capi
    opt = pkg.BatchOptimization(pkg.default_params(), max_batch=64, dtype=torch.float64, device=0)
    z = torch.zeros((opt.dim, 64), dtype=torch.float64, device=DEV)
    x0 = torch.zeros((opt.nx, 64), dtype=torch.float64, device=DEV)
    g = torch.zeros((2, 64), dtype=torch.float64, device=DEV)
    with pytest.raises(capi.CpmpcError) as e:
        opt.plan_weight_vjp(x0, fr.DYN["single"], torch.zeros((opt.N + 1, 64), dtype=torch.float64, device=DEV), z=z)
    assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        opt.plan_weight_vjp(x0, fr.DYN["single"], g)   # no previous solution, no z
    with pytest.raises(ValueError):
        opt.plan_weight_vjp(x0, fr.DYN["single"], g, z=z, want=())   # nothing asked for
    with pytest.raises(ValueError):
        opt.plan_weight_vjp(x0, fr.DYN["single"], None, z=z)   # gradients without a cotangent
    with pytest.raises(ValueError):
        opt.plan_weight_vjp(x0, fr.DYN["single"], g[:, :32].contiguous(), z=z)   # gbar's batch is not x0's
    inp = capi.WeightVjpInputs(struct_size=C.sizeof(capi.WeightVjpInputs))
    inp.lin.struct_size = C.sizeof(capi.GainInputs)
    inp.lin.dyn_shared_host = C.cast(capi.dbl_array(fr.DYN["single"], 9), C.POINTER(C.c_double))
    inp.x0 = x0.data_ptr()
    k = torch.empty((64,), dtype=torch.float64, device=DEV)
    call = capi.load().cpmpc_plan_weight_vjp_batch
    bad = capi.ERR_INVALID_ARG
    assert call(opt._h, 64, C.byref(inp), 1, g.data_ptr(), None, k.data_ptr(), None, None, None, None) == bad   # no z, no step yet
    opt.step(x0[:, :32].contiguous() + 0.1, fr.DYN["single"], 0.0)
    assert call(opt._h, 64, C.byref(inp), 1, g.data_ptr(), None, k.data_ptr(), None, None, None, None) == bad   # 32 < 64
    assert call(opt._h, 32, C.byref(inp), 1, g.data_ptr(), None, None, None, None, None, None) == bad           # no output
    assert call(opt._h, 32, C.byref(inp), 1, None, None, k.data_ptr(), None, None, None, None) == bad           # no gbar
    assert call(opt._h, 32, C.byref(inp), opt.N + 1, g.data_ptr(), None, k.data_ptr(), None, None, None, None) == bad
    assert call(opt._h, 32, C.byref(inp), 1, g.data_ptr(), None, k.data_ptr(), None, None, None, None) == capi.OK
    assert call(opt._h, 32, C.byref(inp), 1, None, None, None, None, k.data_ptr(), None, None) == capi.OK       # du alone
    torch.cuda.synchronize()
    opt.close()


def test_host_pointer_form_and_facade_equal_the_device_form(pkg):
    capi = pkg.capi
    lib = capi.load()
    model, sp = "single", 10
    case = Case(pkg, pkg.default_params(state_spacing=sp), model, sp, "default", torch.float64)
    gb = np.ascontiguousarray(N_(case.gbar["uniform"])[:3])
    sp_np = np.random.default_rng(9).uniform(-0.2, 0.2, B)
    dev = case.call(T(gb), set_point=T(sp_np), want_du=True)
    inp = capi.WeightVjpInputs(struct_size=C.sizeof(capi.WeightVjpInputs))
    inp.lin.struct_size = C.sizeof(capi.GainInputs)
    arr = capi.dbl_array(fr.DYN[model], 9)
    inp.lin.dyn_shared_host = C.cast(arr, C.POINTER(C.c_double))
    x0h, uph = np.ascontiguousarray(case.x0), np.full(B, pw.U_PREV)
    inp.x0, inp.set_point, inp.u_prev = x0h.ctypes.data, sp_np.ctypes.data, uph.ctypes.data
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    gt, gu, gd, du = np.zeros((4, B)), np.zeros(B), np.zeros(B), np.zeros((3, B))
    ok = np.zeros(B, dtype=np.int32)
    capi.check(lib.cpmpc_plan_weight_vjp_batch_host(case.opt._h, B, C.byref(inp), 3, gb.ctypes.data_as(dp),
                                                    gt.ctypes.data_as(dp), gu.ctypes.data_as(dp), gd.ctypes.data_as(dp),
                                                    du.ctypes.data_as(dp), ok.ctypes.data_as(ip)))
    assert ok.all() and np.array_equal(gt, N_(dev["terminal"])) and np.array_equal(gu, N_(dev["u"]))
    assert np.array_equal(gd, N_(dev["du_dt"])) and np.array_equal(du, N_(dev["du"]))
    zc = np.ascontiguousarray(case.z)   # an explicit z, one output alone
    inp.lin.z = zc.ctypes.data
    g2 = np.zeros(B)
    capi.check(lib.cpmpc_plan_weight_vjp_batch_host(case.opt._h, B, C.byref(inp), 3, gb.ctypes.data_as(dp), None, None,
                                                    g2.ctypes.data_as(dp), None, None))
    assert np.array_equal(g2, gd)
    # the facade's single controller: what the batched call gives for its solution
    pp = pkg.pypendulum()
    prm = pp.SingleCartPoleParams(*fr.DYN["single"])
    one = pp.Optimization(pp.OptimizationParams())
    x0 = fr.sample_states("single", 21, 1)[:, 0]
    with pytest.raises(ValueError):
        one.plan_weight_vjp(pp.SingleCartPoleState(*x0), prm, 0.0, 0.0, [1.0])   # before the first step
    one.step(pp.SingleCartPoleState(*x0), prm, 0.0)
    z1 = np.array(one.get_solution_batch(1)).reshape(-1, 1)
    g1 = [0.5, -1.0, 0.25]
    x1 = x0 + 0.01
    ft, fu, fd, fdu = one.plan_weight_vjp(pp.SingleCartPoleState(*x1), prm, 0.3, 0.7, g1)
    ref = pkg.BatchOptimization(pkg.default_params(), max_batch=1, dtype=torch.float64, device=0)
    want = ref.plan_weight_vjp(T(x1[:, None]), fr.DYN["single"], T(np.array(g1)[:, None]), set_point=0.3,
                               u_prev=T(np.array([0.7])), z=T(z1), want_du=True)
    assert np.array_equal(np.array(ft), N_(want["terminal"])[:, 0]) and np.array_equal(np.array(fdu), N_(want["du"])[:, 0])
    assert fu == N_(want["u"])[0] and fd == N_(want["du_dt"])[0]
    for bad in ([], [0.0] * 41):
        with pytest.raises(ValueError):
            one.plan_weight_vjp(pp.SingleCartPoleState(*x1), prm, 0.3, 0.7, bad)
    ref.close()
    case.opt.close()
