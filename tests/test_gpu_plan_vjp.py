"""The reverse mode of the plan's sensitivities on the GPU (cpmpc_plan_vjp_batch, BatchOptimization.plan_vjp and
step_differentiable) against the numpy references of tests/helpers/plan_vjp_ref.py.

Shapes: N = 40, B = 130 -- two full waves and a partial one.  z is the handle's own solution after one cold-start step from
the configuration's seeded states, as in tests/test_gpu_plan_sensitivity.py.
fp64: every configuration of feedback_ref.configs() (state_spacing 20 puts the 6-state handle on the split pipeline), both
golden cotangents, every lane and every output within 100 x the worst relative difference between the condensed and the dense
adjoint that the CPU sample of the SAME configuration recorded (tests/golden/plan_vjp_sample.json) -- the rule and the margin
of tests/test_gpu_feedback.py, for its reason: the GPU's linearisation differs from the oracle's by rounding, amplified by the
same conditioning.  Relative to max |ref| per problem over its NX + 2 outputs.
fp32: the GPU's median and 99th-percentile error against the fp64 dense reference are held to 4 x those of the numpy condensed
adjoint with Phi, Gamma, Psi, w_k rounded to float32 on the same lanes (the existing fp32 rule).
Every test prints its figures before it asserts; DESIGN.md section 5d is where they are recorded."""
import ctypes as C

import numpy as np
import pytest

from helpers import feedback_ref as fr
from helpers import plan_vjp_ref as pv

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = 130
ALL = ("x0", "set_point", "u_prev")


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def packed(res):
    """[B, NX + 2]: the helper's layout."""
    return np.concatenate([N_(res["x0"]), N_(res["set_point"])[None], N_(res["u_prev"])[None]]).astype(np.float64).T


@pytest.fixture(scope="module")
def golden():
    return pv.load_golden()


def _params(pkg, orc, model, sp, mix):
    tw = fr.TERMINAL_MIXES[mix]
    tw = None if tw is None else tw[model]
    po = fr.params_for(orc, model, sp, tw)
    pg = pkg.default_params(state_spacing=sp, b_x_final_cost_weight=po.b_x_final_cost_weight,
                            th_final_cost_weight=po.th_final_cost_weight,
                            b_x_dot_final_cost_weight=po.b_x_dot_final_cost_weight,
                            th_dot_final_cost_weight=po.th_dot_final_cost_weight)
    return po, pg


def _stepped(pkg, pg, model, sp, mix, dtype, wide=None):
    """A handle after one cold-start step from the configuration's seeded states: (handle, z [dim, B] as float64)."""
    opt = pkg.BatchOptimization(pg, max_batch=B, dtype=dtype, device=0, model=model, wide_qp=wide)
    x0 = fr.sample_states(model, fr.config_seed(model, sp, mix), B)
    opt.step(T(x0, dtype), fr.DYN[model], 0.0)
    return opt, N_(opt.get_solution(B)).astype(np.float64)


def _check_bitwise_properties(opt, model, gbar, full, **kw):
    """Each output asked for alone is the output asked for with the others; n_rows = 1 and 3 are n_rows = N with the
    cotangent padded with zeros; two consecutive calls agree: all bitwise, as include/cpmpc.h states."""
    dyn = fr.DYN[model]
    again = opt.plan_vjp(dyn, gbar, want_ok=True, **kw)
    for name in ALL + ("ok",):
        assert torch.equal(again[name], full[name]), name
    for name in ALL:
        alone = opt.plan_vjp(dyn, gbar, want=(name,), **kw)
        assert list(alone) == [name] and torch.equal(alone[name], full[name]), name
    pair = opt.plan_vjp(dyn, gbar, want=("set_point", "u_prev"), **kw)
    assert torch.equal(pair["set_point"], full["set_point"]) and torch.equal(pair["u_prev"], full["u_prev"])
    for n in (1, 3):
        padded = torch.zeros_like(gbar)
        padded[:n] = gbar[:n]
        part = opt.plan_vjp(dyn, gbar[:n].contiguous(), **kw)
        whole = opt.plan_vjp(dyn, padded, **kw)
        for name in ALL:
            assert torch.equal(part[name], whole[name]), (name, n)
        assert not torch.equal(part["x0"], full["x0"])   # the rows beyond n do count


@pytest.mark.parametrize("model,sp,mix", fr.configs(), ids=[fr.config_key(*c) for c in fr.configs()])
def test_fp64_matches_dense_reference(pkg, orc, golden, model, sp, mix):
    po, pg = _params(pkg, orc, model, sp, mix)
    bound = 100.0 * golden["configs"][fr.config_key(model, sp, mix)]["condensed_vs_dense_worst_rel"]
    opt, z = _stepped(pkg, pg, model, sp, mix, torch.float64)
    if model == "double" and sp == 20:
        assert opt.pipeline() == "split"
    cots = pv.cotangents(model, sp, mix, B, opt.N)
    for name in pv.COTANGENTS:
        gbar = T(cots[name])
        full = opt.plan_vjp(fr.DYN[model], gbar, want_ok=True)
        assert tuple(full["x0"].shape) == (opt.nx, B) and tuple(full["set_point"].shape) == tuple(full["u_prev"].shape) == (B,)
        assert N_(full["ok"]).all()
        got = packed(full)
        err = np.array([pv.rel_err(got[b], pv.dense_vjp(orc, po, fr.DYN[model], z[:, b], cots[name][:, b], model=model))
                        for b in range(B)])
        print("%s fp64 %s: worst rel error %.3e, bound %.3e (pipeline %s)"
              % (fr.config_key(model, sp, mix), name, err.max(), bound, opt.pipeline()))
        assert err.max() <= bound, (name, err.max(), bound, int(err.argmax()))
        if name == "uniform":
            _check_bitwise_properties(opt, model, gbar, full)
    opt.close()


@pytest.mark.parametrize("model,wide", [("single", False), ("single", True), ("double", False), ("double", True)])
def test_fp32_within_4x_of_the_float_emulation(pkg, orc, model, wide):
    sp, mix = 10, "default"
    po, pg = _params(pkg, orc, model, sp, mix)
    opt, z = _stepped(pkg, pg, model, sp, mix, torch.float32, wide=wide)
    assert opt.wide_qp == wide
    cots = pv.cotangents(model, sp, mix, B, opt.N)
    for name in pv.COTANGENTS:
        gbar = T(cots[name], torch.float32)
        g_used = N_(gbar).astype(np.float64)   # the cotangent as the float kernel reads it
        full = opt.plan_vjp(fr.DYN[model], gbar, want_ok=True)
        assert N_(full["ok"]).all()
        got = packed(full)
        assert np.isfinite(got).all()
        e_gpu, e_emu = [], []
        for b in range(B):
            gd = pv.dense_vjp(orc, po, fr.DYN[model], z[:, b], g_used[:, b], model=model)
            ge = pv.condensed_ref(orc, po, fr.DYN[model], z[:, b], g_used[:, b], model=model, lin=np.float32)
            e_gpu.append(pv.rel_err(got[b], gd))
            e_emu.append(pv.rel_err(ge, gd))
        g50, g99 = np.percentile(e_gpu, 50), np.percentile(e_gpu, 99)
        m50, m99 = np.percentile(e_emu, 50), np.percentile(e_emu, 99)
        print("%s fp32 wide_qp=%s %s: GPU median %.3e p99 %.3e; emulation median %.3e p99 %.3e"
              % (model, wide, name, g50, g99, m50, m99))
        assert g50 <= 4.0 * m50 and g99 <= 4.0 * m99, (name, g50, g99, m50, m99)
        if name == "uniform":
            _check_bitwise_properties(opt, model, gbar, full)
    opt.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_unit_cotangents_against_the_forward_rows(pkg, dtype):
    """e_0 and e_{N-1} at n_rows = N give rows 0 and N - 1 of plan_sensitivity's K, k_sp, k_up.  A cross-check that is
    printed, not asserted beyond finiteness: the two kernels round differently and the forward kernels' own GPU error
    figures are not on record."""
    model, sp = "single", 10
    opt, _ = _stepped(pkg, pkg.default_params(state_spacing=sp), model, sp, "default", dtype)
    sens = opt.plan_sensitivity(fr.DYN[model], n_rows=opt.N)
    for j in (0, opt.N - 1):
        gbar = torch.zeros((opt.N, B), dtype=dtype, device=DEV)
        gbar[j] = 1.0
        res = opt.plan_vjp(fr.DYN[model], gbar)
        for name, fwd in (("x0", sens["K"][j]), ("set_point", sens["k_sp"][j]), ("u_prev", sens["k_up"][j])):
            assert torch.isfinite(res[name]).all()
            diff = (res[name] - fwd).abs().max().item() / fwd.abs().max().item()
            print("%s unit cotangent e_%d, %s: max |vjp - forward row| / max |forward row| = %.3e" % (dtype, j, name, diff))
    opt.close()


@pytest.mark.parametrize("dtype,wide", [(torch.float32, False), (torch.float32, True), (torch.float64, None)])
def test_poisoned_lane_reports_ok_0_and_disturbs_nobody(pkg, dtype, wide):
    model, sp = "single", 10
    opt, _ = _stepped(pkg, pkg.default_params(state_spacing=sp), model, sp, "default", dtype, wide=wide)
    gbar = T(pv.cotangents(model, sp, "default", B, opt.N)["uniform"], dtype)
    dyn = np.tile(np.array(fr.DYN[model])[:, None], (1, B))
    clean = opt.plan_vjp(T(dyn, dtype), gbar, want_ok=True)
    bad = 70
    dyn[1, bad] = np.nan
    got = opt.plan_vjp(T(dyn, dtype), gbar, want_ok=True)
    assert N_(clean["ok"]).all()
    assert N_(got["ok"])[bad] == 0 and N_(got["ok"]).sum() == B - 1
    keep = [b for b in range(B) if b != bad]
    for name in ALL:
        assert torch.isnan(got[name][..., bad]).all(), name
        assert torch.isfinite(clean[name]).all(), name
        assert torch.equal(got[name][..., keep], clean[name][..., keep]), name
    only = opt.plan_vjp(T(dyn, dtype), gbar[:2].contiguous(), want=("u_prev",), want_ok=True)   # one output alone: NaN too
    assert torch.isnan(only["u_prev"][bad]) and N_(only["ok"])[bad] == 0
    opt.close()


@pytest.mark.parametrize("model,dtype,pipeline,wide", [
    ("single", torch.float64, "auto", None), ("single", torch.float32, "auto", True), ("single", torch.float32, "auto", False),
    ("single", torch.float32, "split", False), ("double", torch.float64, "split", None),
    ("double", torch.float32, "auto", True), ("double", torch.float32, "auto", False)])
def test_vjp_calls_leave_the_solver_untouched(pkg, model, dtype, pipeline, wide):
    """A step after VJP calls is bitwise the step of a twin handle that never made them: every instantiation a handle can
    reach (fp64 of both models, fp32 plain and wide of both models, wide_qp given explicitly), and the split pipeline."""
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
    a.plan_vjp(fr.DYN[model], gbar)
    a.plan_vjp(fr.DYN[model], gbar[:1].contiguous(), want=("set_point",), z=b.get_solution(B) * 0.5)
    assert a.previous_solution_batch() == b.previous_solution_batch() == B
    assert torch.equal(a.get_solution(B), b.get_solution(B))
    ra = a.step(T(x1, dtype), fr.DYN[model], 0.0, want_guess=True)
    rb = b.step(T(x1, dtype), fr.DYN[model], 0.0, want_guess=True)
    for name in ("u", "predicted_states", "status", "iterations", "ls_evals", "final_cost", "final_eq_l1", "guess"):
        assert torch.equal(getattr(ra, name), getattr(rb, name)), name
    assert torch.equal(a.get_solution(B), b.get_solution(B))
    for o in twins:
        o.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_step_differentiable(pkg, dtype):
    model, sp = "single", 10
    dyn = fr.DYN[model]
    x0_np = fr.sample_states(model, fr.config_seed(model, sp, "default"), B)
    x1 = T(x0_np + 0.01, dtype)
    sp_np = np.random.default_rng(8).uniform(-0.2, 0.2, B)
    opt, twin = (pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=dtype, device=0)
                 for _ in range(2))
    x0, spt = T(x0_np, dtype).requires_grad_(), T(sp_np, dtype).requires_grad_()
    for bad_rows in (0, opt.N + 1):   # refused before the step: the handle has not moved
        with pytest.raises(ValueError):
            opt.step_differentiable(x0, dyn, spt, n_rows=bad_rows)
    assert opt.previous_solution_batch() == 0
    u, o = opt.step_differentiable(x0, dyn, spt)
    ref = twin.step(T(x0_np, dtype), dyn, T(sp_np, dtype))
    assert torch.equal(o.u, ref.u) and torch.equal(o.status, ref.status)
    assert tuple(u.shape) == (opt.N, B) and torch.equal(u.detach(), ref.u) and u.requires_grad
    z = opt.get_solution(B)
    G = T(pv.cotangents(model, sp, "default", B, opt.N)["uniform"], dtype)
    opt.step(x1, dyn, 0.0)   # a later step on the handle before backward: the graph holds its own z
    gx, gs = torch.autograd.grad((u * G).sum(), (x0, spt))
    want = twin.plan_vjp(dyn, G, z=z, want=("x0", "set_point"), want_ok=True)
    assert N_(want["ok"]).all() and torch.isfinite(gx).all() and gx.abs().max() > 0
    assert torch.equal(gx, want["x0"]) and torch.equal(gs, want["set_point"])
    # the leading rows only, the set-point a float: one gradient
    x0b = T(x0_np, dtype).requires_grad_()
    u3, _ = twin.step_differentiable(x0b, dyn, 0.1, n_rows=3)
    assert tuple(u3.shape) == (3, B)
    z3 = twin.get_solution(B)
    (u3 * G[:3]).sum().backward()
    assert torch.equal(x0b.grad, twin.plan_vjp(dyn, G[:3].contiguous(), z=z3, want="x0")["x0"])
    # a poisoned lane (per-problem parameters, NaN from the start): gradient 0, not NaN, the other lanes untouched; raw
    # plan_vjp keeps NaN
    bad = 70
    dyn_pp = np.tile(np.array(dyn)[:, None], (1, B))
    grads = []
    for poisoned, h in ((False, twin), (True, opt)):
        dyn_t = T(dyn_pp, dtype)
        if poisoned:
            dyn_t[1, bad] = float("nan")
        h.reset()
        x0c = T(x0_np, dtype).requires_grad_()
        uc, _ = h.step_differentiable(x0c, dyn_t, 0.0)
        zc = h.get_solution(B)
        dyn_t.fill_(float("nan"))   # the graph keeps its own copy of dyn
        grads.append(torch.autograd.grad((uc * G).sum(), (x0c,))[0])
    keep = [b for b in range(B) if b != bad]
    assert torch.isfinite(grads[1]).all() and (grads[1][:, bad] == 0).all() and grads[0][:, bad].abs().max() > 0
    assert torch.equal(grads[1][:, keep], grads[0][:, keep])
    dyn_bad = T(dyn_pp, dtype)
    dyn_bad[1, bad] = float("nan")
    raw = opt.plan_vjp(dyn_bad, G, z=zc, want="x0", want_ok=True)
    assert N_(raw["ok"])[bad] == 0 and N_(raw["ok"]).sum() == B - 1 and torch.isnan(raw["x0"][:, bad]).all()
    for h in (opt, twin):
        h.close()


def test_argument_checks_with_a_handle(pkg):
    capi = pkg.capi
    opt = pkg.BatchOptimization(pkg.default_params(), max_batch=64, dtype=torch.float64, device=0)
    z = torch.zeros((opt.dim, 64), dtype=torch.float64, device=DEV)
    with pytest.raises(capi.CpmpcError) as e:
        opt.plan_vjp(fr.DYN["single"], torch.zeros((opt.N + 1, 64), dtype=torch.float64, device=DEV), z=z)
    assert e.value.code == capi.ERR_INVALID_ARG
    g = torch.zeros((2, 64), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        opt.plan_vjp(fr.DYN["single"], g)   # no previous solution, no z
    with pytest.raises(ValueError):
        opt.plan_vjp(fr.DYN["single"], g, z=z, want=())
    with pytest.raises(ValueError):
        opt.plan_vjp(fr.DYN["single"], g[:, :32].contiguous(), z=z)   # gbar's batch is not z's
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    inp.dyn_shared_host = C.cast(capi.dbl_array(fr.DYN["single"], 9), C.POINTER(C.c_double))
    k = torch.empty((64,), dtype=torch.float64, device=DEV)
    call = capi.load().cpmpc_plan_vjp_batch
    assert call(opt._h, 64, C.byref(inp), 1, g.data_ptr(), None, k.data_ptr(), None, None, None) == capi.ERR_INVALID_ARG
    opt.step(torch.zeros((4, 32), dtype=torch.float64, device=DEV) + 0.1, fr.DYN["single"], 0.0)
    assert call(opt._h, 64, C.byref(inp), 1, g.data_ptr(), None, k.data_ptr(), None, None, None) == capi.ERR_INVALID_ARG
    assert call(opt._h, 32, C.byref(inp), 1, g.data_ptr(), None, None, None, None, None) == capi.ERR_INVALID_ARG   # no output
    assert call(opt._h, 32, C.byref(inp), 1, None, None, k.data_ptr(), None, None, None) == capi.ERR_INVALID_ARG   # no gbar
    assert call(opt._h, 32, C.byref(inp), 1, g.data_ptr(), None, k.data_ptr(), None, None, None) == capi.OK
    torch.cuda.synchronize()
    opt.close()


def test_host_pointer_form_and_facade_equal_the_device_form(pkg):
    capi = pkg.capi
    lib = capi.load()
    model, sp = "single", 10
    opt, z = _stepped(pkg, pkg.default_params(state_spacing=sp), model, sp, "default", torch.float64)
    gb = np.ascontiguousarray(pv.cotangents(model, sp, "default", B, opt.N)["uniform"][:3])
    dev = opt.plan_vjp(fr.DYN[model], T(gb))
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    arr = capi.dbl_array(fr.DYN[model], 9)
    inp.dyn_shared_host = C.cast(arr, C.POINTER(C.c_double))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    gx, gs, gu = np.zeros((4, B)), np.zeros(B), np.zeros(B)
    ok = np.zeros(B, dtype=np.int32)
    capi.check(lib.cpmpc_plan_vjp_batch_host(opt._h, B, C.byref(inp), 3, gb.ctypes.data_as(dp), gx.ctypes.data_as(dp),
                                             gs.ctypes.data_as(dp), gu.ctypes.data_as(dp), ok.ctypes.data_as(ip)))
    assert ok.all() and np.array_equal(gx, N_(dev["x0"])) and np.array_equal(gs, N_(dev["set_point"]))
    assert np.array_equal(gu, N_(dev["u_prev"]))
    zc = np.ascontiguousarray(z)   # an explicit z, one output alone
    inp.z = zc.ctypes.data
    g2 = np.zeros(B)
    capi.check(lib.cpmpc_plan_vjp_batch_host(opt._h, B, C.byref(inp), 3, gb.ctypes.data_as(dp), None, None,
                                             g2.ctypes.data_as(dp), None))
    assert np.array_equal(g2, gu)
    # the facade's single controller: what the batched call gives for its solution
    pp = pkg.pypendulum()
    prm = pp.SingleCartPoleParams(*fr.DYN["single"])
    one = pp.Optimization(pp.OptimizationParams())
    with pytest.raises(ValueError):
        one.plan_vjp(prm, [1.0])   # before the first step
    x0 = fr.sample_states("single", 21, 1)[:, 0]
    one.step(pp.SingleCartPoleState(*x0), prm, 0.0)
    z1 = np.array(one.get_solution_batch(1)).reshape(-1, 1)
    g1 = [0.5, -1.0, 0.25]
    fx, fs, fu = one.plan_vjp(prm, g1)
    ref = pkg.BatchOptimization(pkg.default_params(), max_batch=1, dtype=torch.float64, device=0)
    want = ref.plan_vjp(fr.DYN["single"], T(np.array(g1)[:, None]), z=T(z1))
    assert np.array_equal(np.array(fx), N_(want["x0"])[:, 0])
    assert fs == N_(want["set_point"])[0] and fu == N_(want["u_prev"])[0]
    for bad in ([], [0.0] * 41):
        with pytest.raises(ValueError):
            one.plan_vjp(prm, bad)
    ref.close()
    opt.close()
