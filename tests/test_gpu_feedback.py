"""Feedback gains K = du / dx0 of the plan on the GPU (cpmpc_feedback_gain_batch, cpmpc_feedback_apply_batch,
ClosedLoop(feedback=True)) against the numpy references of tests/helpers/feedback_ref.py.

fp64 bound: 100 x the worst relative difference between the condensed closed form and the dense KKT solve that the CPU
sample of the SAME configuration recorded (tests/golden/feedback_gain_sample.json): the kernel is that condensed arithmetic
in another order on another sincos; 100 covers the tail of a four times larger sample and Phi / Gamma agreeing with the
oracle only to ~1e-12 through a system of condition up to 1e9.  Relative to max |K_ref| per problem, every lane, all rows.
fp32: no fixed number -- the GPU's median and 99th-percentile error against the fp64 reference are held to 4 x those of the
numpy condensed form with Phi, Gamma, Psi, w_k rounded to float32 and S, its solve in double, on the same lanes."""
import ctypes as C

import numpy as np
import pytest

from helpers import feedback_ref as fr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
LANES = 256


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    return fr.load_golden()


def _params(pkg, orc, model, sp, mix):
    tw = fr.TERMINAL_MIXES[mix]
    tw = None if tw is None else tw[model]
    po = fr.params_for(orc, model, sp, tw)
    pg = pkg.default_params(state_spacing=sp, b_x_final_cost_weight=po.b_x_final_cost_weight,
                            th_final_cost_weight=po.th_final_cost_weight,
                            b_x_dot_final_cost_weight=po.b_x_dot_final_cost_weight,
                            th_dot_final_cost_weight=po.th_dot_final_cost_weight)
    return po, pg


def _lane_errors(orc, po, model, z, K, **kw):
    """K [N, NX, B] from the GPU against the dense reference at z [dim, B]: relative error per lane."""
    errs = []
    for b in range(z.shape[1]):
        Kd = fr.feedback_gain_ref(orc, po, fr.DYN[model], z[:, b], model=model, **kw)
        errs.append(fr.rel_err(K[:, :, b], Kd))
    return np.array(errs)


@pytest.mark.parametrize("model,sp,mix", fr.configs(), ids=[fr.config_key(*c) for c in fr.configs()])
def test_fp64_gain_matches_dense_reference(pkg, orc, golden, model, sp, mix):
    po, pg = _params(pkg, orc, model, sp, mix)
    _, _, x0, z_cpu = fr.solve_sample(orc, model, sp, mix, LANES)
    bound = 100.0 * golden["configs"][fr.config_key(model, sp, mix)]["condensed_vs_dense_worst_rel"]
    opt = pkg.BatchOptimization(pg, max_batch=LANES, dtype=torch.float64, device=0, model=model)
    N, nx = opt.N, opt.nx
    # explicit z (the oracle's solutions), before any step: the handle needs no warm start for it
    K, ok = opt.feedback_gain(fr.DYN[model], n_rows=N, z=T(z_cpu), want_ok=True)
    assert tuple(K.shape) == (N, nx, LANES) and N_(ok).all()
    e_z = _lane_errors(orc, po, model, z_cpu, N_(K))
    assert not opt.has_previous_solution()
    # after a real step: z = None is the handle's own solution
    opt.step(T(x0), fr.DYN[model], 0.0)
    z_gpu = N_(opt.get_solution(LANES))
    K2, ok2 = opt.feedback_gain(fr.DYN[model], n_rows=N, want_ok=True)
    assert N_(ok2).all()
    e_prev = _lane_errors(orc, po, model, z_gpu, N_(K2))
    print("%s fp64: worst rel error, explicit z %.3e, previous solution %.3e, bound %.3e (pipeline %s)"
          % (fr.config_key(model, sp, mix), e_z.max(), e_prev.max(), bound, opt.pipeline()))
    assert e_z.max() <= bound, (e_z.max(), bound, int(e_z.argmax()))
    assert e_prev.max() <= bound, (e_prev.max(), bound, int(e_prev.argmax()))
    # n_rows = 1 is row 0 of n_rows = N, bitwise; a few rows likewise
    K1 = opt.feedback_gain(fr.DYN[model], n_rows=1)
    assert tuple(K1.shape) == (1, nx, LANES) and torch.equal(K1[0], K2[0])
    K3 = opt.feedback_gain(fr.DYN[model], n_rows=3, z=T(z_cpu))
    assert torch.equal(K3, K[:3])
    opt.close()


@pytest.mark.parametrize("model", ["single", "double"])
def test_per_problem_parameters_lane_by_lane(pkg, orc, model):
    """Per-problem dyn and terminal_weights: every lane against the dense reference made with ITS parameters.  Bound: 100 x the
    worst condensed-vs-dense difference of the numpy forms on these very lanes (the rule of the fp64 test, for a
    configuration the golden file does not hold)."""
    sp, B = 10, LANES
    rng = np.random.default_rng(77)
    _, _, x0, z = fr.solve_sample(orc, model, sp, "default", B)
    dyn = np.tile(np.array(fr.DYN[model])[:, None], (1, B))
    dyn[1] *= rng.uniform(0.8, 1.25, B)                    # pole mass
    dyn[2 if model == "single" else 3] *= rng.uniform(0.8, 1.25, B)   # (first) pole length
    default_w = [150.0] + [-1.0] * (3 if model == "single" else 5)   # the default parameters' rows, per problem
    mixes = [default_w, fr.TERMINAL_MIXES["mix"][model]]
    tw = np.stack([np.array(mixes[b % 2], dtype=np.float64) for b in range(B)], axis=1)
    opt = pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=torch.float64, device=0, model=model)
    K = N_(opt.feedback_gain(T(dyn), n_rows=opt.N, z=T(z), terminal_weights=T(tw)))
    p0 = fr.params_for(orc, model, sp)
    errs, cpu = [], []
    for b in range(B):
        Kd = fr.feedback_gain_ref(orc, p0, dyn[:, b], z[:, b], terminal_weights=tw[:, b], model=model)
        pb = fr.params_for(orc, model, sp, tw[:, b])
        Phi, Gam = fr.blocks_of(orc, pb, dyn[:, b], z[:, b], model)
        Rw, Dg = fr.terminal_rows(orc, pb, model, tw[:, b])
        Kc = fr.condensed_gain(Phi, Gam, Rw, Dg, pb.u_cost_weight, pb.u_derivative_cost_weight, sp)
        errs.append(fr.rel_err(K[:, :, b], Kd))
        cpu.append(fr.rel_err(Kc, Kd))
    errs, cpu = np.array(errs), np.array(cpu)
    print("%s per-problem parameters: GPU worst %.3e (even lanes %.3e, odd %.3e); numpy condensed worst %.3e / %.3e"
          % (model, errs.max(), errs[0::2].max(), errs[1::2].max(), cpu[0::2].max(), cpu[1::2].max()))
    for par in (0, 1):   # default rows / mixed rows: each against its own figure
        assert errs[par::2].max() <= 100.0 * cpu[par::2].max()
    opt.close()


@pytest.mark.parametrize("model,dtype,pipeline,wide", [
    ("single", torch.float64, "auto", None), ("single", torch.float64, "split", None), ("single", torch.float32, "auto", None),
    ("single", torch.float32, "auto", True), ("single", torch.float32, "split", True),
    ("double", torch.float64, "auto", None), ("double", torch.float32, "auto", None), ("double", torch.float32, "split", None)])
def test_gain_call_leaves_the_solver_untouched(pkg, orc, model, dtype, pipeline, wide):
    """A handle's warm start, get_solution() and the next step()'s outputs are bitwise those of a twin that never asked for
    gains: both models, both pipelines, the float kernels' wide form (the 6-state float handles are wide by default)."""
    sp, B = 10, 512
    x0 = fr.sample_states(model, 5, B)
    x1 = x0 + np.random.default_rng(6).normal(0, 0.01, x0.shape)
    twins = [pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=dtype, device=0, model=model,
                                   wide_qp=wide) for _ in range(2)]
    for o in twins:
        o.set_pipeline(pipeline)
        o.step(T(x0, dtype), fr.DYN[model], 0.0)
    a, b = twins
    z_other = T(fr.solve_sample(orc, model, sp, "default", 8)[3], dtype).repeat(1, B // 8).contiguous()
    a.feedback_gain(fr.DYN[model], n_rows=a.N)
    a.feedback_gain(fr.DYN[model], n_rows=1, z=z_other)
    assert a.previous_solution_batch() == b.previous_solution_batch() == B
    assert torch.equal(a.get_solution(B), b.get_solution(B))
    ra = a.step(T(x1, dtype), fr.DYN[model], 0.0, want_guess=True)
    rb = b.step(T(x1, dtype), fr.DYN[model], 0.0, want_guess=True)
    for name in ("u", "predicted_states", "status", "iterations", "ls_evals", "final_cost", "final_eq_l1", "guess"):
        assert torch.equal(getattr(ra, name), getattr(rb, name)), name
    assert torch.equal(a.get_solution(B), b.get_solution(B))
    for o in twins:
        o.close()


def test_argument_checks_with_a_handle(pkg):
    capi = pkg.capi
    opt = pkg.BatchOptimization(pkg.default_params(), max_batch=64, dtype=torch.float64, device=0)
    z = torch.zeros((opt.dim, 64), dtype=torch.float64, device=DEV)
    for bad in (0, -1, opt.N + 1):
        with pytest.raises(capi.CpmpcError) as e:
            opt.feedback_gain(fr.DYN["single"], n_rows=bad, z=z)
        assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        opt.feedback_gain(fr.DYN["single"])   # no previous solution, no z
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    inp.dyn_shared_host = C.cast(capi.dbl_array(fr.DYN["single"], 9), C.POINTER(C.c_double))
    K = torch.empty((1, 4, 64), dtype=torch.float64, device=DEV)
    lib = capi.load()
    assert lib.cpmpc_feedback_gain_batch(opt._h, 64, C.byref(inp), 1, K.data_ptr(), None, None) == capi.ERR_INVALID_ARG
    opt.step(torch.zeros((4, 32), dtype=torch.float64, device=DEV) + 0.1, fr.DYN["single"], 0.0)
    assert lib.cpmpc_feedback_gain_batch(opt._h, 64, C.byref(inp), 1, K.data_ptr(), None, None) == capi.ERR_INVALID_ARG
    assert lib.cpmpc_feedback_gain_batch(opt._h, 32, C.byref(inp), 1, K.data_ptr(), None, None) == capi.OK
    inp.struct_size = 8
    assert lib.cpmpc_feedback_gain_batch(opt._h, 32, C.byref(inp), 1, K.data_ptr(), None, None) == capi.ERR_INVALID_ARG
    torch.cuda.synchronize()
    opt.close()


@pytest.mark.parametrize("model,wide", [("single", False), ("single", True), ("double", False), ("double", True)])
def test_fp32_gain_within_4x_of_the_float_emulation(pkg, orc, model, wide):
    """Recorded on the MI355X (median / 99th percentile of the per-lane relative error against the fp64 reference, GPU then
    the numpy emulation): see DESIGN.md, "Feedback gains"."""
    sp, mix, B = 10, "default", LANES
    po, pg = _params(pkg, orc, model, sp, mix)
    _, _, _, z = fr.solve_sample(orc, model, sp, mix, B)
    z = z.astype(np.float32).astype(np.float64)   # the linearisation point both sides see
    opt = pkg.BatchOptimization(pg, max_batch=B, dtype=torch.float32, device=0, model=model, wide_qp=wide)
    assert opt.wide_qp == wide
    K, ok = opt.feedback_gain(fr.DYN[model], n_rows=opt.N, z=T(z, torch.float32), want_ok=True)
    K = N_(K).astype(np.float64)
    assert N_(ok).all() and np.isfinite(K).all()
    e_gpu, e_emu = [], []
    for b in range(B):
        Kd = fr.feedback_gain_ref(orc, po, fr.DYN[model], z[:, b], model=model)
        Ke = fr.condensed_gain_ref(orc, po, fr.DYN[model], z[:, b], model=model, lin=np.float32)
        e_gpu.append(fr.rel_err(K[:, :, b], Kd))
        e_emu.append(fr.rel_err(Ke, Kd))
    g50, g99 = np.percentile(e_gpu, 50), np.percentile(e_gpu, 99)
    m50, m99 = np.percentile(e_emu, 50), np.percentile(e_emu, 99)
    print("%s fp32 wide_qp=%s: GPU median %.3e p99 %.3e; emulation median %.3e p99 %.3e" % (model, wide, g50, g99, m50, m99))
    assert g50 <= 4.0 * m50 and g99 <= 4.0 * m99, (g50, g99, m50, m99)
    # n_rows = 1 is row 0, bitwise, in either form
    assert torch.equal(opt.feedback_gain(fr.DYN[model], n_rows=1, z=T(z, torch.float32))[0], T(K[0], torch.float32))
    opt.close()


@pytest.mark.parametrize("dtype,wide", [(torch.float32, False), (torch.float32, True), (torch.float64, None)])
def test_poisoned_lane_reports_ok_0_and_disturbs_nobody(pkg, orc, dtype, wide):
    model, sp, B = "single", 10, 192
    _, _, _, z = fr.solve_sample(orc, model, sp, "default", B)
    dyn = np.tile(np.array(fr.DYN[model])[:, None], (1, B))
    opt = pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=dtype, device=0, wide_qp=wide)
    K_clean, ok_clean = opt.feedback_gain(T(dyn, dtype), n_rows=opt.N, z=T(z, dtype), want_ok=True)
    bad = 70
    dyn[1, bad] = np.nan
    K, ok = opt.feedback_gain(T(dyn, dtype), n_rows=opt.N, z=T(z, dtype), want_ok=True)
    assert N_(ok_clean).all()
    assert N_(ok)[bad] == 0 and N_(ok).sum() == B - 1
    assert torch.isnan(K[:, :, bad]).all()
    keep = [b for b in range(B) if b != bad]
    assert torch.equal(K[:, :, keep], K_clean[:, :, keep])
    opt.close()


def test_host_pointer_form_equals_the_device_form(pkg, orc):
    capi = pkg.capi
    lib = capi.load()
    model, sp, B = "single", 10, 40
    _, _, x0, z = fr.solve_sample(orc, model, sp, "default", B)
    opt = pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=torch.float64, device=0)
    K_dev = N_(opt.feedback_gain(fr.DYN[model], n_rows=2, z=T(z)))
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    arr = capi.dbl_array(fr.DYN[model], 9)
    inp.dyn_shared_host = C.cast(arr, C.POINTER(C.c_double))
    zc = np.ascontiguousarray(z)
    inp.z = zc.ctypes.data
    K_host = np.zeros((2, 4, B))
    ok = np.zeros(B, dtype=np.int32)
    capi.check(lib.cpmpc_feedback_gain_batch_host(opt._h, B, C.byref(inp), 2, K_host.ctypes.data_as(C.POINTER(C.c_double)),
                                                  ok.ctypes.data_as(C.POINTER(C.c_int32))))
    assert ok.all() and np.array_equal(K_host, K_dev)
    # the handle's own solution, after a host-pointer-free step
    opt.step(T(x0), fr.DYN[model], 0.0)
    K_prev = N_(opt.feedback_gain(fr.DYN[model], n_rows=1))
    inp.z = None
    K1 = np.zeros((1, 4, B))
    capi.check(lib.cpmpc_feedback_gain_batch_host(opt._h, B, C.byref(inp), 1, K1.ctypes.data_as(C.POINTER(C.c_double)), None))
    assert np.array_equal(K1, K_prev)
    opt.close()


def _mod_pi(a):
    a = np.fmod(a, 2 * np.pi)
    a = np.where(a < 0, a + 2 * np.pi, a)
    return np.where(a > np.pi, a - 2 * np.pi, a)


@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_feedback_apply_matches_numpy(pkg, model, dtype):
    """u = clamp(u_nom + K0 . wrap(x - x_nom), +-u_limit): to 1e-13 (fp64; float eps-scaled: 1e-13 * eps_f / eps_d in fp32) of
    max |K| |dx| -- a handful of fused multiply-adds."""
    nx, nq = (4, 2) if model == "single" else (6, 3)
    B = 100000
    rng = np.random.default_rng(3)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    K0 = rng.uniform(-200, 200, (nx, B))
    K0[:, ::7] *= 10.0                                   # some lanes run into the clamp
    x_nom = rng.uniform(-1, 1, (nx, B))
    x_nom[1:nq] = rng.uniform(-np.pi, np.pi, (nq - 1, B))
    x = x_nom + rng.uniform(-0.3, 0.3, (nx, B))
    x[1:nq] = _mod_pi(x[1:nq])                           # angle differences across +-pi
    u_nom = rng.uniform(-50, 50, B)
    K0, x_nom, x, u_nom = (a.astype(npdt) for a in (K0, x_nom, x, u_nom))
    u_limit = 300.0
    got = N_(pkg.feedback_apply(T(u_nom, dtype), T(K0, dtype), T(x_nom, dtype), T(x, dtype), u_limit=u_limit, model=model))
    dx = x.astype(np.float64) - x_nom.astype(np.float64)
    if dtype == torch.float32:
        dx = (x - x_nom).astype(np.float64)              # the subtraction of two floats, as the kernel sees it
    dx[1:nq] = _mod_pi(dx[1:nq])
    assert (np.abs(x[1:nq].astype(np.float64) - x_nom[1:nq]) > np.pi).sum() > 100   # wraps are exercised
    prod = K0.astype(np.float64) * dx
    want = np.clip(u_nom + prod.sum(axis=0), -u_limit, u_limit)
    assert (np.abs(want) == u_limit).sum() > 100 and (np.abs(want) < u_limit).sum() > B // 2   # so is the clamp
    scale = np.abs(prod).max(axis=0)
    tol = 1e-13 * (1.0 if dtype == torch.float64 else np.finfo(np.float32).eps / np.finfo(np.float64).eps)
    err = np.abs(got - want) / scale
    print("feedback_apply %s %s: worst error %.3e of max |K||dx| (tolerance %.3e)" % (model, dtype, err.max(), tol))
    assert err.max() <= tol


def test_closed_loop_feedback_with_one_substep_is_the_plain_loop(pkg):
    """ClosedLoop(feedback=True).tick(substeps=1) applies u_0 + K[0] . 0: bitwise the controls and states of feedback=False;
    20 ticks, 4 096 controllers."""
    B, ticks = 4096, 20
    x0 = T(fr.sample_states("single", 11, B))
    loops = [pkg.ClosedLoop(pkg.default_params(), B, dtype=torch.float64, device=0, feedback=fb) for fb in (False, True)]
    for cl in loops:
        cl.set_state(x0)
    for t in range(ticks):
        loops[0].tick(fr.DYN["single"])
        loops[1].tick(fr.DYN["single"], substeps=1)
        assert torch.equal(loops[0].controls(), loops[1].controls()), t
        assert torch.equal(loops[1].applied[0], loops[0].controls()[0]), t
        assert torch.equal(loops[0].state(), loops[1].state()), t
    assert torch.isfinite(loops[1].state()).all()
    with pytest.raises(ValueError):
        loops[0].tick(fr.DYN["single"], substeps=2)
    for cl in loops:
        cl.close()


def test_facade_feedback_gain_is_the_batched_one(pkg, orc):
    """pendulum::Optimization::FeedbackGain (through pypendulum) for the single controller: the rows the batched call gives for
    the same solution, and INVALID_ARG -> ValueError before the first step."""
    pp = pkg.pypendulum()
    prm = pp.SingleCartPoleParams(*fr.DYN["single"])
    opt = pp.Optimization(pp.OptimizationParams())
    with pytest.raises(ValueError):
        opt.feedback_gain(prm)
    x0 = fr.sample_states("single", 21, 1)[:, 0]
    opt.step(pp.SingleCartPoleState(*x0), prm, 0.0)
    z = np.array(opt.get_solution_batch(1)).reshape(-1, 1)
    K = np.array(opt.feedback_gain(prm, 3)).reshape(3, 4)
    ref = pkg.BatchOptimization(pkg.default_params(), max_batch=1, dtype=torch.float64, device=0)
    assert np.array_equal(K, N_(ref.feedback_gain(fr.DYN["single"], n_rows=3, z=T(z)))[:, :, 0])
    Kd = fr.feedback_gain_ref(orc, orc.default_opt_params(), fr.DYN["single"], z[:, 0])
    assert fr.rel_err(K, Kd[:3]) < 1e-8
    with pytest.raises(ValueError):
        opt.feedback_gain(prm, 41)
    ref.close()


def test_closed_loop_lane_without_a_gain_holds_the_plan(pkg):
    """A controller whose gain call reports ok = 0 (NaN rows) is driven with the plan's u_0, as the plain loop drives it, not
    with NaN: here every third lane's gain is withheld, and with one sub-step the loop is still bitwise the plain one."""
    B, ticks = 768, 5
    x0 = T(fr.sample_states("single", 13, B))
    plain = pkg.ClosedLoop(pkg.default_params(), B, dtype=torch.float64, device=0)
    fb = pkg.ClosedLoop(pkg.default_params(), B, dtype=torch.float64, device=0, feedback=True)
    real = fb.opts[0].feedback_gain

    def withheld(dyn, n_rows=1, want_ok=False, **kw):
        K, ok = real(dyn, n_rows=n_rows, want_ok=True, **kw)
        K[:, :, ::3] = float("nan")
        ok[::3] = 0
        return (K, ok) if want_ok else K
    fb.opts[0].feedback_gain = withheld
    for cl in (plain, fb):
        cl.set_state(x0)
    for t in range(ticks):
        plain.tick(fr.DYN["single"])
        fb.tick(fr.DYN["single"], substeps=1)
        assert torch.isfinite(fb.applied[0]).all(), t
        assert torch.equal(fb.applied[0], plain.controls()[0]), t
        assert torch.equal(fb.state(), plain.state()), t
    # and with sub-steps the withheld lanes still get finite controls
    fb.tick(fr.DYN["single"], substeps=4)
    assert torch.isfinite(fb.applied[0]).all() and torch.isfinite(fb.state()).all()
    for cl in (plain, fb):
        cl.close()
