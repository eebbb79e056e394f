"""Sensitivities of the plan to the set-point and to u_prev on the GPU (cpmpc_plan_sensitivity_batch), the update of the whole
plan made from them (cpmpc_plan_update_batch) and ClosedLoop.tick(set_point_inner=...), against the numpy references of
tests/helpers/plan_sensitivity_ref.py.

Shapes: N = 40, state_spacing 5, 10, 20 (20 puts the 6-state double handle on the split pipeline), both models, default and
mixed terminal rows, B = 130 -- two full waves and a partial one.  z is the handle's own solution after one cold-start step.
fp64 bound: 100 x the worst relative difference between the condensed closed forms and the dense KKT solve that the CPU
sample of the SAME configuration recorded (tests/golden/plan_sensitivity_sample.json) -- the rule and the margin of
tests/test_gpu_feedback.py, for its reason: the GPU's linearisation differs from the oracle's by rounding, amplified by the
same conditioning.  Relative to max |k_ref| per problem, every lane, all rows.
fp32: the GPU's median and 99th-percentile error against the fp64 reference are held to 4 x those of the numpy condensed
form with Phi, Gamma, Psi, w_k rounded to float32 and S, its solves in double, on the same lanes.
Every test prints its figures before it asserts; DESIGN.md section 5d is where they are recorded."""
import ctypes as C

import numpy as np
import pytest

from helpers import feedback_ref as fr
from helpers import plan_sensitivity_ref as ps

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = 130
ALL = ("K", "k_sp", "k_up")


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    return ps.load_golden()


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


def _check_rows_and_subsets(opt, model, full, **kw):
    """n_rows 1 and 3 are the leading rows of n_rows = N, each output asked for alone is the output asked for with the
    others, and K is cpmpc_feedback_gain_batch's: all bitwise, as include/cpmpc.h states."""
    for n in (1, 3):
        part = opt.plan_sensitivity(fr.DYN[model], n_rows=n, **kw)
        for name in ALL:
            assert part[name].shape[0] == n and torch.equal(part[name], full[name][:n]), (name, n)
    for name in ALL:
        alone = opt.plan_sensitivity(fr.DYN[model], n_rows=opt.N, want=(name,), **kw)
        assert list(alone) == [name] and torch.equal(alone[name], full[name]), name
    pair = opt.plan_sensitivity(fr.DYN[model], n_rows=opt.N, want=("k_sp", "k_up"), **kw)
    assert torch.equal(pair["k_sp"], full["k_sp"]) and torch.equal(pair["k_up"], full["k_up"])
    assert torch.equal(opt.feedback_gain(fr.DYN[model], n_rows=opt.N, **kw), full["K"])
    assert torch.equal(opt.feedback_gain(fr.DYN[model], n_rows=1, **kw), full["K"][:1])


@pytest.mark.parametrize("model,sp,mix", fr.configs(), ids=[fr.config_key(*c) for c in fr.configs()])
def test_fp64_matches_dense_reference(pkg, orc, golden, model, sp, mix):
    po, pg = _params(pkg, orc, model, sp, mix)
    bound = 100.0 * golden["configs"][fr.config_key(model, sp, mix)]["condensed_vs_dense_worst_rel"]
    opt, z = _stepped(pkg, pg, model, sp, mix, torch.float64)
    if model == "double" and sp == 20:
        assert opt.pipeline() == "split"
    N = opt.N
    full = opt.plan_sensitivity(fr.DYN[model], n_rows=N, want_ok=True)
    assert tuple(full["K"].shape) == (N, opt.nx, B) and tuple(full["k_sp"].shape) == tuple(full["k_up"].shape) == (N, B)
    assert N_(full["ok"]).all()
    k_sp, k_up = N_(full["k_sp"]), N_(full["k_up"])
    e_sp, e_up = [], []
    for b in range(B):
        sd, ud = ps.sensitivity_ref(orc, po, fr.DYN[model], z[:, b], model=model)
        e_sp.append(ps.rel_err(k_sp[:, b], sd))
        e_up.append(ps.rel_err(k_up[:, b], ud))
    e_sp, e_up = np.array(e_sp), np.array(e_up)
    print("%s fp64: worst rel error k_sp %.3e, k_up %.3e, bound %.3e (pipeline %s)"
          % (fr.config_key(model, sp, mix), e_sp.max(), e_up.max(), bound, opt.pipeline()))
    assert e_sp.max() <= bound, (e_sp.max(), bound, int(e_sp.argmax()))
    assert e_up.max() <= bound, (e_up.max(), bound, int(e_up.argmax()))
    _check_rows_and_subsets(opt, model, full)
    opt.close()


@pytest.mark.parametrize("model,wide", [("single", False), ("single", True), ("double", False), ("double", True)])
def test_fp32_within_4x_of_the_float_emulation(pkg, orc, model, wide):
    sp, mix = 10, "default"
    po, pg = _params(pkg, orc, model, sp, mix)
    opt, z = _stepped(pkg, pg, model, sp, mix, torch.float32, wide=wide)
    assert opt.wide_qp == wide
    full = opt.plan_sensitivity(fr.DYN[model], n_rows=opt.N, want_ok=True)
    assert N_(full["ok"]).all()
    got = {n: N_(full[n]).astype(np.float64) for n in ("k_sp", "k_up")}
    assert all(np.isfinite(v).all() for v in got.values())
    e_gpu, e_emu = {"k_sp": [], "k_up": []}, {"k_sp": [], "k_up": []}
    for b in range(B):
        sd, ud = ps.sensitivity_ref(orc, po, fr.DYN[model], z[:, b], model=model)
        _, se, ue = ps.condensed_ref(orc, po, fr.DYN[model], z[:, b], model=model, lin=np.float32)
        for name, kd, ke in (("k_sp", sd, se), ("k_up", ud, ue)):
            e_gpu[name].append(ps.rel_err(got[name][:, b], kd))
            e_emu[name].append(ps.rel_err(ke, kd))
    for name in ("k_sp", "k_up"):
        g50, g99 = np.percentile(e_gpu[name], 50), np.percentile(e_gpu[name], 99)
        m50, m99 = np.percentile(e_emu[name], 50), np.percentile(e_emu[name], 99)
        print("%s fp32 wide_qp=%s %s: GPU median %.3e p99 %.3e; emulation median %.3e p99 %.3e"
              % (model, wide, name, g50, g99, m50, m99))
        assert g50 <= 4.0 * m50 and g99 <= 4.0 * m99, (name, g50, g99, m50, m99)
    _check_rows_and_subsets(opt, model, full)
    opt.close()


@pytest.mark.parametrize("dtype,wide", [(torch.float32, False), (torch.float32, True), (torch.float64, None)])
def test_poisoned_lane_reports_ok_0_and_disturbs_nobody(pkg, dtype, wide):
    model, sp = "single", 10
    opt, z = _stepped(pkg, pkg.default_params(state_spacing=sp), model, sp, "default", dtype, wide=wide)
    dyn = np.tile(np.array(fr.DYN[model])[:, None], (1, B))
    clean = opt.plan_sensitivity(T(dyn, dtype), n_rows=opt.N, want_ok=True)
    bad = 70
    dyn[1, bad] = np.nan
    got = opt.plan_sensitivity(T(dyn, dtype), n_rows=opt.N, want_ok=True)
    assert N_(clean["ok"]).all()
    assert N_(got["ok"])[bad] == 0 and N_(got["ok"]).sum() == B - 1
    keep = [b for b in range(B) if b != bad]
    for name in ALL:
        assert torch.isnan(got[name][..., bad]).all(), name
        assert torch.equal(got[name][..., keep], clean[name][..., keep]), name
    only = opt.plan_sensitivity(T(dyn, dtype), n_rows=2, want=("k_up",), want_ok=True)   # one output alone: NaN too
    assert torch.isnan(only["k_up"][:, bad]).all() and N_(only["ok"])[bad] == 0
    opt.close()


@pytest.mark.parametrize("model,dtype,pipeline,wide", [
    ("single", torch.float64, "auto", None), ("single", torch.float32, "auto", True), ("single", torch.float32, "split", None),
    ("double", torch.float64, "split", None), ("double", torch.float32, "auto", None)])
def test_sensitivity_calls_leave_the_solver_untouched(pkg, model, dtype, pipeline, wide):
    """A step after sensitivity calls is bitwise the step of a twin handle that never made them."""
    sp = 10
    x0 = fr.sample_states(model, 5, B)
    x1 = x0 + np.random.default_rng(6).normal(0, 0.01, x0.shape)
    twins = [pkg.BatchOptimization(pkg.default_params(state_spacing=sp), max_batch=B, dtype=dtype, device=0, model=model,
                                   wide_qp=wide) for _ in range(2)]
    for o in twins:
        o.set_pipeline(pipeline)
        o.step(T(x0, dtype), fr.DYN[model], 0.0)
    a, b = twins
    a.plan_sensitivity(fr.DYN[model], n_rows=a.N)
    a.plan_sensitivity(fr.DYN[model], n_rows=1, want=("k_sp",), z=b.get_solution(B) * 0.5)
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
            opt.plan_sensitivity(fr.DYN["single"], n_rows=bad, z=z)
        assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        opt.plan_sensitivity(fr.DYN["single"])   # no previous solution, no z
    with pytest.raises(ValueError):
        opt.plan_sensitivity(fr.DYN["single"], z=z, want=())
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    inp.dyn_shared_host = C.cast(capi.dbl_array(fr.DYN["single"], 9), C.POINTER(C.c_double))
    k = torch.empty((1, 64), dtype=torch.float64, device=DEV)
    call = capi.load().cpmpc_plan_sensitivity_batch
    assert call(opt._h, 64, C.byref(inp), 1, None, k.data_ptr(), None, None, None) == capi.ERR_INVALID_ARG   # no warm start
    opt.step(torch.zeros((4, 32), dtype=torch.float64, device=DEV) + 0.1, fr.DYN["single"], 0.0)
    assert call(opt._h, 64, C.byref(inp), 1, None, k.data_ptr(), None, None, None) == capi.ERR_INVALID_ARG   # covers 32 only
    assert call(opt._h, 32, C.byref(inp), 1, None, None, None, None, None) == capi.ERR_INVALID_ARG           # no output
    assert call(opt._h, 65, C.byref(inp), 1, None, k.data_ptr(), None, None, None) in (capi.ERR_BATCH, capi.ERR_INVALID_ARG)
    assert call(opt._h, 32, C.byref(inp), 1, None, k.data_ptr(), None, None, None) == capi.OK
    torch.cuda.synchronize()
    opt.close()


def test_host_pointer_form_and_facade_equal_the_device_form(pkg):
    capi = pkg.capi
    lib = capi.load()
    model, sp = "single", 10
    opt, z = _stepped(pkg, pkg.default_params(state_spacing=sp), model, sp, "default", torch.float64)
    dev = opt.plan_sensitivity(fr.DYN[model], n_rows=2)
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    arr = capi.dbl_array(fr.DYN[model], 9)
    inp.dyn_shared_host = C.cast(arr, C.POINTER(C.c_double))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    K, k_sp, k_up = np.zeros((2, 4, B)), np.zeros((2, B)), np.zeros((2, B))
    ok = np.zeros(B, dtype=np.int32)
    capi.check(lib.cpmpc_plan_sensitivity_batch_host(opt._h, B, C.byref(inp), 2, K.ctypes.data_as(dp), k_sp.ctypes.data_as(dp),
                                                     k_up.ctypes.data_as(dp), ok.ctypes.data_as(ip)))
    assert ok.all() and np.array_equal(K, N_(dev["K"])) and np.array_equal(k_sp, N_(dev["k_sp"]))
    assert np.array_equal(k_up, N_(dev["k_up"]))
    zc = np.ascontiguousarray(z)   # an explicit z, one output alone
    inp.z = zc.ctypes.data
    k2 = np.zeros((2, B))
    capi.check(lib.cpmpc_plan_sensitivity_batch_host(opt._h, B, C.byref(inp), 2, None, None, k2.ctypes.data_as(dp), None))
    assert np.array_equal(k2, k_up)
    # the facade's single controller: the rows the batched call gives for its solution
    pp = pkg.pypendulum()
    prm = pp.SingleCartPoleParams(*fr.DYN["single"])
    one = pp.Optimization(pp.OptimizationParams())
    with pytest.raises(ValueError):
        one.plan_sensitivity(prm)
    x0 = fr.sample_states("single", 21, 1)[:, 0]
    one.step(pp.SingleCartPoleState(*x0), prm, 0.0)
    z1 = np.array(one.get_solution_batch(1)).reshape(-1, 1)
    Kf, sf, uf = one.plan_sensitivity(prm, 3)
    ref = pkg.BatchOptimization(pkg.default_params(), max_batch=1, dtype=torch.float64, device=0)
    want = ref.plan_sensitivity(fr.DYN["single"], n_rows=3, z=T(z1))
    assert np.array_equal(np.array(Kf).reshape(3, 4), N_(want["K"])[:, :, 0])
    assert np.array_equal(np.array(sf), N_(want["k_sp"])[:, 0]) and np.array_equal(np.array(uf), N_(want["k_up"])[:, 0])
    assert Kf == one.feedback_gain(prm, 3)
    with pytest.raises(ValueError):
        one.plan_sensitivity(prm, 41)
    ref.close()
    opt.close()


def _mod_pi(a):
    a = np.fmod(a, 2 * np.pi)
    a = np.where(a < 0, a + 2 * np.pi, a)
    return np.where(a > np.pi, a - 2 * np.pi, a)


@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_plan_update_matches_numpy(pkg, model, dtype):
    """u = clamp(u_nom + K . wrap(x - x_nom) + k_sp (sp - sp_nom) + k_up (u_prev - u_prev_nom), +-u_limit), every combination
    of absent terms, per element to 1e-13 = 450 eps (fp64; 450 eps_f in fp32) of max(|u_nom|, max |K||dx|, |k_sp dsp|,
    |k_up du_prev|): NX + 2 fused multiply-adds lose at most (NX + 2)(NX + 3) / 2 = 36 eps of that, and the float kernel's
    wrap subtracts a 2 pi rounded to float (1e-7 rad, times |K|) -- the multiple is feedback_apply's test's, the scale its
    max |K||dx| extended by the terms that are new here (|u_nom| bounds the rounding of the sum when every term is small).
    1 000 problems: four blocks, the last one partial; 3 rows."""
    nx, nq = (4, 2) if model == "single" else (6, 3)
    Bu, rows, u_limit = 1000, 3, 300.0
    rng = np.random.default_rng(3)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    K = rng.uniform(-200, 200, (rows, nx, Bu))
    K[:, :, ::7] *= 10.0                                  # some lanes run into the clamp
    x_nom = rng.uniform(-1, 1, (nx, Bu))
    x_nom[1:nq] = rng.uniform(-np.pi, np.pi, (nq - 1, Bu))
    x = x_nom + rng.uniform(-0.3, 0.3, (nx, Bu))
    x[1:nq] = _mod_pi(x[1:nq])                            # angle differences across +-pi
    u_nom = rng.uniform(-50, 50, (rows, Bu))
    k_sp, k_up = rng.uniform(-200, 200, (rows, Bu)), rng.uniform(-0.5, 0.5, (rows, Bu))
    sp_nom, sp = rng.uniform(-1, 1, Bu), rng.uniform(-1, 1, Bu)
    up_nom, up = rng.uniform(-100, 100, Bu), rng.uniform(-100, 100, Bu)
    K, x_nom, x, u_nom, k_sp, k_up, sp_nom, sp, up_nom, up = (
        a.astype(npdt) for a in (K, x_nom, x, u_nom, k_sp, k_up, sp_nom, sp, up_nom, up))
    f64 = np.float64
    dx = (x - x_nom).astype(f64)                          # the subtractions as the kernel sees them, in its type
    dx[1:nq] = _mod_pi(dx[1:nq])
    assert (np.abs(x[1:nq].astype(f64) - x_nom[1:nq]) > np.pi).sum() > 10   # wraps are exercised
    t_K = K.astype(f64) * dx[None]
    t_sp = k_sp.astype(f64) * (sp - sp_nom).astype(f64)[None]
    t_up = k_up.astype(f64) * (up - up_nom).astype(f64)[None]
    tol = 1e-13 * (1.0 if dtype == torch.float64 else np.finfo(np.float32).eps / np.finfo(np.float64).eps)
    g = {n: T(v, dtype) for n, v in dict(u_nom=u_nom, K=K, x_nom=x_nom, x=x, k_sp=k_sp, sp_nom=sp_nom, sp=sp, k_up=k_up,
                                        u_prev_nom=up_nom, u_prev=up).items()}
    worst = 0.0
    for use_K in (True, False):
        for use_sp in (True, False):
            for use_up in (True, False):
                kw = {}
                if use_K:
                    kw.update(K=g["K"], x_nom=g["x_nom"], x=g["x"])
                if use_sp:
                    kw.update(k_sp=g["k_sp"], sp_nom=g["sp_nom"], sp=g["sp"])
                if use_up:
                    kw.update(k_up=g["k_up"], u_prev_nom=g["u_prev_nom"], u_prev=g["u_prev"])
                got = N_(pkg.plan_update(g["u_nom"], u_limit=u_limit, model=model, **kw)).astype(f64)
                total = u_nom.astype(f64) + use_K * t_K.sum(axis=1) + use_sp * t_sp + use_up * t_up
                want = np.clip(total, -u_limit, u_limit)
                if not (use_K or use_sp or use_up):
                    assert np.array_equal(got, want)      # nothing but the clamp
                    continue
                scale = np.maximum.reduce([np.abs(u_nom.astype(f64)), use_K * np.abs(t_K).max(axis=1), use_sp * np.abs(t_sp),
                                           use_up * np.abs(t_up)])
                err = (np.abs(got - want) / scale).max()
                worst = max(worst, err)
                assert err <= tol, (use_K, use_sp, use_up, err, tol)
                if use_K and use_sp and use_up:
                    assert (np.abs(want) == u_limit).sum() > 10 and (np.abs(want) < u_limit).sum() > rows * Bu // 2
                    alias = g["u_nom"].clone()            # u_out aliasing u_nom: the same result
                    out = pkg.plan_update(alias, u_limit=u_limit, model=model, out=alias, **kw)
                    assert out is alias and np.array_equal(N_(alias).astype(f64), got)
                    free = N_(pkg.plan_update(g["u_nom"], u_limit=float("inf"), model=model, **kw)).astype(f64)
                    assert (np.abs(free) > u_limit).sum() > 10 and (np.abs(free - total) / scale).max() <= tol
    print("plan_update %s %s: worst error %.3e of max(|u_nom|, largest term) (tolerance %.3e)" % (model, dtype, worst, tol))


def test_sensitivities_predict_the_oracle_qp_at_a_moved_set_point_and_u_prev(pkg, orc, golden):
    """The QP is linear in both inputs: u_nom + k_sp 0.3 m + k_up 5 N, with the GPU's sensitivities at z, is the oracle's QP
    solution at the moved set-point and u_prev.  Tolerance: the fp64 bound of this configuration (relative to max |k_ref|
    per sensitivity) times the size of the update, 0.3 max |k_sp| + 5 max |k_up|, and nothing else: the two QP solves are an
    independent witness, so a sign or a convention that the dense reference shared with the kernel would show here.  (What
    the oracle's own two solves miss of their dense KKT derivative is 2e-4 of this tolerance at the worst lane of the configuration's 64-lane CPU sample.)"""
    model, sp, mix = "single", 10, "default"
    d_sp, d_up = 0.3, 5.0
    po, pg = _params(pkg, orc, model, sp, mix)
    bound = 100.0 * golden["configs"][fr.config_key(model, sp, mix)]["condensed_vs_dense_worst_rel"]
    opt, z = _stepped(pkg, pg, model, sp, mix, torch.float64)
    N, nx = opt.N, opt.nx
    sens = opt.plan_sensitivity(fr.DYN[model], n_rows=N, want=("k_sp", "k_up"))
    k_sp, k_up = N_(sens["k_sp"]), N_(sens["k_up"])
    worst = 0.0
    for b in range(B):
        zb = z[:, b]
        r, c, J, A = fr.problem_eval(orc, model, po, fr.DYN[model], zb[:nx], 0.1, 2.0, zb)
        r2, c2, _, _ = fr.problem_eval(orc, model, po, fr.DYN[model], zb[:nx], 0.1 + d_sp, 2.0 + d_up, zb)
        rc, dz = orc.qp_solve(J, r, A, c, N, 0.0)
        rc2, dz2 = orc.qp_solve(J, r2, A, c2, N, 0.0)
        assert rc == 0 and rc2 == 0
        u_nom, u_moved = (zb + dz)[-N:], (zb + dz2)[-N:]
        sd, ud = ps.sensitivity_ref(orc, po, fr.DYN[model], zb, model=model)
        tol = bound * (d_sp * np.abs(sd).max() + d_up * np.abs(ud).max())
        err = np.abs(u_nom + d_sp * k_sp[:, b] + d_up * k_up[:, b] - u_moved).max()
        worst = max(worst, err / tol)
        assert err <= tol, (b, err, tol)
        assert np.abs(u_moved - u_nom).max() > 1.0    # the plan really moved (newtons)
    print("QP at the moved set-point and u_prev: worst error / tolerance %.3f" % worst)
    opt.close()


def test_closed_loop_set_point_inner(pkg):
    """set_point_inner absent or equal to the tick's set-point: bitwise the existing tick (3 ticks, 2 sub-steps).  A different
    inner set-point moves the applied control by k_sp[0] times the difference on every lane with ok = 1."""
    dyn, delta = fr.DYN["single"], 0.3
    x0 = T(fr.sample_states("single", 11, B))
    loops = [pkg.ClosedLoop(pkg.default_params(), B, dtype=torch.float64, device=0, feedback=True) for _ in range(4)]
    old, absent, equal, moved = loops
    for cl in loops:
        cl.set_state(x0)
    sp_t = torch.full((B,), 0.2, dtype=torch.float64, device=DEV)
    for t in range(3):
        old.tick(dyn, 0.2, substeps=2)
        moved.tick(dyn, 0.2, substeps=2)
        absent.tick(dyn, 0.2, substeps=2, set_point_inner=None)
        equal.tick(dyn, 0.2, substeps=2, set_point_inner=0.2 if t == 1 else sp_t)   # a float or a [B] tensor
        for cl in (absent, equal):
            assert torch.equal(cl.applied[0], old.applied[0]), t
            assert torch.equal(cl.state(), old.state()) and torch.equal(cl.controls(), old.controls()), t
    # one more tick of two loops in the same state, one sub-step (x = x0: the gain term is K . 0)
    old.tick(dyn, 0.2, substeps=1)
    moved.tick(dyn, 0.2, substeps=1, set_point_inner=0.2 + delta)
    assert torch.equal(moved.controls(), old.controls())       # the same plan
    sens = moved.opts[0].plan_sensitivity(dyn, n_rows=1, want=("k_sp",), want_ok=True)
    ok, k0 = sens["ok"].bool(), sens["k_sp"][0]
    assert ok.all() and torch.isfinite(k0).all()
    u_nom = old.controls()[0]
    assert torch.equal(old.applied[0], u_nom.clamp(-300.0, 300.0))
    want = (u_nom + k0 * delta).clamp(-300.0, 300.0)
    # The kernel rounds u_nom + k0 d once (a fused multiply-add, d = 0.5 - 0.2 being the double 0.3), `want` rounds the
    # product and then the sum: with unit roundoff eps / 2 the two differ by at most eps / 2 (|k0 d| + 2 |u_nom + k0 d|)
    # <= 2 eps (|u_nom| + |k0 d|), and the clamp widens no difference.
    eps = np.finfo(np.float64).eps
    tol = 2 * eps * (u_nom.abs() + (k0 * delta).abs())
    err = (moved.applied[0] - want).abs()
    print("closed loop, moved inner set-point: worst |applied - (u_0 + k_sp[0] d)| / tolerance %.3f" % (err / tol).max().item())
    assert (err <= tol).all()
    assert ((moved.applied[0] - old.applied[0]).abs() > 1.0).sum() > B // 2                          # newtons, not rounding
    with pytest.raises(ValueError):
        pkg.ClosedLoop(pkg.default_params(), 4, dtype=torch.float64, device=0).tick(dyn, set_point_inner=0.1)
    for cl in loops:
        cl.close()


def test_closed_loop_lane_without_sensitivities_holds_the_plan(pkg):
    """A lane whose sensitivity call reports ok = 0 (NaN outputs) holds the plan's u_0 under a moved inner set-point."""
    dyn = fr.DYN["single"]
    x0 = T(fr.sample_states("single", 13, B))
    plain = pkg.ClosedLoop(pkg.default_params(), B, dtype=torch.float64, device=0)
    fb = pkg.ClosedLoop(pkg.default_params(), B, dtype=torch.float64, device=0, feedback=True)
    real = fb.opts[0].plan_sensitivity

    def withheld(dyn, **kw):
        res = real(dyn, **kw)
        for name in ("K", "k_sp"):
            res[name][..., ::3] = float("nan")
        res["ok"][::3] = 0
        return res
    fb.opts[0].plan_sensitivity = withheld
    for cl in (plain, fb):
        cl.set_state(x0)
    plain.tick(dyn, 0.0)
    fb.tick(dyn, 0.0, substeps=1, set_point_inner=0.3)
    assert torch.isfinite(fb.applied[0]).all()
    assert torch.equal(fb.applied[0][::3], plain.controls()[0][::3])
    assert not torch.equal(fb.applied[0][1::3], plain.controls()[0][1::3])
    for cl in (plain, fb):
        cl.close()
