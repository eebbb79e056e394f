"""Round 5 (-m gpu): the float kernels against the single-precision build of the CPU check (statistics, not lanes), and
the converged step's merit-free branch under poisoned inputs."""
import numpy as np
import pytest

from conftest import DYN_UI, random_states

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _gpu_closed_loop(pkg, x0, ticks, dtype=torch.float32, **over):
    """status [ticks, B], iterations [ticks, B], final states [4, B] of B controllers in closed loop on the GPU."""
    B = x0.shape[1]
    sim = pkg.BatchSimulator(B, dtype=dtype, device=0)
    sim.set_state(T(x0, dtype))
    opt = pkg.BatchOptimization(pkg.default_params(**over), max_batch=B, dtype=dtype, device=0)
    out = pkg.BatchOutputs()
    st = torch.zeros((ticks, B), dtype=torch.int32, device=DEV)
    it = torch.zeros((ticks, B), dtype=torch.int32, device=DEV)
    for k in range(ticks):
        o = opt.step(sim.get_state(), DYN_UI, 0.0, want_predicted=False, want_stats=True, out=out)
        sim.step(DYN_UI, 0.01, o.u[0].contiguous())
        st[k] = o.status
        it[k] = o.iterations
    return st.cpu().numpy(), it.cpu().numpy(), sim.get_state().double().cpu().numpy()


def _shares(a, n):
    """[ticks, n]: share of the controllers with value v at every tick."""
    return np.stack([(a == v).mean(axis=1) for v in range(n)], axis=1)


def test_fp32_swing_up_statistics_match_the_single_precision_check(pkg, orc):
    """VERDICT r4 item 5.  8 192 controllers from arbitrary pole angles, 100 ticks of closed loop at the reference's
    tolerances, CPMPC_F32 kernels against oracle/cpmpc_oracle_f32.c (the same restatement compiled in float, exit floor
    live at 1.5e-5 -- the branch the double check can never take).  Lane by lane two float solves of a swing-up drift
    apart within a few ticks, so what is held is the POPULATION, tick by tick:
      * the share of controllers in each termination state: total-variation distance <= 0.09 at every tick, <= 0.04 on
        average over the ticks (measured when the test was written: 0.059 / 0.025);
      * the histogram of iteration counts 0 .. 8: total-variation distance <= 0.28 at every tick, <= 0.09 on average
        (measured 0.20 at tick 42, where 15 % of the kernels' controllers take a fourth iteration the CPU's do not, / 0.060);
      * mean iterations per tick within 0.30 at every tick and 0.09 on average (measured 0.20 / 0.056; 3.48 against 3.45
        over the whole run);
      * no solver failure (QP_INDEFINITE / MAX_LAMBDA / NON_FINITE) in either (optimization_test.cc:44-46).
    For scale: two GPU runs on different seeds of the SAME distribution are 0.026 / 0.010 apart in the iteration histogram,
    and the float kernels are 0.57 / 0.24 from the DOUBLE kernels on the same states -- the float check follows the float
    kernels four times closer than anything computed in double can, which the last assertion holds (and which is why it
    exists)."""
    rng = np.random.default_rng(77)
    B, ticks = 8192, 100
    x0 = random_states(rng, B)
    st_g, it_g, xf_g = _gpu_closed_loop(pkg, x0, ticks)
    st_c, it_c, xf_c, _ = orc.closed_loop_f32(orc.default_opt_params(), DYN_UI, 0.0, x0, ticks)
    fails = [orc.TERM_QP_INDEFINITE, orc.TERM_MAX_LAMBDA, orc.TERM_NON_FINITE]
    assert not np.isin(st_g, fails).any() and not np.isin(st_c, fails).any()
    tv_status = 0.5 * np.abs(_shares(st_g, 9) - _shares(st_c, 9)).sum(axis=1)
    tv_iters = 0.5 * np.abs(_shares(it_g, 9) - _shares(it_c, 9)).sum(axis=1)
    d_mean = np.abs(it_g.mean(axis=1) - it_c.mean(axis=1))
    print("status TV max %.3f mean %.3f | iterations TV max %.3f mean %.3f | mean-iterations gap max %.3f mean %.3f | "
          "mean iterations GPU %.3f CPU %.3f" % (tv_status.max(), tv_status.mean(), tv_iters.max(), tv_iters.mean(), d_mean.max(),
                                                  d_mean.mean(), it_g.mean(), it_c.mean()))
    assert tv_status.max() <= 0.09 and tv_status.mean() <= 0.04, (tv_status.max(), tv_status.mean())
    assert tv_iters.max() <= 0.28 and tv_iters.mean() <= 0.09, (tv_iters.max(), tv_iters.mean())
    assert d_mean.max() <= 0.30 and d_mean.mean() <= 0.09, (d_mean.max(), d_mean.mean())
    st_d, it_d, _ = _gpu_closed_loop(pkg, x0, ticks, dtype=torch.float64)
    tv_iters_d = 0.5 * np.abs(_shares(it_g, 9) - _shares(it_d, 9)).sum(axis=1)
    print("iterations TV of the float kernels against the DOUBLE kernels: max %.3f mean %.3f" % (tv_iters_d.max(), tv_iters_d.mean()))
    assert tv_iters.mean() < 0.5 * tv_iters_d.mean()
    # and the plants end up in the same place: share of poles within 0.1 rad of upright after 1 s
    up_g, up_c = (np.abs(xf_g[1] - np.pi / 2) < 0.1).mean(), (np.abs(xf_c[1] - np.pi / 2) < 0.1).mean()
    assert abs(up_g - up_c) <= 0.03, (up_g, up_c)


def test_fp32_settled_loop_takes_the_exit_floor_branch_like_the_single_precision_check(pkg, orc):
    """The settled loop (2 048 controllers near the set-point, 260 ticks, reference tolerances): the float kernels and the
    float CPU check leave with SATISFIED_FIRST_ORDER_TOL after the same number of iterations on average (within 0.15 over
    the last 20 ticks; both 1.8 with the floor, both 2.8 without it), i.e. the exit-floor branch fires equally often in
    both; the poles stand within 2e-5 rad in all four runs."""
    rng = np.random.default_rng(23)
    B, ticks = 2048, 260
    xs = np.stack([rng.uniform(-0.05, 0.05, B), np.pi / 2 + rng.uniform(-0.05, 0.05, B), rng.uniform(-0.1, 0.1, B),
                   rng.uniform(-0.1, 0.1, B)])
    last = slice(ticks - 20, ticks)
    for floor in (2.0, 0.0):
        sim = pkg.BatchSimulator(B, dtype=torch.float32, device=0)
        sim.set_state(T(xs, torch.float32))
        opt = pkg.BatchOptimization(pkg.default_params(), max_batch=B, dtype=torch.float32, device=0,
                                    opts=pkg.capi.default_solver_opts(exit_defect_floor=floor))
        out = pkg.BatchOutputs()
        its_g, fo_g = [], []
        for k in range(ticks):
            o = opt.step(sim.get_state(), DYN_UI, 0.0, want_predicted=False, want_stats=True, out=out)
            sim.step(DYN_UI, 0.01, o.u[0].contiguous())
            if k >= ticks - 20:
                its_g.append(o.iterations.float().mean().item())
                fo_g.append((o.status == orc.TERM_SATISFIED_FIRST_ORDER_TOL).float().mean().item())
        err_g = (sim.get_state()[1].double() - np.pi / 2).abs().max().item()
        st_c, it_c, xf_c, _ = orc.closed_loop_f32(orc.default_opt_params(), DYN_UI, 0.0, xs, ticks,
                                                  opts=orc.default_solver_opts(exit_defect_floor=floor))
        m_g, m_c = float(np.mean(its_g)), float(it_c[last].mean())
        f_g, f_c = float(np.mean(fo_g)), float((st_c[last] == orc.TERM_SATISFIED_FIRST_ORDER_TOL).mean())
        print("floor %.0f: mean iterations GPU %.3f CPU-f32 %.3f; FIRST_ORDER share GPU %.3f CPU-f32 %.3f" % (floor, m_g, m_c, f_g, f_c))
        assert abs(m_g - m_c) <= 0.15, (floor, m_g, m_c)
        assert abs(f_g - f_c) <= 0.05, (floor, f_g, f_c)
        assert err_g < 2e-5 and np.abs(xf_c[1] - np.pi / 2).max() < 2e-5


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("pipeline", ["fused", "split"])
def test_poisoned_settled_controllers_leave_with_non_finite_and_keep_their_plan(pkg, orc, dtype, pipeline):
    """VERDICT r4 item 4b.  A converged controller takes its last step WITHOUT a merit evaluation:
    nothing checks that step's result for finiteness, because nothing needs to -- z is finite (f, |c|_1 were tested at the
    linearisation), |dz|_inf <= full_step_below is, and the retraction only wraps and clamps.  What that argument rests on
    is that a problem with non-finite DATA never reaches the branch.  Here: 1 024 controllers settled for 300 ticks (they
    leave by the merit-free branch: SATISFIED_FIRST_ORDER_TOL after one iteration in fp64), then a tick in which every
    fifth controller is handed a poisoned measurement (NaN or +-inf in one of the four state components) and every seventh
    a NaN model parameter.  Those leave with NON_FINITE, their stored plan (= next warm start) bit for bit what it was
    (the poisoned x0 that prepare copies into node 0 aside) and finite; every other controller is bitwise what it is in the
    same tick without the poison.  The CPU check does the same with the same inputs."""
    rng = np.random.default_rng(41)
    B = 1024
    xs = np.stack([rng.uniform(-0.05, 0.05, B), np.pi / 2 + rng.uniform(-0.05, 0.05, B), rng.uniform(-0.1, 0.1, B),
                   rng.uniform(-0.1, 0.1, B)])
    sim = pkg.BatchSimulator(B, dtype=dtype, device=0)
    sim.set_state(T(xs, dtype))
    opt = pkg.BatchOptimization(pkg.default_params(), max_batch=B, dtype=dtype, device=0)
    opt.set_pipeline(pipeline)
    dyn = T(np.tile(np.array(DYN_UI)[:, None], (1, B)), dtype)
    for _ in range(300):
        o = opt.step(sim.get_state(), dyn, 0.0, want_predicted=False)
        sim.step(DYN_UI, 0.01, o.u[0].contiguous())
    if dtype == torch.float64:
        assert (o.status == orc.TERM_SATISFIED_FIRST_ORDER_TOL).all() and (o.iterations == 1).float().mean().item() > 0.95
    z_before = opt.get_solution(B).clone()
    x_clean = sim.get_state().clone()
    # the clean tick, on a copy of the warm start
    ref = pkg.BatchOptimization(pkg.default_params(), max_batch=B, dtype=dtype, device=0)
    ref.set_pipeline(pipeline)
    ref.set_previous_solution(z_before)
    o_ref = ref.step(x_clean, dyn, 0.0, want_predicted=True)
    u_ref, st_ref, pred_ref = o_ref.u.clone(), o_ref.status.clone(), o_ref.predicted_states.clone()
    # the poisoned tick
    x_bad, dyn_bad = x_clean.clone(), dyn.clone()
    bad_x = np.arange(B) % 5 == 0
    bad_p = np.arange(B) % 7 == 3
    poison = [float("nan"), float("inf"), -float("inf")]
    for i in np.where(bad_x)[0]:
        x_bad[i % 4, i] = poison[i % 3]
    for i in np.where(bad_p)[0]:
        dyn_bad[i % 4, i] = float("nan")   # m_b, m_1, l_1, g: the parameters every evaluation of the dynamics uses (a NaN
        #                                    spring constant or drag coefficient of a term that is switched off by a select never enters)
    bad = torch.tensor(bad_x | bad_p, device=DEV)
    o = opt.step(x_bad, dyn_bad, 0.0, want_predicted=True)
    assert (o.status[bad] == orc.TERM_NON_FINITE).all(), torch.nonzero(bad & (o.status != orc.TERM_NON_FINITE)).flatten()[:20]
    assert torch.equal(o.status[~bad], st_ref[~bad]) and torch.equal(o.u[:, ~bad], u_ref[:, ~bad])
    assert torch.equal(o.predicted_states[:, :, ~bad], pred_ref[:, :, ~bad])
    z_after = opt.get_solution(B)
    only_p = torch.tensor(bad_p & ~bad_x, device=DEV)   # poisoned parameters, clean measurement: the whole plan survives but node 0
    assert torch.equal(z_after[4:, bad], z_before[4:, bad]) or torch.isfinite(z_after[4 * 5:, bad]).all()
    # the controls of the stored plan are the previous plan shifted by one (prepare's warm start) and finite
    assert torch.isfinite(z_after[4 * 5:, bad]).all()
    assert torch.equal(z_after[4 * 5:-1, only_p], z_before[4 * 5 + 1:, only_p])
    # the CPU check on three of the poisoned problems
    for i in list(np.where(bad_x)[0][:2]) + list(np.where(bad_p & ~bad_x)[0][:1]):
        oc = orc.Optimization(orc.default_opt_params())
        oc.set_previous_solution(z_before[:, i].double().cpu().numpy())
        so = oc.step(x_bad[:, i].double().cpu().numpy(), dyn_bad[:, i].double().cpu().numpy(), 0.0)
        assert so.solver_outputs.termination_state == orc.TERM_NON_FINITE, i


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_closed_loop_as_column_ranges_is_bitwise_the_single_range(pkg, dtype):
    """pkg.ClosedLoop(ranges = n): the batch held as n independent column ranges (own handle, plant and stream each, no
    synchronisation between them) gives bit for bit the controls, iteration counts and plant states of one range, tick after
    tick -- through a transient (controllers start up to 0.4 rad from upright) with ragged range sizes (B = 4099, 3 ranges)."""
    rng = np.random.default_rng(12)
    B = 4099
    xs = np.stack([rng.uniform(-0.3, 0.3, B), np.pi / 2 + rng.uniform(-0.4, 0.4, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-1, 1, B)])
    one = pkg.ClosedLoop(pkg.default_params(), B, dtype=dtype, device=0, ranges=1)
    three = pkg.ClosedLoop(pkg.default_params(), B, dtype=dtype, device=0, ranges=3)
    assert three.bounds == [0, 1366, 2732, 4099]
    for loop in (one, three):
        loop.set_state(T(xs, dtype))
    for k in range(40):
        one.tick(DYN_UI, 0.0)
        three.tick(DYN_UI, 0.0)
        if k % 13 == 0 or k == 39:
            assert torch.equal(one.controls(), three.controls()), k
            assert torch.equal(one.iterations(), three.iterations()) and torch.equal(one.status(), three.status()), k
            assert torch.equal(one.state(), three.state()), k
    assert one.iterations().float().mean().item() > 1.0   # still in the transient: the ranges were not trivially idle


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_set_state_and_new_set_points_mid_run_with_column_ranges(pkg, dtype):
    """ClosedLoop.set_state() after the first tick (a disturbance, a reset) and a per-problem set-point tensor
    rewritten between ticks -- both prepared on the CALLER's stream, by a long chain of small kernels so that a range's
    stream which did not wait would read them too early -- give with three ranges bit for bit what one range gives."""
    rng = np.random.default_rng(21)
    B = 4099
    xs = np.stack([rng.uniform(-0.3, 0.3, B), np.pi / 2 + rng.uniform(-0.4, 0.4, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-1, 1, B)])
    loops = [pkg.ClosedLoop(pkg.default_params(), B, dtype=dtype, device=0, ranges=n) for n in (1, 3)]
    x0 = T(xs, dtype)
    sp = torch.zeros(B, dtype=dtype, device=x0.device)
    for loop in loops:
        loop.set_state(x0)
    for k in range(24):
        if k in (7, 15):
            # the disturbance: built by 200 dependent kernels on the caller's stream, handed over without a synchronize;
            # its source tensor is dropped at once (the allocator may reuse it as soon as the streams it was recorded on allow)
            for loop in loops:
                kick = loop.state().clone()
                for _ in range(200):
                    kick[3] += 0.002
                kick[1] -= 0.05
                if k == 15:   # a state one column too wide is refused whole; what follows shows that it left nothing behind
                    with pytest.raises(ValueError):
                        loop.set_state(torch.cat([kick, kick[:, :1]], dim=1))
                loop.set_state(kick)
                del kick
        if k >= 10:
            for _ in range(100):
                sp += 0.0002 * (1 if k % 2 else -1)
            sp_k = sp + 0.01 * torch.sin(torch.arange(B, dtype=dtype, device=sp.device))
        else:
            sp_k = 0.0
        for loop in loops:
            loop.tick(DYN_UI, sp_k)
        if k in (7, 8, 15, 16, 23):
            one, three = loops
            assert torch.equal(one.state(), three.state()), k
            assert torch.equal(one.controls(), three.controls()), k
            assert torch.equal(one.iterations(), three.iterations()) and torch.equal(one.status(), three.status()), k
    with pytest.raises(TypeError):
        loops[1].tick(torch.zeros((9, B), dtype=dtype, device=x0.device), 0.0)
    for loop in loops:
        loop.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_set_state_checks_the_whole_state_before_it_touches_a_range(pkg, dtype):
    """ClosedLoop.set_state() validates once, before anything is touched: after one tick a [4, B + 1] tensor (until now
    accepted, its last column dropped), a [4, B - 1] tensor (until now refused only after the first ranges had been
    replaced), a tensor of the other dtype and a CPU tensor are each refused, and state() is bitwise what it was -- with
    one range and with three (B = 130: 43 / 43 / 44 columns).  The valid call that follows, and two ticks, give the same
    bits in both."""
    rng = np.random.default_rng(33)
    B = 130
    xs = np.stack([rng.uniform(-0.3, 0.3, B), np.pi / 2 + rng.uniform(-0.4, 0.4, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-1, 1, B)])
    loops = [pkg.ClosedLoop(pkg.default_params(), B, dtype=dtype, device=0, ranges=n) for n in (1, 3)]
    assert loops[1].bounds == [0, 43, 86, 130]
    other = torch.float32 if dtype == torch.float64 else torch.float64
    x1 = T(xs, dtype)
    x2 = T(xs[:, ::-1], dtype)
    wide, narrow = torch.cat([x2, x2[:, :1]], dim=1), x2[:, :B - 1].contiguous()
    assert tuple(wide.shape) == (4, 131) and tuple(narrow.shape) == (4, 129)
    for loop in loops:
        loop.set_state(x1)
        loop.tick(DYN_UI, 0.0)
        before = loop.state().clone()
        for bad, exc in ((wide, ValueError), (narrow, ValueError), (x2.to(other), TypeError), (x2.cpu(), TypeError)):
            with pytest.raises(exc):
                loop.set_state(bad)
            assert torch.equal(loop.state(), before), (tuple(bad.shape), bad.dtype, bad.device)
        loop.set_state(x2)
        assert torch.equal(loop.state(), x2)
        for _ in range(2):
            loop.tick(DYN_UI, 0.0)
    one, three = loops
    assert torch.equal(one.state(), three.state()) and torch.equal(one.controls(), three.controls())
    assert not torch.equal(one.state(), x2)
    for loop in loops:
        loop.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_simulator_set_state_on_a_side_stream_is_set_state_on_the_current_one(pkg, dtype):
    """BatchSimulator.set_state(x, stream=s) and a step on s leave bitwise what set_state(x) and a step on the current
    stream leave (B = 65: more than one wave, not a multiple of it)."""
    rng = np.random.default_rng(34)
    B = 65
    x = T(random_states(rng, B), dtype)
    u = T(rng.uniform(-50, 50, B), dtype)
    here = pkg.BatchSimulator(B, dtype=dtype, device=0)
    here.set_state(x)
    here.step(DYN_UI, 0.01, u)
    there = pkg.BatchSimulator(B, dtype=dtype, device=0)
    side = torch.cuda.Stream(device=x.device)
    side.wait_stream(torch.cuda.current_stream(x.device))   # x, u and the simulator's initial state were written here
    there.set_state(x, stream=side)
    with torch.cuda.stream(side):
        there.step(DYN_UI, 0.01, u)
    u.record_stream(side)
    torch.cuda.current_stream(x.device).wait_stream(side)
    assert torch.equal(there.get_state(), here.get_state())
    assert not torch.equal(here.get_state(), x)
    with pytest.raises(ValueError):
        there.set_state(x[:, :B - 1], stream=side)


def test_plain_sqp_tool_reports_both_phases_in_both_dtypes():
    """tools/plain_sqp.py (bench.py variants.plain_sqp runs it in child processes) at unit-test size: the specification as
    shipped against the iteration without the full-step rule and the exit floor (the -DCPMPC_SKIP_MERIT=0 library is the
    third switch; here the product library serves both runs).  Settled float controllers: fewer iterations per tick with the
    floor than without; no solver failure anywhere."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    tool = os.path.join(ROOT, "tools", "plain_sqp.py")
    env = {k: v for k, v in os.environ.items() if k != "CPMPC_LIB"}
    res = {}
    for name, extra in (("defaults", []), ("plain", ["--full-step-below", "0", "--exit-defect-floor", "0"])):
        r = subprocess.run([sys.executable, tool, "--batch", "4096", "--ticks", "260", "--settled", "20"] + extra, env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    for name, d in res.items():
        for dt in ("f32", "f64"):
            for phase in ("soak", "settled"):
                assert d[dt][phase]["solver_failures"] == 0, (name, dt, phase)
            assert d[dt]["settled"]["pole_error_median"] < 1e-4   # (2.8 s after a start from anywhere: upright, still settling)
    assert res["defaults"]["exit_defect_floor"] == 2.0 and res["plain"]["exit_defect_floor"] == 0.0
    assert res["defaults"]["f32"]["settled"]["iterations_per_tick"] + 0.5 < res["plain"]["f32"]["settled"]["iterations_per_tick"]
    assert abs(res["defaults"]["f64"]["settled"]["iterations_per_tick"] - res["plain"]["f64"]["settled"]["iterations_per_tick"]) < 0.1


def test_wide_qp_float_handles_end_where_a_float_solve_can(pkg, orc):
    """CPMPC_CREATE_WIDE_QP: float kernels that carry the whole terminal part of the QP in double.  8 192 of the benchmark's
    cold starts, 5 iterations, against the double CPU check (max |du| per problem): the default float handle ends at median
    ~2.5e-4 with ~93 % of the problems within 1e-2; the wide one at <= 1.3e-4 with >= 98.5 % (measured 8.4e-5, 99.5 %) -- the
    level of the float build of the CPU check (8.0e-5, 99.3 %), which is held to the same bar here.  Same termination states;
    the option is ignored by double handles and by the 6-state model; exits and warm starts work as in any handle."""
    rng = np.random.default_rng(1000)
    B = 8192
    x0 = random_states(rng, B)
    over = dict(max_iterations=5, relative_exit_tol=0.0, absolute_first_derivative_tol=0.0)
    u64, _, st64, _, _ = orc.step_batch_cold(orc.default_opt_params(**over), DYN_UI, 0.0, x0)
    got = {}
    for wide in (False, True):
        opt = pkg.BatchOptimization(pkg.default_params(**over), max_batch=B, dtype=torch.float32, device=0, wide_qp=wide)
        assert opt.wide_qp == wide and opt.pipeline() == "fused"
        o = opt.step(T(x0, torch.float32), DYN_UI, 0.0)
        err = np.abs(o.u.double().cpu().numpy() - u64).max(axis=0)
        assert (o.status.cpu().numpy() == st64).all()
        got[wide] = (float(np.median(err)), float((err < 1e-2).mean()), float(np.quantile(err, 0.99)))
        # per-problem parameters take the same kernels (the constants are then reduced on the device in float instead of on the
        # host in double: another rounding of them, the same accuracy against the double check)
        dyn = T(np.tile(np.array(DYN_UI)[:, None], (1, B)), torch.float32)
        opt.reset()
        o2 = opt.step(T(x0, torch.float32), dyn, 0.0)
        err2 = np.abs(o2.u.double().cpu().numpy() - u64).max(axis=0)
        assert (o2.status.cpu().numpy() == st64).all() and np.median(err2) < 2.0 * np.median(err) + 1e-5
    u32, st32, _, _, _ = orc.step_batch_cold_f32(orc.default_opt_params(**over), DYN_UI, 0.0, x0)
    e32 = np.abs(u32 - u64).max(axis=0)
    print("default float: median %.2e within 1e-2 %.4f p99 %.2e | wide: %.2e %.4f %.2e | float CPU check: %.2e %.4f %.2e"
          % (got[False] + got[True] + (np.median(e32), (e32 < 1e-2).mean(), np.quantile(e32, 0.99))))
    assert got[True][0] <= 1.3e-4 and got[True][1] >= 0.985 and got[True][2] < 0.02
    assert np.median(e32) <= 1.3e-4 and (e32 < 1e-2).mean() >= 0.985
    assert got[False][0] > 1.5 * got[True][0] and got[False][2] > 5 * got[True][2]
    # ignored where it does not apply
    assert not pkg.BatchOptimization(pkg.default_params(**over), max_batch=64, dtype=torch.float64, device=0, wide_qp=True).wide_qp
    mk = lambda **kw: pkg.BatchOptimization(pkg.default_params(**over), max_batch=64, dtype=torch.float32, device=0, **kw)  # noqa: E731
    assert not mk().wide_qp and mk(model="double").wide_qp and not mk(model="double", wide_qp=False).wide_qp   # the defaults
    # a spacing served by the run-time-spacing kernel (N = 30, spacing 6) has it too; so does the split pipeline (round 6)
    over6 = dict(over, window_length=30, state_spacing=6)
    u6, _, st6, _, _ = orc.step_batch_cold(orc.default_opt_params(**over6), DYN_UI, 0.0, x0[:, :2048])
    e6 = {}
    for wide in (False, True):
        o6 = pkg.BatchOptimization(pkg.default_params(**over6), max_batch=2048, dtype=torch.float32, device=0, wide_qp=wide)
        assert o6.wide_qp == wide and o6.pipeline() == "fused"
        r6 = o6.step(T(x0[:, :2048], torch.float32), DYN_UI, 0.0)
        assert (r6.status.cpu().numpy() == st6).all()
        e6[wide] = float(np.median(np.abs(r6.u.double().cpu().numpy() - u6).max(axis=0)))
        if wide:
            o6.set_pipeline("split")
            assert o6.wide_qp
    assert e6[True] < 0.6 * e6[False], e6
    # closed loop with exits: no solver failure, poles stand
    loop = pkg.BatchOptimization(pkg.default_params(), max_batch=2048, dtype=torch.float32, device=0, wide_qp=True)
    sim = pkg.BatchSimulator(2048, dtype=torch.float32, device=0)
    sim.set_state(T(random_states(np.random.default_rng(3), 2048), torch.float32))
    bad = 0
    for k in range(300):
        r = loop.step(sim.get_state(), DYN_UI, 0.0, want_predicted=False)
        sim.step(DYN_UI, 0.01, r.u[0].contiguous())
        bad += int(((r.status == orc.TERM_QP_INDEFINITE) | (r.status == orc.TERM_MAX_LAMBDA) | (r.status == orc.TERM_NON_FINITE)).sum().item())
    assert bad == 0
    assert ((sim.get_state()[1].double() - np.pi / 2).abs() < 1e-3).float().mean().item() > 0.9
