"""The staged fused SQP pipeline where a problem is restarted from the workspace more than once, bit for bit.

With exit tolerances on, a step is several launches of fused_sqp_kernel with compact_active_kernel in between, and "results are
bitwise those of one launch" (DESIGN.md section 5b).  A later launch whose list holds at most run_out_below = 2048 * (64 // L)
problems runs them to the end, so at the batch sizes of the other staged tests a problem is saved and reloaded once and every
compaction after the first finds an empty list.  Here B = 2 * run_out_below + 77: the lists stay longer than one round of
resident waves through several cuts, the three rotating counters each have a non-empty list behind them, the second finishing
rule is reached before the first, the riding lanes of L = 10 and L = 5 and the clamp of the list's last entry work on lists
that are thousands of waves long, and every fused instantiation (SHARED, per-problem, WIDE, plain and REFINE, both models, the
run-time-spacing kernel) takes part.  The same for the chunked host-pointer step with exits on: chunks at col0 != 0 compacting
into their own range of the list, three slots' counters in flight.

The reference of every comparison is the same handle class with set_compaction(0, 0): one launch.  That launch is held to the
CPU checks by the parity files; here nothing is compared with a tolerance -- u, predicted_states, status, iterations, ls_evals,
final_cost, final_eq_l1, guess and get_solution() of a cold step and two warm ticks through BatchSimulator are compared on
their bit patterns, in float32 as well.

Every case first asserts, from the REFERENCE run through tests/helpers/stage_model.py (the launch rules restated on the
host), that its inputs do exercise the machinery -- before it reads a staged result:
  (a) on the cold step and on at least one warm tick the plan 1 + 1 at max_iterations = 12 has at least four launches whose
      lists exceed run_out_below: some problem is reloaded at least three times;
  (b) over the three ticks at least three compactions that feed a working launch each remove at least 1 % of their list;
  (c) at max_iterations = 8, plan 1 + 1, rule 2 finishes a launch, and for an earlier list of the same step neither rule holds;
  (d) no problem ends NON_FINITE in any tick (the model counts on it, and a NaN would make the comparison empty).

Reached on an MI355X, from the single-launch runs (forms with the same figures share a line):
  case                                      lists > run_out_below   most reloads of one    compactions   rule 2 at cap 8
                                            per tick (plan 1 + 1)   problem, per tick      >= 1 %        fires in ticks
  4-state 40/4  f32 shared, per-problem     10, 7, 6                9, 7, 6                14            cold
  4-state 40/4  f32 wide, f64 plain/refine  12, 6, 6                11, 6, 6               15            cold
  4-state 80/5  f32 shared, per-problem     11, 5, 5                11, 5, 5               12, 13        cold
  4-state 80/5  f32 wide, f64 plain/refine  10, 4, 4                10, 4, 4               10            cold
  4-state 40/8  f64 plain, f32 wide         10, 6, 6                9, 6, 6                14            cold
  6-state 40/5  f32 shared                  10, 10, 10              9, 9, 9                5             all three
  6-state 40/5  f32 per-problem             10, 10, 10              9, 9, 9                12            all three
  6-state 40/5  f32 wide, f64 plain/refine  10, 10, 10              9, 9, 9                17            all three
  6-state 40/8  f64 plain, f32 wide         10, 10, 10              9, 9, 9                15            all three
The share of the batch still listed after 1, 2, ... iterations, 4-state 40/4 double: cold 1.0 1.0 1.0 0.996 0.975 0.945 0.887
0.809 0.722 0.645 0.578, first warm tick 1.0 0.991 0.948 0.894 0.688 0.428 (then rule 1), second 1.0 0.991 0.944 0.875 0.558 0.311;
6-state 40/8 double: cold 0.996 0.987 0.977 0.970 0.964 0.957 0.950 0.940 0.931 (rule 2 finishes at 9), warm 0.999 0.989 0.968
0.948 0.930 0.919 0.914 0.909 0.904.  The warm 4-state ticks lose more than half their problems between iterations 4 and 6, so
a 4-state case has its four long lists there and no more; no input needed another seed or another share of upright starts.
Host-pointer test: the library equalises its chunks, so "chunk 13 000" of 24 653 problems is 12 352 + 12 301 (64 problems above
run_out_below = 12 288) and the chunks of 27 077 are 13 568 + 13 509; lists and launch counts in that test's docstring.
Times (pytest --durations=0, setup + call + teardown): the 27 cases sum to 2.0 s inside the whole GPU suite and to 2.6 s when the
file runs alone (the first case then loads the library, 0.6 s), slowest case 0.16 s; the file alone is 4.9 s of wall time, the
rest being interpreter start and imports.  A step at these B is milliseconds.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import DYN_UI
from helpers import batch_position as bp
from helpers import stage_model as sm
from test_gpu_position_independence import FORMS, MODELS, _terminal_defaults

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
TICKS = 3
STEP_FIELDS = ("u", "predicted_states", "status", "iterations", "ls_evals", "final_cost", "final_eq_l1", "guess")
# all five forms at three shapes, float64 plain and float32 WIDE at the two largest batches
ALL, TWO = tuple(FORMS), ("f64-plain", "f32-wide")
CASES = [(s, f) for s, forms in zip(sm.SHAPES, (ALL, ALL, TWO, ALL, TWO)) for f in forms]
PLANS_12 = ((1, 1), (2, 1), (1, 3))
AUTO = {(("single", 40, 4), "f64-plain"), (("single", 40, 4), "f32-shared")}

_INPUTS = {}


def _inputs(pkg, model, B, seed):
    """x0 and the per-problem dyn, set_point, terminal_weights of a shape: drawn once, float64, on the host, never modified."""
    if (model, B, seed) not in _INPUTS:
        m = MODELS[model]
        rng = np.random.default_rng(seed + 100)
        dyn = np.array(m["dyn"]).reshape(-1, 1) * rng.uniform(0.8, 1.2, (len(m["dyn"]), B))
        sp = rng.uniform(-0.2, 0.2, B)
        tw = _terminal_defaults(pkg.default_params(), m["nx"]).reshape(-1, 1) * rng.uniform(0.5, 2.0, (m["nx"], B))
        _INPUTS[model, B, seed] = dict(x0=torch.tensor(sm.cold_states(model, B, seed)), dyn=torch.tensor(dyn),
                                       set_point=torch.tensor(sp), terminal_weights=torch.tensor(tw))
    return _INPUTS[model, B, seed]


def _run(pkg, shape, form, cap, compaction):
    """A cold step and two warm ticks of a fresh handle and a fresh plant; compaction None: the default plan.
    -> ([{output: tensor}] per tick, [stage_plan()] per tick, launches of fused_sqp_kernel counted by the profile)."""
    model, N, sp = shape
    dtype, per_problem, wide, refine = FORMS[form]
    B = sm.batch_of(N // sp)
    inp = _inputs(pkg, model, B, sm.X0_SEED[model])
    kw = dict(dyn=MODELS[model]["dyn"], set_point=0.0, terminal_weights=None)
    if per_problem:
        kw = {k: inp[k].to(dtype).to(DEV) for k in kw}
    opt = pkg.BatchOptimization(pkg.default_params(window_length=N, state_spacing=sp, max_iterations=cap), max_batch=B, dtype=dtype,
                                device=0, model=model, wide_qp=wide, refine_qp=refine)
    opt.set_pipeline("fused")
    assert opt.pipeline() == "fused"
    if wide is not None:
        assert opt.wide_qp == wide
    if refine is not None:
        assert opt.refines_qp == refine
    if compaction is not None:
        opt.set_compaction(*compaction)
    opt.profile_enable(True)
    opt.profile_reset()
    sim = pkg.BatchSimulator(B, dtype=dtype, device=0, model=model)
    sim.set_state(inp["x0"].to(dtype).to(DEV))
    res, plans = [], []
    for _ in range(TICKS):
        o = opt.step(sim.get_state(), kw["dyn"], kw["set_point"], want_predicted=True, want_stats=True, want_guess=True,
                     out=pkg.BatchOutputs(), terminal_weights=kw["terminal_weights"])
        r = {f: getattr(o, f) for f in STEP_FIELDS}
        r["solution"] = opt.get_solution(B)
        plans.append(opt.stage_plan())
        torch.cuda.synchronize()          # the controller acts on u (and the default plan reads this tick's histogram)
        sim.step(kw["dyn"], 0.01, o.u[0].contiguous())
        res.append(r)
    launches = opt.profile_read()["fused_sqp_kernel"][1]
    torch.cuda.synchronize()
    opt.close()
    return res, plans, launches


def _model_of(pkg, tick, first, nxt, L, cap):
    its, st = tick["iterations"].cpu().numpy(), tick["status"].cpu().numpy()
    return sm.working_stages(its, st == pkg.capi.TERM["MAX_ITERATIONS"], sm.plan_bounds(first, nxt, cap), L, cap)


def _assert_conditions(pkg, ref12, ref8, L, what):
    """(a) - (d) of the file's docstring from the single-launch runs; prints what the case reaches."""
    for ref in (ref12, ref8):
        for tick in ref:
            st = tick["status"].cpu().numpy()
            assert (st != pkg.capi.TERM["NON_FINITE"]).all() and (st != pkg.capi.TERM["NONE"]).all(), (what, np.bincount(st))   # (d)
            for name, t in tick.items():
                assert bool(torch.isfinite(t).all()) if t.is_floating_point() else True, (what, name)
    beyond, reloads, removed, lists = [], [], 0, []
    for tick in ref12:
        launches, active_in = _model_of(pkg, tick, 1, 1, L, 12)
        beyond.append(sm.lists_beyond_run_out(launches, L))
        reloads.append(int(active_in.max()) - 1)
        removed += sum(s >= 0.01 for s in sm.removed_shares(launches))
        lists.append([l.n_list for l in launches if l.n_list])
    rule2 = [sm.rule2_fires_after_not_firing(_model_of(pkg, tick, 1, 1, L, 8)[0]) for tick in ref8]
    print("%s: run_out_below %d; lists beyond it per tick %s, most reloads of a problem per tick %s, compactions removing >= 1 %%: "
          "%d, rule 2 at cap 8 per tick %s\n    lists 1 + 1 at cap 12: %s" % (what, sm.run_out_below(L), beyond, reloads, removed,
                                                                             rule2, lists))
    ok = [b >= 4 and r >= 3 for b, r in zip(beyond, reloads)]
    assert ok[0] and any(ok[1:]), (what, "(a)", beyond, reloads)
    assert removed >= 3, (what, "(b)", lists)
    assert any(rule2), (what, "(c)", rule2)


def _assert_same_bits(pkg, ref, got, L, cap, plans, what):
    """plans: the stage plan of every tick (for the message: how often the first differing problem was reloaded)."""
    assert len(ref) == len(got) == TICKS
    for tick, (want, have) in enumerate(zip(ref, got)):
        assert list(want) == list(have)
        for name in want:
            msg = bp.first_difference(want[name], have[name], L, name="%s, tick %d, %s" % (what, tick, name))
            if msg is not None:
                p = int(torch.nonzero((bp._bits(want[name]) != bp._bits(have[name])).reshape(-1, want[name].shape[-1]).any(dim=0))[0, 0])
                launches, active_in = sm.working_stages(want["iterations"].cpu().numpy(),
                                                        want["status"].cpu().numpy() == pkg.capi.TERM["MAX_ITERATIONS"], plans[tick], L, cap)
                msg += "; the problem ran %d iterations and was reloaded %d times (lists %s)" % (
                    int(want["iterations"][p]), int(active_in[p]) - 1, [l.n_list for l in launches])
            assert msg is None, msg


@pytest.mark.parametrize("shape,form", CASES, ids=["%s-%dx%d-%s" % (s + (f,)) for s, f in CASES])
def test_staged_restarts_are_bitwise_the_single_launch(pkg, shape, form):
    """One (shape, form): the single launch at max_iterations 12 and 8, conditions (a) - (d) from it, then the plans 1 + 1,
    2 + 1, 1 + 3 of 12 and 1 + 1 of 8 -- each on a fresh handle and plant, three ticks, every output bit for bit, the profile's
    launch count that of the plan -- and for two forms the default plan (measured: 11 launches cold, then e.g. [0, 7, 9, 10, 12]
    and [0, 4, 5, 6, 7, 12] from the histogram of the tick before)."""
    model, N, sp = shape
    L = N // sp
    what = "%s %d/%d %s, B = %d" % (model, N, sp, form, sm.batch_of(L))
    ref12, plans, launches = _run(pkg, shape, form, 12, (0, 0))
    assert plans == [[0, 12]] * TICKS and launches == TICKS
    ref8, plans, launches = _run(pkg, shape, form, 8, (0, 0))
    assert plans == [[0, 8]] * TICKS and launches == TICKS
    _assert_conditions(pkg, ref12, ref8, L, what)
    for cap, ref, compactions in ((12, ref12, PLANS_12), (8, ref8, ((1, 1),))):
        for first, nxt in compactions:
            bounds = sm.plan_bounds(first, nxt, cap)
            got, plans, launches = _run(pkg, shape, form, cap, (first, nxt))
            assert plans == [bounds] * TICKS and launches == TICKS * (len(bounds) - 1), (plans, launches)
            _assert_same_bits(pkg, ref, got, L, cap, plans, "%s, staged %d + %d of %d" % (what, first, nxt, cap))
    if (shape, form) in AUTO:
        got, plans, launches = _run(pkg, shape, form, 12, None)
        for plan in plans:
            assert plan[0] == 0 and plan[-1] == 12 and all(b > a for a, b in zip(plan, plan[1:])), plan
        assert plans[0] == [0, 2] + list(range(3, 13))             # nothing to plan from yet: 2, then 1 at a time
        assert launches == sum(len(plan) - 1 for plan in plans), (plans, launches)
        print("%s: default plans %s" % (what, plans))
        _assert_same_bits(pkg, ref12, got, L, 12, plans, "%s, default plans" % what)


# ---- the chunked host-pointer step with exits on ---------------------------------------------------------------------------
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int32)


def _dp(a):
    return a.ctypes.data_as(DP)


HOST_CAP, HOST_L = 8, 10
# B -> [(cpmpc_set_host_chunk, compaction or None = the default plan)].  The library equalises the chunks (helpers/stage_model.py:
# host_chunks): "13 000" of 24 653 problems are chunks of 12 352 and 12 301, which the default plan leaves in one launch each
# (1 930 waves; it stages beyond 2 048), and no split of 24 653 in two can do better -- so a batch of 27 077 = 2 * 13 500 + 77
# stands beside it, whose chunks of 13 568 and 13 509 (2 120 and 2 111 waves) the default plan does stage.
HOST_ARRANGEMENTS = {sm.batch_of(HOST_L): [(2048, (1, 1)), (13000, (1, 1)), (13000, None)],
                     27077: [(14000, (1, 1)), (14000, None)]}


@pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "per-problem"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", sorted(HOST_ARRANGEMENTS))
def test_chunked_host_step_with_exits_is_bitwise_the_unsplit_single_launch(pkg, B, dtype, per_problem):
    """cpmpc_step_batch_host_in with the default exit tolerances, 4-state 40/4, max_iterations 8: chunks that are staged
    themselves, against the unsplit handle with one launch -- u, predicted, solution, status, iterations, cost and eq of a
    cold and a warm tick, bit for bit.
    B = 24 653: chunk 2 048 with the plan 1 + 1 (thirteen chunks of 1 920 through the three slots: one restart each, col0 != 0,
    the counters of three slots in flight); chunk 13 000 with 1 + 1 (two chunks, 12 352 and 12 301: the first one's lists stay
    above run_out_below = 12 288 through four launches while the second, at col0 = 12 352 in another slot, compacts into its
    own range of the list); chunk 13 000 with the default plan (neither chunk is staged: the plain chunk pipeline).
    B = 27 077: chunk 14 000 (13 568 and 13 509) with 1 + 1 and with the default plan, which stages both chunks: 2 + 1 + 1 + ...
    on the cold tick, from each slot's own histogram on the warm one.
    Before a chunked result is read, condition (a) is asserted from the reference's counts for the first chunk of every
    two-chunk arrangement, on the cold AND on the warm tick (at least four launches with a list beyond run_out_below, a problem
    reloaded at least three times inside the chunk), and the profile's count of fused launches for every arrangement.
    Measured (double, shared; the other three within 110 problems): first chunk of 12 352, cold, lists 12 352, 12 352, 12 350, 12 349, 12 307, 12 016 (four launches beyond 12 288, then rule 1; five reloads),
    warm 12 352, 12 350, 12 342, 12 322, 12 074 (four beyond, four reloads); first chunk of 13 568, cold 13 568, 13 566, 13 565, 13 563, 13 507, 13 178 (rule 2 at iteration 5), warm 13 568, 13 566, 13 560, 13 533, 13 254, 12 889.  Default plan at 27 077: 14 launches cold (7 per chunk), 4 warm in double
    and 2 in float (the planner then leaves each chunk in one launch)."""
    lib = pkg.capi.load()
    cdt = pkg.capi.F64 if dtype == "f64" else pkg.capi.F32
    N, spacing, cap, L = 40, 4, HOST_CAP, HOST_L
    inp = _inputs(pkg, "single", B, sm.X0_SEED["single"])
    x0 = inp["x0"].numpy()
    dyn_pp, sp, tw = inp["dyn"].numpy(), inp["set_point"].numpy(), inp["terminal_weights"].numpy()
    dyn_shared = (C.c_double * 9)(*DYN_UI)
    params = pkg.default_params(window_length=N, state_spacing=spacing, max_iterations=cap)
    handles = {}

    def make(name, chunk, compaction):
        h = C.c_void_p()
        pkg.capi.check(lib.cpmpc_create(C.byref(params), None, cdt, B, 0, C.byref(h)))
        handles[name] = h
        pkg.capi.check(lib.cpmpc_set_host_chunk(h, chunk))
        if compaction is not None:
            pkg.capi.check(lib.cpmpc_set_compaction(h, *compaction))
        pkg.capi.check(lib.cpmpc_profile_enable(h, 1))
        return h

    def run(h, x):
        dim = lib.cpmpc_dim(h)
        b = dict(u=np.zeros((N, B)), pred=np.zeros((N, 4, B)), st=np.zeros(B, np.int32), it=np.zeros(B, np.int32),
                 cost=np.zeros(B), eq=np.zeros(B), z=np.zeros((dim, B)))
        i = pkg.capi.StepHostInputs(x0=_dp(x), dyn_shared=None if per_problem else dyn_shared,
                                    dyn=_dp(dyn_pp) if per_problem else None, set_point_shared=0.05,
                                    set_point=_dp(sp) if per_problem else None,
                                    terminal_weights=_dp(tw) if per_problem else None)
        o = pkg.capi.StepHostOutputs(u=_dp(b["u"]), predicted=_dp(b["pred"]), status=b["st"].ctypes.data_as(IP),
                                     iterations=b["it"].ctypes.data_as(IP), final_cost=_dp(b["cost"]),
                                     final_eq_l1=_dp(b["eq"]), solution=_dp(b["z"]))
        pkg.capi.check(lib.cpmpc_step_batch_host_in(h, B, C.byref(i), C.byref(o)))
        return b

    def fused_launches(h):
        ms, n = C.c_double(), C.c_int64()
        pkg.capi.check(lib.cpmpc_profile_read(h, pkg.capi.KERNEL_FUSED, C.byref(ms), C.byref(n)))
        pkg.capi.check(lib.cpmpc_profile_reset(h))
        return int(n.value)

    who = "host step B = %d %s %s" % (B, dtype, "per-problem" if per_problem else "shared")
    n11 = len(sm.plan_bounds(1, 1, cap)) - 1
    n21 = len(sm.plan_bounds(2, 1, cap)) - 1           # the default plan before there is a histogram: 2, then 1 at a time
    try:
        make("unsplit", 0, (0, 0))
        for chunk, compaction in HOST_ARRANGEMENTS[B]:
            make("chunk %d, %s" % (chunk, "default plan" if compaction is None else "%d + %d" % compaction), chunk, compaction)
        for tick, x in enumerate((x0, np.ascontiguousarray(x0 + 0.01))):     # cold, then warm from the handle's own solution
            ref = run(handles["unsplit"], x)
            assert fused_launches(handles["unsplit"]) == 1
            assert (ref["st"] != pkg.capi.TERM["NON_FINITE"]).all() and (ref["st"] != pkg.capi.TERM["NONE"]).all()
            assert all(np.isfinite(ref[k]).all() for k in ("u", "pred", "cost", "eq", "z"))
            for (chunk, compaction), name in zip(HOST_ARRANGEMENTS[B], list(handles)[1:]):
                chunks = sm.host_chunks(B, chunk)
                if compaction is not None:
                    want = len(chunks) * n11
                else:
                    staged = [sm.default_plan_stages(n, L) for _, n in chunks]
                    # cold: the fixed pattern; warm: one launch where the default does not stage, else the planner's choice
                    want = sum(n21 if st else 1 for st in staged) if tick == 0 or not any(staged) else None
                if len(chunks) == 2:                                         # condition (a) for the first chunk, cold and warm
                    first = chunks[0][1]
                    launches, active_in = sm.working_stages(ref["it"][:first], ref["st"][:first] == pkg.capi.TERM["MAX_ITERATIONS"],
                                                            sm.plan_bounds(1, 1, cap), L, cap)
                    lists = [l.n_list for l in launches]
                    print("%s tick %d: first chunk of %d, plan 1 + 1: lists %s, most reloads %d" % (
                        who, tick, first, lists, int(active_in.max()) - 1))
                    assert sm.lists_beyond_run_out(launches, L) >= 4 and active_in.max() >= 4, (who, tick, first, lists)
                got = run(handles[name], x)
                n = fused_launches(handles[name])
                print("%s tick %d: %s: %d chunks, %d launches of fused_sqp_kernel" % (who, tick, name, len(chunks), n))
                assert n == want if want is not None else n >= len(chunks), (name, tick, n, want)
                for k in ref:
                    same = ref[k].view(np.int64 if ref[k].dtype == np.float64 else np.int32) == \
                        got[k].view(np.int64 if got[k].dtype == np.float64 else np.int32)
                    if not same.all():
                        p = int(np.nonzero(~same.reshape(-1, B).all(axis=0))[0][0])
                        raise AssertionError("%s, %s, tick %d, %s: problem %d differs (%d do; %d iterations)" % (
                            who, name, tick, k, p, int((~same.reshape(-1, B).all(axis=0)).sum()), int(ref["it"][p])))
    finally:
        for h in handles.values():
            lib.cpmpc_destroy(h)
