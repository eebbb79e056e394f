"""The 6-state model's SQP step against the oracle from the sides the 4-state one is held from (tests/test_gpu_parity.py):
terminal mixes, per-problem dyn / set_point / terminal_weights, weights that differ between the two poles, solver options,
reset and warm start, edge batches, a non-finite lane.  float64 only; the fused kernel, its REFINE form and the split pipeline.

What the terminal mix steers is code only the 6-state kernels have (csrc/mpc_fused_body.inc: the terminal system rebuilt in a
second pass, the cost flags as a bit mask, the structural zeros of Phi / Psi, the REFINE form that keeps one pass), and
test_gpu_double.py runs two mixes.  test_gpu_position_independence.py runs the per-problem inputs, but against a permutation
of the same run, with weights that never change a row between cost and equality.

THE CRITERION.  Some of these problems are rounding-sensitive in the reference itself (the double and the extended-precision
oracle end 1e-5 to 1e2 apart on a few lanes of the mixes with th a cost row and th_dot an equality), so the comparison is on
SETTLED lanes (tests/helpers/double_parity.py): there, the oracle's termination state and iteration count, u and
predicted_states within 1e-5, median |du| below 1e-7.  tests/test_double_parity_cases.py holds the share of settled lanes --
3/4 of every case, 95 % of every test -- from the two oracles alone, and every test here asserts it again before it looks at
the GPU's result.  On the other lanes: u finite, a legal status; their number, and how many of them the arbiter rule of
test_fuzz_with_the_extended_precision_arbiter would call the kernel's fault, are printed, not asserted.

WHAT IT FOUND.  The plain condensed QP of the 6-state kernels loses a digit and a half against the oracle's full-space solve
where the pole angles are cost rows and their rates equalities, and one settled lane ended 5e-5 from the oracle: such handles
now refine the QP by default (test_default_handles_refine_the_qp_where_angles_are_costs_and_their_rates_equalities)."""
import collections

import numpy as np
import pytest

from helpers import double_parity as dp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
TOL, MEDIAN_TOL, PIPELINES_TOL = 1e-5, 1e-7, 1e-6
# (pipeline, refine_qp): None = the handle's default
FORMS = {"fused": ("fused", None), "fused-refine": ("fused", True), "split": ("split", None),
         "fused-plain": ("fused", False), "split-plain": ("split", False)}


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


_TALLY = collections.defaultdict(list)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Per test, over its cases: lanes, settled, unsettled, arbiter faults, worst and median |du| on the settled lanes."""
    yield
    for name, rows in _TALLY.items():
        err = np.concatenate([r[3] for r in rows])
        print("\n[double parity] %-44s cases %3d lanes %5d settled %5d unsettled %4d arbiter faults %3d |du| worst %.2e median %.2e"
              % (name, len(rows), sum(r[0] for r in rows), sum(r[1] for r in rows), sum(r[0] - r[1] for r in rows),
                 sum(r[2] for r in rows), err.max(), np.median(err)), end="")
    print()


def _handle(pkg, over, form, max_batch, opts=None):
    """A float64 6-state handle on the pipeline of the form; skipped with the reason where the shape has no such pipeline
    (tests/test_gpu_parity.py::test_pipeline_selection)."""
    pipeline, refine = FORMS[form]
    opt = pkg.BatchOptimization(pkg.default_params(**over), max_batch=max_batch, dtype=torch.float64, device=0, model="double",
                                refine_qp=refine, opts=opts)
    try:
        opt.set_pipeline(pipeline)
    except pkg.CpmpcError as e:
        if e.code != pkg.capi.ERR_UNSUPPORTED:
            raise
        pytest.skip("no %s pipeline for N = %d, spacing %d: %s" % (pipeline, opt.N, opt.N // (opt.S - 1), e))
    assert opt.pipeline() == pipeline
    if refine is not None:
        assert opt.refines_qp == refine
    return opt


def _outputs(out):
    return {k: N_(getattr(out, k)) for k in ("u", "predicted_states", "status", "iterations", "ls_evals")}


def _hold(pkg, test, what, got, reference):
    """The criterion of this file for one GPU result `got` (_outputs) against reference = dp.settled(...)."""
    (u_c, pred_c, st_c, it_c), mask, dist, u_ld = reference
    u, st, it = got["u"], got["status"], got["iterations"]
    assert u.shape == u_c.shape and got["predicted_states"].shape == pred_c.shape
    legal = [v for k, v in pkg.capi.TERM.items() if k not in ("NONE", "USER_CALLBACK")]
    assert np.isfinite(u).all() and np.isin(st, legal).all(), what            # every lane, settled or not
    err = np.abs(u - u_c).max(axis=0)
    perr = np.abs(got["predicted_states"] - pred_c).max(axis=(0, 1))
    e_gpu = np.abs(u - u_ld).max(axis=0)
    faults = int((~mask & (e_gpu > TOL) & (e_gpu > 2.0 * dist)).sum())
    print("%s %s: settled %d of %d, unsettled %d (arbiter faults %d); settled |du| max %.2e median %.2e, pred max %.2e"
          % (test, what, mask.sum(), mask.size, (~mask).sum(), faults, err[mask].max(), np.median(err[mask]), perr[mask].max()))
    _TALLY[test].append((mask.size, int(mask.sum()), faults, err[mask]))
    assert (st[mask] == st_c[mask]).all() and (it[mask] == it_c[mask]).all(), (what, np.nonzero(mask & ((st != st_c) | (it != it_c)))[0])
    assert err[mask].max() < TOL and perr[mask].max() < TOL, (what, np.sort(err[mask])[-5:], np.sort(perr[mask])[-5:])
    assert np.median(err[mask]) < MEDIAN_TOL, (what, np.median(err[mask]))


def _hold_pipelines(a, b, mask, what):
    """Fused and split on settled lanes: the rule of test_gpu_parity.py::test_fused_with_groups_that_straddle_dpp_rows."""
    for k in ("status", "iterations", "ls_evals"):
        assert (a[k][mask] == b[k][mask]).all(), (what, k, np.nonzero(mask & (a[k] != b[k]))[0])
    assert np.abs(a["u"] - b["u"]).max(axis=0)[mask].max() < PIPELINES_TOL, what


# ---------------------------------------------------------------------------------------------------------------------------
# 1. terminal mixes
# ---------------------------------------------------------------------------------------------------------------------------
_GPU = {}


def _case_on_gpu(pkg, case, form):
    """The cold step of a case through a form, once per process."""
    if (case.id, form) not in _GPU:
        opt = _handle(pkg, case.over, form, dp.B)
        _GPU[case.id, form] = _outputs(opt.step(T(case.x0), dp.DYN, dp.SET_POINT))
        opt.close()
    return _GPU[case.id, form]


def _settled_case(orc, case, table):
    """The reference of a case; the two shares of its table are asserted here, from the oracles alone."""
    dp.assert_shares({c.id: c.reference(orc)[1] for c in table}, "table of " + case.id)
    return case.reference(orc)


def _refined_by_default(case):
    return case.pattern[1] == "+" and case.pattern[3] == "-"


def test_default_handles_refine_the_qp_where_angles_are_costs_and_their_rates_equalities(pkg):
    """What the first run of this file on an MI355X found.  With th a cost row and th_dot an equality the plain condensed solve
    is 7e-9 from the extended-precision answer after the first QP of a cold start, where the oracle is 2e-10 and the REFINE form
    7e-12; on lane 46 of 40/8 '++--', settled at 2.0e-8, four iterations carried that to 5.0e-5 (fused) / 4.2e-5 (split) from
    the oracle, 8.5e-6 from each other, and the REFINE form ended 9.4e-8 away.  Double 6-state handles with such rows therefore
    refine the QP by default (csrc/cpmpc_api.hip), in both pipelines; the 4-state model keeps its rule."""
    for c in dp.MIX_CASES:
        p = pkg.default_params(**c.over)
        want = _refined_by_default(c)
        assert pkg.BatchOptimization(p, max_batch=8, dtype=torch.float64, device=0, model="double").refines_qp == want, c.id
        assert not pkg.BatchOptimization(p, max_batch=8, dtype=torch.float64, device=0, model="double", refine_qp=False).refines_qp
        assert not pkg.BatchOptimization(p, max_batch=8, dtype=torch.float64, device=0).refines_qp


_MIX_RUNS = [pytest.param(c, f, id="%s-%s" % (c.id, f)) for c in dp.MIX_CASES
             for f in ("fused", "fused-refine", "split") + (("fused-plain", "split-plain") if _refined_by_default(c) else ())]


@pytest.mark.parametrize("case,form", _MIX_RUNS)
def test_terminal_mixes(pkg, orc, case, form):
    """All 16 cost / equality sign patterns of (b_x, th, b_x_dot, th_dot) at 40/10 through the fused kernel, its REFINE form
    and the split pipeline.  'fused' and 'split' are the handle's default: the plain kernels, and the refining ones for the
    four patterns of the test above -- which run through the plain kernels as well ('-plain': refine_qp=False), so that the
    code the mix steers in them stays held at this shape (there: worst settled lane 1.4e-6, medians 6e-10 to 1.4e-9)."""
    ref = _settled_case(orc, case, dp.MIX_CASES)
    _hold(pkg, "test_terminal_mixes", "%s %s" % (case.id, form), _case_on_gpu(pkg, case, form), ref)


@pytest.mark.parametrize("form", ["fused", "split"])
@pytest.mark.parametrize("case", dp.SHAPE_CASES, ids=lambda c: c.id)
def test_terminal_mixes_across_shapes(pkg, orc, case, form):
    """All cost rows, all equalities, the default and th a cost row with th_dot an equality at 40/5, 20/10, 20/5, 40/8 and the
    run-time-spacing 30/6 (less the cases helpers/double_parity.py lists as dropped, with the reason)."""
    ref = _settled_case(orc, case, dp.SHAPE_CASES)
    _hold(pkg, "test_terminal_mixes_across_shapes", "%s %s" % (case.id, form), _case_on_gpu(pkg, case, form), ref)


@pytest.mark.parametrize("case", dp.MIX_CASES + dp.SHAPE_CASES, ids=lambda c: c.id)
def test_terminal_mixes_fused_and_split_agree(pkg, orc, case):
    mask = case.reference(orc)[1]
    assert mask.mean() >= dp.MIN_CASE_SHARE
    _hold_pipelines(_case_on_gpu(pkg, case, "fused"), _case_on_gpu(pkg, case, "split"), mask, case.id)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. per-problem inputs, lane by lane against an oracle built for that lane
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["fused", "split"])
@pytest.mark.parametrize("rows", ["default", "soft"])
def test_per_problem_dyn_and_set_points(pkg, orc, rows, pipeline):
    """DoubleCartPoleParams [6, B] (the first five times uniform(0.8, 1.25)) and set-points [B] in +-0.1, with the default
    terminal rows (40/10) and with all six rows costs (SOFT, 40/5): every lane against its own oracle."""
    x0, dyn, sp, _ = dp.per_problem_inputs()
    over = dp.PP_OVER[rows]
    ref = dp.settled(orc, over, dyn, sp, x0)
    dp.assert_shares({rows: ref[1]}, "per-problem dyn and set_point")
    opt = _handle(pkg, over, pipeline, dp.B)
    got = _outputs(opt.step(T(x0), T(dyn), T(sp)))
    _hold(pkg, "test_per_problem_dyn_and_set_points", "%s %s" % (rows, pipeline), got, ref)
    # the inputs did matter: the shared-parameter run of the same states is another result on every lane
    shared = _outputs(_handle(pkg, over, pipeline, dp.B).step(T(x0), dp.DYN, dp.SET_POINT))
    assert (np.abs(shared["u"] - got["u"]).max(axis=0) > 1e-3).all()


_PP_GPU = {}


@pytest.mark.parametrize("pipeline", ["fused", "split"])
def test_per_problem_terminal_weights(pkg, orc, pipeline):
    """Every problem with its own terminal rows [6, B]: magnitudes 10 ** uniform(0, 2.3), each of the four weight classes an
    equality with probability 1/2 (all 16 mixes occur), the two poles sharing their weights so that the oracle's
    OptimizationParams of that lane can say the same.  And the handle's own weights given per problem reproduce the shared path
    bit for bit."""
    tw, x0 = dp.per_problem_inputs()[3], dp.x0_of(dp.PP_SEED, spread=dp.PP_WEIGHTS_SPREAD)
    over = dp.PP_OVER["default"]
    ref = dp.settled(orc, over, dp.DYN, dp.SET_POINT, x0, terminal_weights=tw)
    dp.assert_shares({"terminal_weights": ref[1]}, "per-problem terminal weights")
    opt = _handle(pkg, over, pipeline, dp.B)
    got = _outputs(opt.step(T(x0), dp.DYN, dp.SET_POINT, terminal_weights=T(tw)))
    _PP_GPU[pipeline] = got
    _hold(pkg, "test_per_problem_terminal_weights", pipeline, got, ref)
    if len(_PP_GPU) == 2:
        _hold_pipelines(_PP_GPU["fused"], _PP_GPU["split"], ref[1], "per-problem terminal weights")
    p = pkg.default_params(**over)
    own = np.tile(dp.rows_of([getattr(p, n) for n in dp.NAMES]).reshape(6, 1), (1, dp.B))
    opt.reset()
    a = opt.step(T(x0), dp.DYN, dp.SET_POINT, terminal_weights=T(own)).u.clone()
    opt.reset()
    b = opt.step(T(x0), dp.DYN, dp.SET_POINT).u
    assert torch.equal(a, b)
    assert not torch.equal(b, T(got["u"]))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. weights that differ between the two poles
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["fused", "split"])
def test_terminal_rows_that_differ_between_the_poles(pkg, orc, pipeline):
    """th1 a cost row with th2 an equality on half of the lanes and the reverse on the rest, th1_dot / th2_dot likewise in
    blocks of two lanes (four mixes, b_x and b_x_dot cost rows): the one place a mix-up of rows 1 / 2 or 4 / 5 when the
    per-problem weights are loaded shows.  OptimizationParams cannot say it; the oracle's per-row override can
    (oracle.step_batch_cold_rows).  tests/test_double_parity_cases.py shows that swapping the poles' rows moves u by more than
    1e-3 on every lane."""
    rows, x0 = dp.pole_rows(), dp.x0_of(dp.POLE_SEED)
    ref = dp.settled(orc, dp.POLE_OVER, dp.DYN, dp.SET_POINT, x0, rows=rows)
    dp.assert_shares({"pole rows": ref[1]}, "pole rows")
    opt = _handle(pkg, dp.POLE_OVER, pipeline, dp.B)
    got = _outputs(opt.step(T(x0), dp.DYN, dp.SET_POINT, terminal_weights=T(rows)))
    _hold(pkg, "test_terminal_rows_that_differ_between_the_poles", pipeline, got, ref)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. solver options
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["fused", "split"])
@pytest.mark.parametrize("which", range(len(dp.OPTION_SETS)))
def test_solver_options(pkg, orc, which, pipeline):
    """The three option sets of test_gpu_parity.py::test_step_parity_solver_options, 40/10, default rows, 3 iterations.  With
    the third set (3 line-search trials, c1 = 1e-2) 59 of these 96 problems reject every step and end at the cold guess u = 0:
    the kernels must reject the same ones."""
    sopts = dp.OPTION_SETS[which]
    x0 = dp.x0_of(dp.OPTION_SEED)
    ref = dp.settled(orc, dp.OPTION_OVER, dp.DYN, dp.SET_POINT, x0, opts=orc.default_solver_opts(**sopts))
    dp.assert_shares({"options": ref[1]}, "solver options")
    opt = _handle(pkg, dp.OPTION_OVER, pipeline, dp.B, opts=pkg.capi.default_solver_opts(**sopts))
    got = _outputs(opt.step(T(x0), dp.DYN, dp.SET_POINT))
    _hold(pkg, "test_solver_options", "set %d %s" % (which, pipeline), got, ref)
    moved = np.abs(ref[0][0]).max(axis=0) > 0
    assert ((np.abs(got["u"]).max(axis=0) > 0) == moved).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. reset and warm start
# ---------------------------------------------------------------------------------------------------------------------------
def test_reset_and_set_previous_solution(pkg, orc):
    """Optimization::Reset / SetPreviousSolution with nx = 6, on a handle whose workspace stride (128) is not the batch (80)."""
    nB, nx = dp.WARM_B, 6
    x0, x1 = (dp.x0_of(s, nB) for s in dp.WARM_SEEDS)
    u_ref, st_ref, mask = dp.warm_reference(orc)
    assert mask.sum() >= dp.MIN_CASE_SHARE * mask.size                 # from the two oracles alone
    opt = pkg.BatchOptimization(pkg.default_params(**dp.WARM_OVER), max_batch=dp.WARM_MAX_BATCH, dtype=torch.float64, device=0,
                                model="double")
    assert opt.nx == nx
    u1 = opt.step(T(x0), dp.DYN, dp.SET_POINT).u.clone()
    z1 = opt.get_solution(nB)
    out2 = opt.step(T(x1), dp.DYN, dp.SET_POINT, want_guess=True)
    u2, g2, st2 = out2.u.clone(), out2.guess.clone(), N_(out2.status)
    S, N = opt.S, opt.N
    assert (S, N) == (5, 40) and tuple(g2.shape) == (nx * S + N, nB)
    assert torch.equal(g2[nx * S:nx * S + N - 1], z1[nx * S + 1:])     # shift left (optimization.cc:54-57)
    assert torch.equal(g2[-1], z1[-1]) and torch.equal(g2[:nx], T(x1))
    assert not torch.equal(u2, u1)
    opt.reset()
    assert not opt.has_previous_solution()
    assert torch.equal(opt.step(T(x0), dp.DYN, dp.SET_POINT).u, u1)
    opt.reset()
    opt.set_previous_solution(z1)
    assert torch.equal(opt.step(T(x1), dp.DYN, dp.SET_POINT).u, u2)
    # the warm step against one oracle controller per lane stepped twice, on the lanes settled in both steps
    lanes = np.nonzero(mask)[0]
    err = np.abs(N_(u2)[:, lanes] - u_ref[:, lanes]).max(axis=0)
    print("warm step: %d of %d lanes settled, |du| max %.2e median %.2e" % (lanes.size, mask.size, err.max(), np.median(err)))
    assert (st2[lanes] == st_ref[lanes]).all() and err.max() < TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 6. edge batches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,sp,nB", dp.EDGE_BATCHES)
def test_edge_batches(pkg, orc, N, sp, nB):
    """B = 1, 65 and 127 at 40/10 (16 problems a wave) and 40/8 (12 a wave, four lanes riding), default rows."""
    x0 = dp.x0_of(dp.EDGE_SEED, nB)
    over = dp.edge_over(N, sp)
    ref = dp.settled(orc, over, dp.DYN, dp.SET_POINT, x0)
    dp.assert_shares({"edge": ref[1]}, "edge batch")
    opt = pkg.BatchOptimization(pkg.default_params(**over), max_batch=nB, dtype=torch.float64, device=0, model="double")
    assert opt.pipeline() == "fused"
    _hold(pkg, "test_edge_batches", "%d/%d B = %d" % (N, sp, nB), _outputs(opt.step(T(x0), dp.DYN, dp.SET_POINT)), ref)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. a non-finite lane
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["fused", "split"])
def test_non_finite_lane_does_not_poison_neighbours(pkg, pipeline):
    """NaN in a pole angle of lane 17 and inf in b_x of lane 64 (another wave, and at 16 problems a wave another group of
    lanes): those two report NON_FINITE, every other lane's u is bitwise the clean run's."""
    nB = 128
    x0 = dp.x0_of(68, nB)
    over = dict(dp.OVER, max_iterations=4)
    opt = _handle(pkg, over, pipeline, nB)
    clean = opt.step(T(x0), dp.DYN, dp.SET_POINT).u.clone()
    assert torch.isfinite(clean).all()
    bad = x0.copy()
    bad[2, 17] = np.nan
    bad[0, 64] = np.inf
    opt.reset()
    out = opt.step(T(bad), dp.DYN, dp.SET_POINT)
    st = N_(out.status)
    assert st[17] == pkg.capi.TERM["NON_FINITE"] and st[64] == pkg.capi.TERM["NON_FINITE"]
    keep = np.ones(nB, bool)
    keep[[17, 64]] = False
    assert (st[keep] != pkg.capi.TERM["NON_FINITE"]).all()
    assert torch.equal(out.u[:, T(keep, torch.bool)], clean[:, T(keep, torch.bool)])
