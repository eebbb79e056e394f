"""The reference of tests/test_gpu_limits_parity.py, checked on the CPU before any kernel is compared with it.

The cold steps of the case table (tests/helpers/limits_parity.py) are solved by the double oracle and by its
extended-precision build, with option sets that pull the retraction limits (b_x_limit, u_limit) into the solution and move
every rung of the damping ladder.  From the two oracles alone, for every case: at least 95 % of the lanes are settled; at
least 20 % end with a control exactly on the limit; where the set lowers b_x_limit, at least a quarter of the inspected lanes
end with a node on it; sets A, C and D of the 4-state model end in at least two termination states with three lanes or more
each, MAX_LAMBDA among them at 40/10; and no lambda_max lies on a rung of its ladder, where the exit iteration would depend
on rounding."""
import numpy as np
import pytest

from helpers import double_parity as dp
from helpers import limits_parity as lp


def test_the_table_holds_what_the_tests_are_to_cover():
    assert len({(c.model, c.id) for c in lp.ALL_CASES}) == len(lp.ALL_CASES)
    assert {(c.N, c.sp, c.set_name) for c in lp.CASES4} == {(N, sp, s) for (N, sp) in lp.SHAPES4 for s in "ABCD"}
    assert {(c.N, c.sp, c.set_name) for c in lp.CASES6} == {(N, sp, s) for (N, sp) in lp.SHAPES6 for s in ("A6", "B6", "C6")}
    assert [(c.N, c.sp, c.set_name, c.kind) for c in lp.SITE_CASES] == [(40, 10, "A", "pp"), (40, 10, "A", "refine")]
    # the sets, verbatim: a case may move a limit (below), the table never edits a set
    assert lp.SETS["A"] == dict(u_limit=8.0, lambda_max=30.0) and lp.SETS["B"] == dict(u_limit=12.0, b_x_limit=0.4)
    assert lp.SETS["C"] == dict(u_limit=20.0, lambda_initial=3.0, lambda_scale_up=4.0, lambda_scale_down=0.5, lambda_min=0.2,
                                lambda_max=150.0)
    assert lp.SETS["D"] == dict(b_x_limit=0.3, u_limit=15.0, max_line_search_iterations=2, lambda_failure_init=0.7,
                                lambda_max=500.0)
    assert lp.SETS["A6"] == dict(u_limit=2.0) and lp.SETS["B6"] == dict(u_limit=1.0, b_x_limit=0.05)
    assert lp.SETS["C6"] == dict(lp.SETS["C"], u_limit=3.0)
    # ... and the two this repository adds: C and C6 with lambda_min on a rung times scale_down
    assert lp.SETS["E"] == dict(lp.SETS["C"], lambda_min=0.375) and lp.SETS["E6"] == dict(lp.SETS["C6"], lambda_min=0.375)
    assert [(c.model, c.N, c.sp, c.set_name) for c in lp.RUNG_CASES] == [("single", 40, 10, "E"), ("double", 40, 10, "E6")]
    # a case may move a limit of its set (with the reason in the table), never the ladder or the line search
    for c in lp.ALL_CASES:
        assert set(c.moved) <= {"u_limit", "b_x_limit"}, c.id
        assert c.inspected.size <= lp.INSPECTED and len(set(c.inspected.tolist())) == c.inspected.size
    assert sum(bool(c.moved) for c in lp.ALL_CASES) == 3
    dyn, sp = lp.per_problem_inputs()
    assert dyn.shape == (9, lp.B4) and sp.shape == (lp.B4,) and len(set(sp.tolist())) == lp.B4


@pytest.mark.parametrize("case", lp.ALL_CASES, ids=lambda c: "%s-%s" % (c.model, c.id))
def test_cases_are_settled_and_the_limits_and_the_ladder_are_live(orc, case):
    (u, pred, st, it), mask, dist, _ = case.reference(orc)
    o = orc.default_solver_opts(**case.sopts)
    assert np.isfinite(u).all() and mask.shape == (case.B,)
    at_u = lp.u_at_limit(u, o.u_limit)
    nodes, controls, z = case.at_limits(orc)
    hist = lp.histogram(orc, st)
    print("limits %s %s: settled %d of %d, control on u_limit %.0f %% of lanes, node on b_x_limit %d of %d inspected, %s" % (
        case.model, case.id, mask.sum(), mask.size, 100 * at_u.mean(), nodes.sum(), nodes.size, hist))
    assert mask.mean() >= lp.MIN_SETTLED, (int(mask.sum()), mask.size)
    assert at_u.mean() >= lp.MIN_AT_U_LIMIT, at_u.mean()
    # only the retraction clamps: a lane that rejects every step returns its cold guess as it is, and with set A (u_limit 8)
    # the guess's sinusoid (amplitude 10) lies beyond the limit.  Such a lane ends in MAX_LAMBDA; every other one is inside.
    beyond = (np.abs(u) > o.u_limit).any(axis=0)
    assert (st[beyond] == orc.TERM["MAX_LAMBDA"]).all() and np.abs(u).max() <= max(o.u_limit, case.amplitude(orc))
    assert not beyond.any() or case.set_name == "A"
    # the controller per lane is the batch call's lane: same controls, so the same lanes on the limit
    S = case.N // case.sp + 1
    assert np.array_equal(z[case.nx * S:], u[:, case.inspected]) and np.array_equal(controls, at_u[case.inspected])
    if case.set_name in lp.LOWERS_B_X:
        assert nodes.mean() >= lp.MIN_AT_B_X_LIMIT, (int(nodes.sum()), nodes.size)
    else:
        assert o.b_x_limit == 5.0 and not nodes.any()
    if case.set_name in lp.LADDER_SETS:
        held = [k for k, v in hist.items() if v >= lp.MIN_STATE_LANES]
        assert len(held) >= 2, hist
        if (case.N, case.sp) == (40, 10):
            assert "MAX_LAMBDA" in held, hist


@pytest.mark.parametrize("name", sorted(lp.SETS))
def test_lambda_max_is_on_no_rung_of_its_ladder(orc, name):
    """lambda > lambda_max is tested after the multiply: were lambda_max a reachable rung, the double oracle (exactly on it:
    goes on) and the extended-precision one (an ulp of long double above: stops) would leave one iteration apart."""
    o = orc.default_solver_opts(**lp.SETS[name])
    rungs = lp.rungs_of(o, 8)
    assert rungs.size >= 8 and (rungs > 0).all()
    rel = np.abs(rungs - o.lambda_max) / o.lambda_max
    assert rel.min() > 1e-9, (name, o.lambda_max, rungs[rel.argmin()])
    # and the guard does see the trap: lambda_max = 10 on the default ladder 1e-2 * 10^k
    trap = orc.default_solver_opts(lambda_max=10.0)
    assert (np.abs(lp.rungs_of(trap, 8) - 10.0) / 10.0).min() <= 1e-9


@pytest.mark.parametrize("case", lp.RUNG_CASES, ids=lambda c: "%s-%s" % (c.model, c.id))
def test_lambda_min_on_a_rung_tells_less_from_less_or_equal(orc, case):
    """Sets E / E6: lambda_min = 0.375 is reached exactly (3 * 0.5^3).  With `<` the reference is that of C / C6 bit for bit;
    with lambda_min one ulp higher -- what `<=` would do -- at least half of the lanes exit elsewhere or end more than the
    kernels' tolerance away, so a kernel that compares with `<=` cannot pass the GPU test of these cases."""
    o = orc.default_solver_opts(**case.sopts)
    assert o.lambda_min in lp.rungs_of(o, 8).tolist() and o.lambda_min / o.lambda_scale_down in lp.rungs_of(o, 8).tolist()
    (u, pred, st, it), mask, _, _ = case.reference(orc)
    plain = lp.Case(case.model, case.N, case.sp, case.set_name.replace("E", "C"))
    (u_c, pred_c, st_c, it_c), mask_c, _, _ = plain.reference(orc)
    assert np.array_equal(u, u_c) and np.array_equal(st, st_c) and np.array_equal(it, it_c) and np.array_equal(mask, mask_c)
    above = dict(case.sopts, lambda_min=float(np.nextafter(o.lambda_min, 1.0)))
    (u_a, _, st_a, it_a), _, _, _ = dp.settled(orc, case.over, case.dyn, case.set_point, case.x0,
                                               opts=orc.default_solver_opts(**above), model=case.model)
    told = (st_a != st) | (it_a != it) | (np.abs(u_a - u).max(axis=0) > 1e-5)
    print("lambda_min on a rung, %s %s: `<=` would change %d of %d lanes" % (case.model, case.id, told.sum(), told.size))
    assert told.mean() >= 0.5


def test_the_trap_is_real_and_an_artefact_of_the_comparison(orc):
    """lambda_max = 10 on the default ladder: the two oracles part on lanes that climb to it, and with 30 they do not."""
    c = lp.CASES4[0]
    on_rung = dp.settled(orc, c.over, c.dyn, c.set_point, c.x0, opts=orc.default_solver_opts(u_limit=8.0, lambda_max=10.0),
                         model="single")[1]
    print("lambda_max = 10 on the ladder: %d of %d lanes settled; with 30: %d" % (on_rung.sum(), on_rung.size,
                                                                                   c.reference(orc)[1].sum()))
    assert on_rung.mean() < lp.MIN_SETTLED <= c.reference(orc)[1].mean()


@pytest.mark.parametrize("model", ["single", "double"])
def test_warm_cases_are_settled_and_start_from_a_solution_on_the_limit(orc, model):
    u2, st2, it2, mask, first, z2 = lp.warm_reference(orc, model)
    print("warm %s: %d of %d lanes settled in both steps, %d with the first solution on u_limit" % (
        model, mask.sum(), mask.size, first.sum()))
    assert mask.size == lp.WARM_LANES and mask.mean() >= lp.MIN_SETTLED
    assert first.mean() >= lp.MIN_AT_U_LIMIT


def test_references_are_cached_and_read_only(orc):
    c = lp.CASES4[0]
    assert c.reference(orc) is c.reference(orc) and c.at_limits(orc) is c.at_limits(orc)
    with pytest.raises(ValueError):
        c.at_limits(orc)[2][0, 0] = 1.0
