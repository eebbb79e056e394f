"""The reference of tests/test_gpu_double_parity.py, checked on the CPU before any kernel is compared with it.

The 6-state cold steps of the case table (tests/helpers/double_parity.py) are solved by the double oracle and by its
extended-precision build.  A lane on which the two agree within 1e-7 (and on termination state and iteration count) is
settled; the GPU tests hold the kernels to the oracle on settled lanes only.  That rule must not become a place to hide a
failure, so here, from the two oracles alone: at least 3/4 of every case's lanes are settled, at least 95 % over each
parametrized test, every case run with the exit tolerances on is mixed (two termination states or two iteration counts), and
no more than one case in eight of a table was dropped, each with its measured reason."""
import numpy as np
import pytest

from helpers import double_parity as dp


def _mixed(ref):
    _, _, st, it = ref
    return len(set(st.tolist())) >= 2 or len(set(it.tolist())) >= 2


@pytest.mark.parametrize("table", ["MIX_CASES", "SHAPE_CASES"])
def test_terminal_mix_cases_are_settled_and_mixed(orc, table):
    cases = getattr(dp, table)
    assert len({c.id for c in cases}) == len(cases)
    masks = {}
    for c in cases:
        ref, m, dist, _ = c.reference(orc)
        assert np.isfinite(ref[0]).all() and m.shape == (dp.B,)
        assert _mixed(ref), c.id
        masks[c.id] = m
    total = dp.assert_shares(masks, table)
    print("%s: %d cases, settled %.4f of the lanes, fewest in a case %d of %d" % (
        table, len(cases), total, min(int(m.sum()) for m in masks.values()), dp.B))


def test_the_tables_hold_what_the_tests_are_to_cover():
    """All 16 sign patterns at 40/10; all cost rows, all equalities, the default and th a cost row with th_dot an equality at
    each of the five other shapes, less the cases listed as dropped: at most one in eight, each with a reason and a distance."""
    assert sorted(c.pattern for c in dp.MIX_CASES) == sorted(dp.PATTERNS) and len(set(dp.PATTERNS)) == 16
    assert all((c.N, c.sp) == (40, 10) for c in dp.MIX_CASES)
    want = {"%dx%d%s" % (N, sp, p) for (N, sp) in dp.SHAPES for p in (dp.ALL_COST, dp.ALL_EQ, dp.DEFAULT, dp.TH_COST_THDOT_EQ)}
    assert len(want) == 20
    dropped = {d[0] for d in dp.DROPPED}
    assert {c.id for c in dp.SHAPE_CASES} == want - dropped and dropped <= want
    assert len(dropped) <= dp.MAX_DROPPED_SHARE * len(want)
    for cid, why, dist in dp.DROPPED:
        assert why and dist > dp.SETTLED_TOL
    # the default mix is the library's default parameters
    assert dp.mix(dp.DEFAULT) == dict(zip(dp.NAMES, (150.0, -1.0, -1.0, -1.0)))


def test_dropped_cases_do_miss_the_share(orc):
    """A case may be listed as dropped only while it does miss 3/4 with the table's default inputs."""
    for cid, _, _ in dp.DROPPED:
        shape, pattern = cid[:-4], cid[-4:]
        N, sp = (int(v) for v in shape.split("x"))
        _, m, _, _ = dp.Case(N, sp, pattern).reference(orc)
        assert m.mean() < dp.MIN_CASE_SHARE, (cid, int(m.sum()))


def test_per_problem_cases_are_settled(orc):
    x0, dyn, sp, tw = dp.per_problem_inputs()
    masks = {k: dp.settled(orc, over, dyn, sp, x0)[1] for k, over in dp.PP_OVER.items()}
    print("per-problem dyn and set_point: settled %.4f" % dp.assert_shares(masks, "per-problem dyn and set_point"))
    x0w = dp.x0_of(dp.PP_SEED, spread=dp.PP_WEIGHTS_SPREAD)
    masks = {"terminal_weights": dp.settled(orc, dp.PP_OVER["default"], dp.DYN, dp.SET_POINT, x0w, terminal_weights=tw)[1]}
    # every one of the 16 sign patterns of the four classes is drawn, and the poles share their rows
    assert len({tuple(c) for c in (tw[[0, 1, 3, 4]] < 0).T.tolist()}) == 16
    assert (tw[1] == tw[2]).all() and (tw[4] == tw[5]).all()
    print("per-problem terminal weights: settled %.4f" % dp.assert_shares(masks, "per-problem terminal weights"))


def test_pole_rows_case_is_settled_and_the_override_is_the_parameters_where_they_can_say_it(orc):
    """The per-row override of the oracle (step_batch_cold_rows): with rows that OptimizationParams can express it is bitwise
    the oracle built from those parameters, in both builds; and the case of the GPU test, whose poles differ, is settled."""
    c = dp.MIX_CASES[6]
    p = orc.default_opt_params(**c.over)
    other = orc.default_opt_params(**dp.MIX_CASES[9].over)      # the rows win over the parameters
    rows = np.tile(dp.rows_of([getattr(p, n) for n in dp.NAMES]).reshape(6, 1), (1, dp.B))
    a = orc.step_batch_cold(p, dp.DYN, dp.SET_POINT, c.x0, want_pred=True, model="double")
    b = orc.step_batch_cold_rows(other, dp.DYN, dp.SET_POINT, c.x0, rows, want_pred=True, model="double")
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
    a = orc.step_batch_cold_ld(p, dp.DYN, dp.SET_POINT, c.x0, model="double")
    b = orc.step_batch_cold_rows_ld(other, dp.DYN, dp.SET_POINT, c.x0, rows, model="double")
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    rows = dp.pole_rows()
    assert ((rows[1] < 0) != (rows[2] < 0)).all() and ((rows[4] < 0) != (rows[5] < 0)).all()
    assert len({tuple(c) for c in (rows < 0).T.tolist()}) == 4
    ref, m, _, _ = dp.settled(orc, dp.POLE_OVER, dp.DYN, dp.SET_POINT, dp.x0_of(dp.POLE_SEED), rows=rows)
    # swapping the poles' rows is another problem: the case can tell a mix-up of rows 1/2 or 4/5
    swapped = dp.settled(orc, dp.POLE_OVER, dp.DYN, dp.SET_POINT, dp.x0_of(dp.POLE_SEED), rows=rows[[0, 2, 1, 3, 5, 4]])[0]
    assert (np.abs(ref[0] - swapped[0]).max(axis=0) > 1e-3).all()
    print("pole rows: settled %.4f" % dp.assert_shares({"pole_rows": m}, "pole rows"))


def test_option_and_edge_cases_are_settled(orc):
    masks = {"options %d" % i: dp.settled(orc, dp.OPTION_OVER, dp.DYN, dp.SET_POINT, dp.x0_of(dp.OPTION_SEED),
                                          opts=orc.default_solver_opts(**s))[1] for i, s in enumerate(dp.OPTION_SETS)}
    print("solver options: settled %.4f" % dp.assert_shares(masks, "solver options"))
    masks = {"%d/%d B=%d" % e: dp.settled(orc, dp.edge_over(e[0], e[1]), dp.DYN, dp.SET_POINT, dp.x0_of(dp.EDGE_SEED, e[2]))[1]
             for e in dp.EDGE_BATCHES}
    print("edge batches: settled %.4f" % dp.assert_shares(masks, "edge batches"))


def test_settled_is_cached_and_read_only(orc):
    c = dp.MIX_CASES[0]
    a, b = c.reference(orc), c.reference(orc)
    assert a is b
    with pytest.raises(ValueError):
        a[0][0][0, 0] = 1.0
