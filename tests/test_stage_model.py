"""tests/helpers/stage_model.py pinned on the CPU, on hand-made iteration counts: both finishing rules of the staged fused
pipeline on either side of their thresholds, the counter index beyond three cuts, the problems-per-wave counts that round
down, a list that empties -- and, with the double CPU check, that the inputs of tests/test_gpu_staged_restarts.py reach the
conditions that file asserts on the GPU (float64 forms: the fp64 kernels reproduce the check's iteration counts)."""
import numpy as np
import pytest

from helpers import stage_model as sm


def _counts(hist):
    """{final count: problems} -> the count vector, sorted (the model does not depend on the order)."""
    return np.concatenate([np.full(n, c, np.int64) for c, n in sorted(hist.items())])


def _stages(hist, bounds, L, cap, at_cap=None):
    its = _counts(hist)
    none = its == cap if at_cap is None else at_cap
    return sm.working_stages(its, none, bounds, L, cap)


def test_run_out_threshold_rounds_the_problems_per_wave_down():
    assert [sm.run_out_below(L) for L in (2, 4, 5, 8, 10, 16)] == [65536, 32768, 24576, 16384, 12288, 8192]
    assert sm.run_out_below(10) == 2048 * 6 and sm.run_out_below(5) == 2048 * 12      # not 6.4 and 12.8
    assert [sm.batch_of(L) for L in (10, 16, 5, 8)] == [24653, 16461, 49229, 32845]


def test_plan_bounds_restate_the_fixed_plan():
    assert sm.plan_bounds(0, 0, 8) == [0, 8] and sm.plan_bounds(8, 1, 8) == [0, 8] and sm.plan_bounds(3, 0, 8) == [0, 8]
    assert sm.plan_bounds(1, 1, 4) == [0, 1, 2, 3, 4]
    assert sm.plan_bounds(2, 1, 5) == [0, 2, 3, 4, 5]
    assert sm.plan_bounds(1, 3, 12) == [0, 1, 4, 7, 10, 12]       # the last launch takes what is left
    assert sm.plan_bounds(3, 2, 8) == [0, 3, 5, 7, 8]


def test_host_chunks_are_equalised_and_the_default_plan_needs_more_than_2048_waves():
    assert sm.host_chunks(24653, 0) == [(0, 24653)]
    chunks = sm.host_chunks(24653, 2048)                          # thirteen chunks of 1 920, the last one ragged
    assert len(chunks) == 13 and chunks[:2] == [(0, 1920), (1920, 1920)] and chunks[-1] == (23040, 1613)
    assert sm.host_chunks(24653, 13000) == [(0, 12352), (12352, 12301)]      # not 13 000 + 11 653
    assert sm.host_chunks(24653, 13200) == [(0, 12352), (12352, 12301)]
    assert sm.host_chunks(24653, 16436) == [(0, 24653)]           # up to one and a half chunks: unsplit
    assert sm.host_chunks(27077, 14000) == [(0, 13568), (13568, 13509)]
    assert not sm.default_plan_stages(12352, 10) and not sm.default_plan_stages(13107, 10)
    assert sm.default_plan_stages(13108, 10) and sm.default_plan_stages(13509, 10) and sm.default_plan_stages(24653, 10)


@pytest.mark.parametrize("L", [10, 5, 16])
def test_rule_1_on_either_side_of_its_threshold(L):
    """A list of exactly run_out_below problems finishes; one more does not (cap 12, plan 1 + 1: rule 2 cannot hold before
    done = 9).  Everybody who is listed runs all 12, so no list shrinks by itself."""
    T = sm.run_out_below(L)
    for extra, fires in ((0, True), (1, False)):
        hist = {1: 3 * T, 12: T + extra}
        launches, active_in = _stages(hist, sm.plan_bounds(1, 1, 12), L, 12)
        assert len(launches) == 12 and launches[0] == sm.Launch(0, 4 * T + extra, False, False, False)
        assert launches[1].n_list == T + extra and launches[1].rule1 == fires and not launches[1].rule2
        if fires:
            assert launches[1].finishes and [l.n_list for l in launches[2:]] == [0] * 10
            assert not any(l.rule1 or l.rule2 or l.finishes for l in launches[2:])
            assert active_in.max() == 2 and (active_in == 2).sum() == T
        else:
            # ... then it is worked on at done = 1 .. 8 without a rule, and rule 2 finishes it at done = 9 (remaining 3 <= 3)
            assert [l.n_list for l in launches[1:10]] == [T + 1] * 9 and not any(l.finishes for l in launches[1:9])
            assert launches[9].done == 9 and launches[9].rule2 and not launches[9].rule1 and launches[9].finishes
            assert [l.n_list for l in launches[10:]] == [0, 0]
            assert active_in.max() == 10 and (active_in == 10).sum() == T + 1 and (active_in == 1).sum() == 3 * T


def test_rule_2_on_either_side_of_both_thresholds():
    L, cap = 10, 8
    n = 40000                                  # every list stays above run_out_below(10) = 12 288: rule 1 never holds
    # the ratio: 36 000 of 40 000 listed at done = 5 is exactly nine tenths -- fires; 35 999 does not
    for listed, fires in ((36000, True), (35999, False)):
        hist = {5: n - listed, 8: listed}
        launches, active_in = _stages(hist, sm.plan_bounds(5, 1, cap), L, cap)
        assert [l.done for l in launches] == [0, 5, 6, 7]
        assert launches[1].n_list == listed and launches[1].rule2 == fires and not launches[1].rule1
        if fires:
            assert launches[1].finishes and launches[2].n_list == 0 and launches[3].n_list == 0
            assert active_in.max() == 2
        else:
            # at done = 6 nobody has stopped since: the ratio is 1 against the list BEFORE it (35 999, not the batch)
            assert launches[2].n_list == listed and launches[2].rule2 and launches[2].finishes and launches[3].n_list == 0
            assert active_in.max() == 3
    # the budget: remaining <= max(2 k, 3).  Plan 1 + 1 (k = 1): from done = 5 on; plan 2 + 2 (k = 2): remaining 4 <= 4 at done = 4
    hist = {8: n}
    launches, _ = _stages(hist, sm.plan_bounds(1, 1, cap), L, cap)
    assert [l.rule2 for l in launches] == [False] * 5 + [True] + [False] * 2      # done = 4: 4 > 3; done = 5: 3 <= 3
    assert [l.n_list for l in launches] == [n] * 6 + [0, 0]
    assert sm.rule2_fires_after_not_firing(launches)
    launches, _ = _stages(hist, sm.plan_bounds(2, 2, cap), L, cap)
    assert [(l.done, l.rule2) for l in launches] == [(0, False), (2, False), (4, True), (6, False)]   # done = 2: 6 > 4
    # k is the launch's own share of the plan: in 1 + 3 at cap 12 the launch at done = 7 has k = 3 and remaining 5 <= 6
    launches, _ = _stages({12: n}, sm.plan_bounds(1, 3, 12), L, 12)
    assert [(l.done, l.rule2) for l in launches] == [(0, False), (1, False), (4, False), (7, True), (10, False)]
    # ... and the last launch of a plan finishes whoever it holds without any rule
    launches, _ = _stages({3: 10000, 8: 30000}, [0, 2, 8], L, cap)
    assert launches[1] == sm.Launch(2, 40000, False, True, True)                 # (remaining 6 <= 12: rule 2 as well)
    launches, _ = _stages({3: 30000, 12: 30000}, [0, 2, 5, 12], L, 12)
    assert launches[1] == sm.Launch(2, 60000, False, False, False)                # remaining 10 > 6
    assert launches[2] == sm.Launch(5, 30000, False, False, True)                 # half left, 7 > ... no rule: the last launch


def test_rule_2_compares_with_the_list_before_it_across_the_counter_wrap():
    """Seven cuts: the counters of compactions 0 .. 6 sit at indices 0 1 2 0 1 2 0, and n_prev of each is the list before it --
    never the batch again.  The lists fall by a fifth each time, so rule 2's ratio does not hold where its budget half first
    does (done = 5); then they hold still and it fires."""
    L, cap = 16, 8
    lists = [100000, 80000, 64000, 51200, 40960, 40000, 39000]       # listed after done = 1 .. 7
    hist = {1: 200000 - lists[0]}
    for j in range(1, 7):
        hist[j + 1] = lists[j - 1] - lists[j]
    hist[8] = lists[6]
    launches, active_in = _stages(hist, sm.plan_bounds(1, 1, cap), L, cap)
    assert [l.n_list for l in launches] == [200000] + lists[:6] + [0]
    # done = 5: 40 960 * 10 >= 51 200 * 9 is false (409 600 < 460 800) although remaining 3 <= 3 ...
    assert launches[5].done == 5 and not launches[5].rule2 and not launches[5].finishes
    # ... done = 6: 40 000 of 40 960 -- fires, the list of done = 7 is empty
    assert launches[6].rule2 and launches[6].finishes and launches[7].n_list == 0
    assert sm.rule2_fires_after_not_firing(launches)
    assert active_in.max() == 7 and (active_in == 7).sum() == 40000 and (active_in == 6).sum() == 960
    shares = sm.removed_shares(launches)
    assert len(shares) == 6 and shares[0] == 0.5 and all(abs(s - 0.2) < 1e-12 for s in shares[1:5]) and abs(shares[5] - 960 / 40960) < 1e-12


def test_a_list_that_empties_and_problems_without_a_status_at_the_cap():
    L, cap = 5, 6
    T = sm.run_out_below(L)
    # everybody stops by iteration 3: the lists of done = 3, 4, 5 are empty without any rule having fired
    launches, active_in = _stages({1: T, 2: T, 3: 2 * T}, sm.plan_bounds(1, 1, cap), L, cap)
    assert [l.n_list for l in launches] == [4 * T, 3 * T, 2 * T, 0, 0, 0]
    assert not any(l.rule1 or l.rule2 or l.finishes for l in launches)
    assert sm.removed_shares(launches) == [0.25, 1.0 - 2.0 / 3.0]           # the emptying compaction feeds no launch
    assert sorted(set(active_in.tolist())) == [1, 2, 3] and not sm.rule2_fires_after_not_firing(launches)
    # a problem at the cap is listed at every done < cap whether it ended there with a status or without one ...
    its = _counts({2: 2 * T, 6: 2 * T})
    for none in (its == cap, np.zeros(its.size, bool)):
        launches, active_in = sm.working_stages(its, none, [0, 1, 2, 3, 6], L, cap)
        assert [l.n_list for l in launches] == [4 * T, 4 * T, 2 * T, 2 * T]
        # done = 2: 2 T > T, no rule 1; half the list before it, no rule 2 -- so the list of done = 3 holds them again
        assert launches[2] == sm.Launch(2, 2 * T, False, False, False)
        assert launches[3] == sm.Launch(3, 2 * T, False, True, True)         # (remaining 3 <= 2 * 3)
        assert (active_in == 4).sum() == 2 * T and (active_in == 2).sum() == 2 * T
    # ... but "no status" below the cap is not a count a launch can leave behind
    with pytest.raises(AssertionError):
        sm.working_stages(its, its == 2, [0, 3, 6], L, cap)
    with pytest.raises(AssertionError):
        sm.working_stages(its, its == cap, [0, 3, 5], L, cap)               # a plan ends at the cap
    with pytest.raises(AssertionError):
        sm.working_stages(its + 1, its + 1 == cap, [0, 3, 6], L, cap)       # no count beyond the cap


DYN = {"single": [1.0, 0.1, 0.25, 9.81, 0.05, 0.1, 0.02, 0.8, 100.0], "double": [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]}


@pytest.mark.parametrize("model,N,sp", sm.SHAPES, ids=["%s-%dx%d" % s for s in sm.SHAPES])
def test_the_cold_inputs_of_the_staged_restart_cases_reach_their_conditions(orc, model, N, sp):
    """Conditions (a) and (c) of tests/test_gpu_staged_restarts.py on the cold step, from the double CPU check's iteration
    counts on the first 2 048 problems of the shape's batch, repeated up to B (shared inputs): in the plan 1 + 1 at cap 12 at
    least four launches work on a list beyond run_out_below, so that some problem is reloaded three times or more; at cap 8
    rule 2 finishes a launch after not holding for an earlier list.  And no problem ends NON_FINITE, without which the
    model would not describe the run."""
    L = N // sp
    B = sm.batch_of(L)
    x0 = sm.cold_states(model, B, sm.X0_SEED[model])[:, :2048]
    for cap in (12, 8):
        p = orc.default_opt_params(window_length=N, state_spacing=sp, max_iterations=cap)
        _, _, status, its, _ = orc.step_batch_cold(p, DYN[model], 0.0, x0, model=model)
        assert (status != 8).all() and (status != 0).all(), np.bincount(status)
        launches, active_in = sm.working_stages(np.resize(its, B), np.resize(status == 1, B), sm.plan_bounds(1, 1, cap), L, cap)
        lists = [l.n_list for l in launches]
        if cap == 12:
            assert sm.lists_beyond_run_out(launches, L) >= 4 and active_in.max() >= 4, lists
        else:
            assert sm.rule2_fires_after_not_firing(launches), lists
