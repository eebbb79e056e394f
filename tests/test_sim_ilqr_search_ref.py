"""CPU: the numpy reference of the fused line search (tests/helpers/sim_ilqr_search_ref.py) held to the reference loop, and the
conditions the GPU test's loop inputs must meet.  The four loop configurations of tests/helpers/sim_ilqr_ref.py (both models, free
and clamped), LOOP_ITERS iterations of LOOP_TRIALS trials, on the first 8 lanes of the 4-state model and the first 4 of the
6-state one.

1. sim_ilqr_ref.loop with search() in the ladder's place reproduces loop's u, cost_history, accepted and mu EXACTLY: the search is
   the ladder, and a failed problem's copy is what the loop's closing roll yields.  The rolls a search took are 1 where alpha = 1 is
   accepted, j + 1 at alpha = 2^-j, and LOOP_TRIALS where nothing is.
2. Admissibility: over those lanes and iterations each configuration shows failure and at least five distinct accepted steps, and
   the union over the four shows every rung 1, 1/2, 1/4, 1/8, 1/16, 1/32 and failure -- so a search that mistook any rung, or
   failure, would show.  The counts are printed."""
import numpy as np
import pytest

from helpers import sim_ilqr_ref as il
from helpers import sim_ilqr_search_ref as se
from helpers import sim_jac_ref as sj
from helpers import sim_rollout_ref as sr

CONFIGS = [(m, c) for m in ("single", "double") for c in (False, True)]
IDS = ["%s-%s" % (m, "clamped" if c else "free") for m, c in CONFIGS]
_RUNS = {}


def _runs(orc, model, clamped):
    """-> (the reference loop's dict, the loop with search()'s dict), each stacked over the configuration's lanes (last axis)"""
    key = (model, clamped)
    if key not in _RUNS:
        nb = se.LOOP_LANES[model]
        x0, u0, target, qf = il.loop_draws(model, nb)
        lim = il.loop_limit(model, clamped)
        xr = il.expand_ref(target, il.LOOP_T, sj.NX[model], nb)
        both = []
        for fn in (il.loop, se.loop_with_search):
            runs = [fn(orc, model, sr._params(sj.DYN[model], b), il.LOOP_DT, x0[:, b], u0[:, b], xr[:, :, b], np.zeros(il.LOOP_T),
                       il.Q[model], il.R, il._terminal(il.Q[model], qf, b), lim, il.LOOP_ITERS, il.LOOP_TRIALS) for b in range(nb)]
            both.append({n: np.stack([np.asarray(run[n]) for run in runs], axis=-1) for n in runs[0]})
        _RUNS[key] = tuple(both)
    return _RUNS[key]


@pytest.mark.parametrize("model,clamped", CONFIGS, ids=IDS)
def test_the_search_in_the_ladders_place_reproduces_the_loop(orc, model, clamped):
    ref, got = _runs(orc, model, clamped)
    for name in ("u", "cost_history", "accepted", "mu", "xs", "cost"):
        assert np.array_equal(ref[name], got[name]), name
    assert np.array_equal(got["accepted"], got["alpha"] > 0)
    j = np.where(got["alpha"] > 0, np.log2(np.where(got["alpha"] > 0, got["alpha"], 1.0)), 0.0)
    assert np.array_equal(got["rolls"], np.where(got["alpha"] > 0, 1 - j, il.LOOP_TRIALS).astype(int))


@pytest.mark.parametrize("model,clamped", CONFIGS, ids=IDS)
def test_the_loops_steps_cover_the_ladder(orc, model, clamped):
    _, got = _runs(orc, model, clamped)
    a = got["alpha"]
    counts = [int((a == s).sum()) for s in se.RUNGS] + [int((a == 0).sum())]
    print("ilqr search ref %s %s: steps accepted over %d lanes x %d iterations: %s, no step %d; rolls %d of %d" % (
        model, "clamped" if clamped else "free", a.shape[1], a.shape[0],
        "  ".join("%g: %d" % (s, c) for s, c in zip(se.RUNGS, counts)), counts[-1], got["rolls"].sum(), a.size * (il.LOOP_TRIALS + 1)))
    assert sum(counts) == a.size                                                  # nothing but the rungs and failure
    assert counts[-1] > 0 and sum(c > 0 for c in counts[:-1]) >= 5


def test_the_four_configurations_together_show_every_rung_and_failure(orc):
    a = np.concatenate([_runs(orc, m, c)[1]["alpha"].ravel() for m, c in CONFIGS])
    assert set(np.unique(a)) == set(se.RUNGS) | {0.0}
