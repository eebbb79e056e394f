"""The launches of a staged fused SQP step, restated on the host from the iteration counts of a single-launch run.

With exit tolerances on, the fused pipeline runs `bounds[i + 1] - bounds[i]` iterations per launch of fused_sqp_kernel and
compacts the problems that still iterate between two launches (csrc/engine_impl.hpp: step_batch_impl).  A staged run gives
the single launch's results, so the single launch's per-problem iteration counts say what every launch of any plan worked on:

  * compact_active_kernel (csrc/mpc_kernels.hpp) lists problem p when `status[p] == NONE && iters[p] < iter_cap`.  After
    `done < cap` iterations that is the set of problems whose final count exceeds `done`: an active problem gains one count per
    iteration, and whichever iteration gives it a status is counted too -- except NON_FINITE, which stops a problem WITHOUT
    counting the iteration, so the model holds for runs without that status only (the callers assert it).  A problem that is
    still NONE at the cap has count == cap > done and is listed like the others; once a launch has run to the cap it fails
    the `iters < iter_cap` half and later lists do not hold it.
  * a later launch gives itself the whole budget (csrc/mpc_fused_body.inc, lines 54-65)
      rule 1:  n_active <= run_out_below = 2048 * (64 // L), or
      rule 2:  n_active * 10 >= n_prev * 9  and  remaining <= max(2 k, 3),
    with k = bounds[stage + 2] - done its own share of the plan, remaining = cap - done, and n_prev the list of the launch
    before it (the whole batch for the first compaction).  Every problem then runs to its own end and the launches that follow
    find an empty list.
"""
from collections import namedtuple

import numpy as np

from conftest import random_states
from helpers.double_parity import near_upright

# one launch of fused_sqp_kernel: iterations done before it, problems it works on, whether rule 1 / rule 2 holds for it
# (both False for the first launch, which has no list, and for a launch with an empty list), and whether it runs every
# problem it holds to the end (a rule, or simply the last launch of the plan)
Launch = namedtuple("Launch", "done n_list rule1 rule2 finishes")


def run_out_below(L):
    """engine_impl.hpp: a.run_out_below -- the problems of one round of resident waves (64 // L per wave, rounded down)."""
    return 2048 * (64 // L)


def working_stages(iterations, status_none_at_cap, bounds, L, cap):
    """iterations [B]: final count per problem of a single launch; status_none_at_cap [B] bool: the problem ran into
    max_iterations without a status (what finalize reports as MAX_ITERATIONS) -- a sanity check of the counts only, it does
    not enter the lists: such a problem is listed at every done < cap like any other whose count exceeds done;
    bounds: the plan, 0 = bounds[0] < ... < bounds[n] = cap; L: shooting intervals.
    -> ([Launch] * n, active_in [B]: the launches a problem was worked on in; it was reloaded active_in - 1 times)."""
    its = np.asarray(iterations).astype(np.int64)
    at_cap = np.asarray(status_none_at_cap).astype(bool)
    bounds = [int(b) for b in bounds]
    assert its.ndim == 1 and at_cap.shape == its.shape
    assert len(bounds) >= 2 and bounds[0] == 0 and bounds[-1] == cap and all(b > a for a, b in zip(bounds, bounds[1:])), bounds
    assert its.min() >= 0 and its.max() <= cap, (its.min(), its.max())
    assert (its[at_cap] == cap).all(), "a problem without a status stops at the cap only"
    n = len(bounds) - 1
    B = its.size
    launches = [Launch(0, B, False, False, n == 1)]
    active_in = np.ones(B, np.int64)
    finished = n == 1          # some launch has run everybody to the end
    n_prev = B                 # stage 0: prev_count is null, prev_total = B
    for stage in range(n - 1):
        done = bounds[stage + 1]
        listed = np.zeros(B, bool) if finished else its > done
        n_active = int(listed.sum())
        k, remaining = bounds[stage + 2] - done, cap - done
        rule1 = n_active > 0 and n_active <= run_out_below(L)
        rule2 = n_active > 0 and n_active * 10 >= n_prev * 9 and remaining <= max(2 * k, 3)
        last = stage + 2 == n
        launches.append(Launch(done, n_active, rule1, rule2, n_active > 0 and (rule1 or rule2 or last)))
        active_in += listed
        finished = finished or rule1 or rule2
        n_prev = n_active      # the counter of this compaction is the next one's prev_count, empty or not
    return launches, active_in


def plan_bounds(first, nxt, cap):
    """cpmpc_set_compaction(first, nxt) as cpmpc_plan_stages cuts it (csrc/cpmpc_api.hip: fixed): `first` iterations, then
    `nxt` at a time, the last launch taking what is left; one launch when either is 0 or first >= cap."""
    if first <= 0 or nxt <= 0 or cap <= first:
        return [0, cap]
    bounds = [0, first]
    while bounds[-1] < cap:
        bounds.append(min(bounds[-1] + nxt, cap))
    return bounds


def host_chunks(B, chunk):
    """The chunks (first column, problems) that cpmpc_step_batch_host_in cuts B problems into after cpmpc_set_host_chunk(chunk)
    (csrc/cpmpc_host.hip: host_chunks_of): unsplit up to one and a half chunks, else ceil(B / chunk) chunks of EQUAL size rounded
    up to a multiple of 64 -- so two chunks of "13 000" out of 24 653 are 12 352 and 12 301 problems."""
    n = (B + chunk - 1) // chunk if chunk > 0 and B > chunk + chunk // 2 else 1
    step = ((B + n - 1) // n + 63) // 64 * 64
    return [(c0, min(step, B - c0)) for c0 in range(0, B, step)]


def default_plan_stages(n_problems, L):
    """cpmpc_plan_stages: the default plan stages a batch (a chunk) only beyond one round of resident waves, 2 048."""
    return (n_problems * L + 63) // 64 > 2048


def lists_beyond_run_out(launches, L):
    """Launches whose list is longer than one round of resident waves (the first launch's is the batch)."""
    return sum(1 for l in launches if l.n_list > run_out_below(L))


def rule2_fires_after_not_firing(launches):
    """Condition (c) of tests/test_gpu_staged_restarts.py on one step: a later launch that only rule 2 finishes, and before it
    a later launch with a list for which neither rule holds."""
    later = launches[1:]
    for i, l in enumerate(later):
        if l.n_list > 0 and l.rule2 and not l.rule1:
            return any(e.n_list > 0 and not e.rule1 and not e.rule2 for e in later[:i])
    return False


# ---- the shapes of tests/test_gpu_staged_restarts.py, shared with the CPU check of their inputs (tests/test_stage_model.py) --
# (model, N, spacing): B = 2 * run_out_below + 77 -- two rounds of resident waves and a ragged tail for every problems-per-wave
# count: 24 653 at L = 10, 16 461 at L = 16 (the run-time-spacing kernel), 49 229 at L = 5, 32 845 at L = 8
SHAPES = [("single", 40, 4), ("single", 80, 5), ("single", 40, 8), ("double", 40, 5), ("double", 40, 8)]
X0_SEED = {"single": 2026, "double": 2027}


def batch_of(L):
    return 2 * run_out_below(L) + 77


def cold_states(model, B, seed):
    """The cold initial states [nx, B] of a shape (float64): the 4-state model from BASELINE.md's distribution with every third
    pole within 0.3 rad of upright, the 6-state one with both poles within 0.15 rad of upright -- the families of
    tests/test_gpu_position_independence.py."""
    rng = np.random.default_rng(seed)
    if model == "single":
        x0 = random_states(rng, B)
        x0[1, ::3] = np.pi / 2 + rng.uniform(-0.3, 0.3, x0[1, ::3].shape)
        return x0
    return near_upright(rng, B, spread=0.15)


def removed_shares(launches):
    """Per compaction whose list is worked on again (not empty, and the launch before it did not run everybody to the end):
    the share of the list before it that it removed."""
    return [1.0 - b.n_list / a.n_list for a, b in zip(launches, launches[1:]) if b.n_list > 0 and not a.finishes]
