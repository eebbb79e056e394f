"""Cases and references of the 6-state (cart + double pendulum) SQP parity tests, float64.

One table for tests/test_double_parity_cases.py (CPU: is the reference itself fit to compare against?) and
tests/test_gpu_double_parity.py (GPU: do the kernels agree with it?).  numpy and the oracle only: no torch here.

SETTLED LANES.  The double oracle and its extended-precision build (oracle/cpmpc_oracle_ld.c: the same algorithm in x87 long
double) are run on the same problems.  A lane is settled when the two agree on termination state and iteration count and on u
within SETTLED_TOL = 1e-7: two decades under the 1e-5 the kernels are held to, so a lane whose own rounding sensitivity could
carry a correct kernel -- another summation order, another QP algorithm -- past the tolerance is not in the compared set.  The
kernels are held to the oracle on settled lanes only; how many lanes of a case must be settled is asserted from the two
oracles alone (MIN_CASE_SHARE, MIN_TEST_SHARE), before anything from the GPU is looked at.

Inputs everywhere: near_upright (tests/test_gpu_double.py) with the given spread, x0[0] and x0[3:] times 0.2, the seed written
in the case, u_guess_sinusoid_amplitude = 0."""
import itertools

import numpy as np

DYN = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]
OVER = dict(u_guess_sinusoid_amplitude=0.0)
SOFT = dict(state_spacing=5, th_final_cost_weight=200.0, th_dot_final_cost_weight=20.0, b_x_dot_final_cost_weight=20.0)
SETTLED_TOL = 1e-7
MIN_CASE_SHARE = 0.75        # of the lanes of one case
MIN_TEST_SHARE = 0.95        # of the lanes of all cases of one parametrized test
MAX_DROPPED_SHARE = 1 / 8    # of the cases of one parametrized test
B = 96
SET_POINT = 0.02

# the four weight classes of OptimizationParams in the order of a sign pattern; '+' = the weight (a cost row), '-' = -1 (an
# equality row).  For the 6-state model the th and th_dot weights apply to both poles (oracle/cpmpc_oracle.c: terminal_spec).
NAMES = ("b_x_final_cost_weight", "th_final_cost_weight", "b_x_dot_final_cost_weight", "th_dot_final_cost_weight")
WEIGHTS = (150.0, 200.0, 20.0, 20.0)
PATTERNS = ["".join(s) for s in itertools.product("+-", repeat=4)]
ALL_COST, ALL_EQ, DEFAULT, TH_COST_THDOT_EQ = "++++", "----", "+---", "++--"
SHAPES = [(40, 5), (20, 10), (20, 5), (40, 8), (30, 6)]          # 30/6: the run-time-spacing kernel


def near_upright(rng, B, spread=0.15):
    """tests/test_gpu_double.py: near_upright, draw for draw."""
    return np.stack([rng.uniform(-0.3, 0.3, B), np.pi / 2 + rng.uniform(-spread, spread, B),
                     np.pi / 2 + rng.uniform(-spread, spread, B), rng.uniform(-0.3, 0.3, B),
                     rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B)])


_X0 = {}


def x0_of(seed, B=B, spread=0.05):
    """The initial states of a seed, drawn once and read-only."""
    key = (seed, B, spread)
    if key not in _X0:
        x0 = near_upright(np.random.default_rng(seed), B, spread)
        x0[0] *= 0.2
        x0[3:] *= 0.2
        x0.setflags(write=False)
        _X0[key] = x0
    return _X0[key]


def mix(pattern):
    """The four *_final_cost_weight parameters of a sign pattern."""
    return {n: (w if s == "+" else -1.0) for n, w, s in zip(NAMES, WEIGHTS, pattern)}


def rows_of(weights4, nx=6):
    """Four class weights [4] or [4, B] -> terminal weights in state order [nx] or [nx, B] (both poles share theirs)."""
    w = np.asarray(weights4, dtype=np.float64)
    nq = nx // 2
    return np.stack([w[0 if t == 0 else 1 if t < nq else 2 if t == nq else 3] for t in range(nx)])


class Case:
    """One problem definition and its inputs.  iterations: max_iterations, with the default exit tolerances (exits on)."""

    def __init__(self, N, sp, pattern, iterations=4, seed=61, spread=0.05):
        self.N, self.sp, self.pattern, self.iterations, self.seed, self.spread = N, sp, pattern, iterations, seed, spread

    @property
    def id(self):
        return "%dx%d%s" % (self.N, self.sp, self.pattern)

    @property
    def over(self):
        return dict(OVER, window_length=self.N, state_spacing=self.sp, max_iterations=self.iterations, **mix(self.pattern))

    @property
    def x0(self):
        return x0_of(self.seed, B, self.spread)

    def reference(self, orc):
        return settled(orc, self.over, DYN, SET_POINT, self.x0)


# THE TABLE.  Default inputs of a case: 4 iterations with the default exit tolerances, seed 61, spread 0.05.  Measured on the
# CPU with these, every case has lanes that stop for different reasons (4 is the smallest cap at which that holds; at 8 the
# rounding-sensitive mixes fall to 67 settled lanes of 96).  Cases with other inputs, and why:
#   - th a cost row with th_dot an equality, 40/10 (four patterns): with spread 0.05 they have 75, 79, 74 and 81 settled lanes
#     of 96 and pull the share of the whole test to 94.7 %; with spread 0.03: 81, 94, 93, 96.
#   - the default rows at 20/10 and 20/5: with spread 0.05 80 and 86 settled lanes and one termination state up to 4
#     iterations; with spread 0.03: 95 and 92, mixed.
_TIGHT = dict(spread=0.03)
MIX_CASES = [Case(40, 10, p, **(_TIGHT if p[1] == "+" and p[3] == "-" else {})) for p in PATTERNS]
SHAPE_CASES = [Case(N, sp, p, **(_TIGHT if N == 20 and p == DEFAULT else {}))
               for (N, sp) in SHAPES for p in (ALL_COST, ALL_EQ, DEFAULT, TH_COST_THDOT_EQ)]
# Cases taken out because fewer than MIN_CASE_SHARE of their lanes are settled with every input tried (2 to 8 iterations;
# spread 0.05, 0.03, 0.02; seeds 61, 62, 63): (case id, why, largest distance of the two oracles on u over the inputs tried).
DROPPED = [
    ("20x10----", "44 to 66 settled lanes of 96 (2 to 8 iterations, three spreads, three seeds); 54 with the default inputs", 7.6e-3),
    ("20x5----", "44 to 62 settled lanes of 96 (2 to 8 iterations, three spreads, three seeds); 50 with the default inputs", 1e-4),
]
SHAPE_CASES = [c for c in SHAPE_CASES if c.id not in [d[0] for d in DROPPED]]

_CACHE = {}


def _key(*parts):
    out = []
    for p in parts:
        if isinstance(p, dict):
            out.append(tuple(sorted(p.items())))
        elif p is None or isinstance(p, (int, float, str)):
            out.append(p)
        elif hasattr(p, "_fields_"):
            out.append(bytes(p))
        else:
            a = np.ascontiguousarray(p, dtype=np.float64)
            out.append((a.shape, a.tobytes()))
    return tuple(out)


def _lane_over(over, terminal_weights, b):
    """OptimizationParams overrides of lane b: terminal_weights [nx, B] in state order, both poles alike."""
    if terminal_weights is None:
        return over
    w = terminal_weights[:, b]
    nq = w.size // 2
    assert (w[1:nq] == w[1]).all() and (w[nq + 1:] == w[nq + 1]).all(), "OptimizationParams has one weight for both poles"
    return dict(over, **dict(zip(NAMES, (float(w[0]), float(w[1]), float(w[nq]), float(w[nq + 1])))))


def settled(orc, over, dyn, set_point, x0, opts=None, terminal_weights=None, rows=None, model="double"):
    """The double oracle's cold step and where it can be trusted to 1e-7: -> ((u [N, B], pred [N, 6, B], status [B],
    iters [B]), settled mask [B], distance of the two oracles on u [B], the extended-precision u [N, B]).
    dyn [6] or [6, B], set_point a float or [B], terminal_weights None or [6, B] with both poles alike: with any of them per
    problem every lane is solved by an oracle built for that lane alone, from its own OptimizationParams.  rows: None or
    terminal weights [6, B] whose poles may differ, through the per-row override (oracle.step_batch_cold_rows; shared dyn and
    set_point).  opts: oracle SolverOpts.  model: "double" (6 states) or "single" (4: tests/helpers/limits_parity.py).  Cached
    per process on the values of all arguments; the arrays are read-only."""
    key = _key(over, dyn, set_point, x0, opts, terminal_weights, rows, model)
    if key in _CACHE:
        return _CACHE[key]
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    dyn = np.asarray(dyn, dtype=np.float64)
    per_problem = dyn.ndim == 2 or np.ndim(set_point) == 1 or terminal_weights is not None
    if rows is not None:
        assert not per_problem
        p = orc.default_opt_params(**over)
        u, pred, st, it, _ = orc.step_batch_cold_rows(p, dyn, set_point, x0, rows, opts=opts, want_pred=True, model=model)
        u_ld, st_ld, it_ld, _, _ = orc.step_batch_cold_rows_ld(p, dyn, set_point, x0, rows, opts=opts, model=model)
    elif not per_problem:
        p = orc.default_opt_params(**over)
        u, pred, st, it, _ = orc.step_batch_cold(p, dyn, set_point, x0, opts=opts, want_pred=True, model=model)
        u_ld, st_ld, it_ld, _, _ = orc.step_batch_cold_ld(p, dyn, set_point, x0, opts=opts, model=model)
    else:
        lanes, lanes_ld = [], []
        for b in range(x0.shape[1]):
            p = orc.default_opt_params(**_lane_over(over, terminal_weights, b))
            d = dyn[:, b] if dyn.ndim == 2 else dyn
            s = float(set_point[b]) if np.ndim(set_point) == 1 else set_point
            lanes.append(orc.step_batch_cold(p, d, s, x0[:, b:b + 1], opts=opts, want_pred=True, model=model)[:4])
            lanes_ld.append(orc.step_batch_cold_ld(p, d, s, x0[:, b:b + 1], opts=opts, model=model)[:3])
        u, pred, st, it = (np.concatenate([l[i] for l in lanes], axis=-1) for i in range(4))
        u_ld, st_ld, it_ld = (np.concatenate([l[i] for l in lanes_ld], axis=-1) for i in range(3))
    dist = np.abs(u - u_ld).max(axis=0)
    with np.errstate(invalid="ignore"):
        mask = (st == st_ld) & (it == it_ld) & (dist <= SETTLED_TOL)
    res = ((u, pred, st, it), mask, dist, u_ld)
    for a in (u, pred, st, it, mask, dist, u_ld):
        a.setflags(write=False)
    _CACHE[key] = res
    return res


def assert_shares(masks, what):
    """The two conditions on the reference alone: MIN_CASE_SHARE of every case, MIN_TEST_SHARE over the whole test.
    masks: {case id: settled mask} -> the share over the test."""
    for name, m in masks.items():
        assert m.mean() >= MIN_CASE_SHARE, "%s, case %s: %d of %d lanes settled" % (what, name, m.sum(), m.size)
    total = sum(int(m.sum()) for m in masks.values()) / sum(m.size for m in masks.values())
    assert total >= MIN_TEST_SHARE, "%s: %.4f of the lanes settled" % (what, total)
    return total


# ---------------------------------------------------------------------------------------------------------------------------
# the other tests' inputs, each drawn once from the seed written here
# ---------------------------------------------------------------------------------------------------------------------------
PP_SEED = 62
PP_WEIGHTS_SPREAD = 0.03
PP_OVER = {"default": dict(OVER, max_iterations=3), "soft": dict(OVER, max_iterations=3, **SOFT)}


def per_problem_inputs():
    """x0, dyn [6, B] (the first five parameters times uniform(0.8, 1.25)), set_point [B] in +-0.1, and terminal weights
    [6, B]: magnitudes 10 ** uniform(0, 2.3), each of the four classes an equality with probability 1/2, the poles alike.
    The terminal weights go with the states x0_of(PP_SEED, spread=0.03): with the spread 0.05 of x0 91 of the 96 lanes are
    settled after 3 iterations (94.8 %: under MIN_TEST_SHARE), with 0.03 93."""
    rng = np.random.default_rng(PP_SEED)
    x0 = near_upright(rng, B, 0.05)
    x0[0] *= 0.2
    x0[3:] *= 0.2
    dyn = np.tile(np.array(DYN).reshape(6, 1), (1, B))
    dyn[:5] *= rng.uniform(0.8, 1.25, (5, B))
    sp = rng.uniform(-0.1, 0.1, B)
    w = 10.0 ** rng.uniform(0, 2.3, (4, B))
    w[rng.random((4, B)) < 0.5] = -1.0
    return x0, dyn, sp, rows_of(w)


def pole_rows():
    """Weights that differ between the two poles, on the all-cost mix: th1 a cost row with th2 an equality on the even lanes
    and the reverse on the odd ones; th1_dot / th2_dot likewise with the halves swapped lane by lane in blocks of two."""
    rows = np.tile(rows_of(WEIGHTS).reshape(6, 1), (1, B))
    lane = np.arange(B)
    rows[1, lane % 2 == 1] = -1.0
    rows[2, lane % 2 == 0] = -1.0
    rows[4, (lane // 2) % 2 == 1] = -1.0
    rows[5, (lane // 2) % 2 == 0] = -1.0
    return rows


POLE_OVER = dict(OVER, max_iterations=3, **mix(ALL_COST))
POLE_SEED = 63

# (the retraction limits and the damping ladder: tests/helpers/limits_parity.py)
OPTION_SETS = [dict(ls_alpha_growth=2.0, ls_alpha_growth_backtracked=1.0), dict(ls_alpha_growth=0.0),
               dict(ls_shrink_max=0.7, ls_shrink_min=0.2, armijo_c1=1e-2, max_line_search_iterations=3,
                    lambda_failure_init=1.0, penalty_rho=0.5)]          # tests/test_gpu_parity.py
OPTION_OVER = dict(OVER, max_iterations=3)
OPTION_SEED = 64

EDGE_BATCHES = [(N, sp, nB) for (N, sp) in ((40, 10), (40, 8)) for nB in (1, 65, 127)]
EDGE_SEED = 65


def edge_over(N, sp):
    return dict(OVER, window_length=N, state_spacing=sp, max_iterations=4)


WARM_OVER = dict(OVER, max_iterations=3)
WARM_B, WARM_MAX_BATCH, WARM_SEEDS, WARM_LANES = 80, 128, (66, 67), 16


def warm_reference(orc):
    """Two steps of one controller per lane, cold from x0 and warm from x1, for the first WARM_LANES lanes: the double
    Optimization and the extended-precision one, each warm-started from its own first solution -> (u of the warm step
    [N, lanes], status [lanes], mask of the lanes settled in both steps)."""
    key = "warm"
    if key not in _CACHE:
        p = orc.default_opt_params(**WARM_OVER)
        x0, x1 = (x0_of(s, WARM_B) for s in WARM_SEEDS)
        u2, st2, mask = [], [], []
        for b in range(WARM_LANES):
            o, l = orc.Optimization(p, model="double"), orc.OptimizationLd(p, model="double")
            ok = True
            for x in (x0, x1):
                a, (u_ld, st_ld, it_ld) = o.step(x[:, b], DYN, SET_POINT), l.step(x[:, b], DYN, SET_POINT)
                s = a.solver_outputs
                ok = ok and s.termination_state == st_ld and s.iterations == it_ld and np.abs(a.u - u_ld).max() <= SETTLED_TOL
            u2.append(a.u)
            st2.append(s.termination_state)
            mask.append(ok)
        _CACHE[key] = (np.stack(u2, axis=1), np.array(st2), np.array(mask))
    return _CACHE[key]
