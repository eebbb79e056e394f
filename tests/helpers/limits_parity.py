"""Cases and references of the SQP parity tests with the retraction limits and the damping ladder live, float64.

One table for tests/test_limits_parity_cases.py (CPU: is the reference fit to compare against, and are the clamps and the
ladder really at work in it?) and tests/test_gpu_limits_parity.py (GPU: do the kernels agree with it?).  numpy and the oracle
only: no torch here.

Every SQP kernel clamps its trial and accepted iterates -- node positions b_x to +-b_x_limit, controls to +-u_limit -- and
carries the Levenberg-Marquardt ladder (lambda_initial, lambda_scale_up, lambda_scale_down, lambda_min, lambda_max;
cpmpc_solver_opts).  With the defaults (5.0, 300.0, a ladder from 1e-2 to 1e6) the clamps are dead code on nearly every lane
and the ladder is climbed from one starting rung only, so the option sets below pull the limits into the solution and move
every rung.  Settled lanes, SETTLED_TOL and assert_shares are those of tests/helpers/double_parity.py.

LAMBDA_MAX ON A RUNG.  The exit test is `lambda > lambda_max` after the multiply.  With lambda_max = 10 and the default rungs
1e-2 * 10^k the double oracle reaches exactly 10.0 and goes on, the extended-precision one reaches 10.000...02 and stops an
iteration earlier: an artefact of the comparison, not a defect, and the reason every lambda_max here lies strictly between
rungs (rungs_of, asserted in tests/test_limits_parity_cases.py).

Inputs.  4-state: random_states(default_rng(7), 192), DYN_UI, set-point 0.05, 8 iterations with the default exits.  6-state:
double_parity.x0_of(61) (near_upright, spread 0.05), double_parity.DYN, set-point 0.02, 4 iterations, sinusoid amplitude 0."""
import numpy as np

from conftest import DYN_UI, random_states
from helpers import double_parity as dp

SETS = {
    "A": dict(u_limit=8.0, lambda_max=30.0),
    "B": dict(u_limit=12.0, b_x_limit=0.4),
    "C": dict(u_limit=20.0, lambda_initial=3.0, lambda_scale_up=4.0, lambda_scale_down=0.5, lambda_min=0.2, lambda_max=150.0),
    "D": dict(b_x_limit=0.3, u_limit=15.0, max_line_search_iterations=2, lambda_failure_init=0.7, lambda_max=500.0),
    "A6": dict(u_limit=2.0),
    "B6": dict(u_limit=1.0, b_x_limit=0.05),
    # C's ladder with u_limit = 3.0.  Measured on the CPU at 40/10, 40/5 and 30/6: 33, 31 and 40 % of the 96 lanes end on the
    # limit, with 17, 17 and 6 lanes in SATISFIED_RELATIVE_TOL next to MAX_ITERATIONS: this u_limit stands, no other was tried
    "C6": dict(u_limit=3.0, lambda_initial=3.0, lambda_scale_up=4.0, lambda_scale_down=0.5, lambda_min=0.2, lambda_max=150.0),
}
# LAMBDA_MIN ON A RUNG.  `lambda < lambda_min -> 0` written as `<=` goes unnoticed with set C: its ladder 3, 1.5, 0.75, 0.375,
# 0.1875 never lands on 0.2 (a kernel library mutated in that way passed every case of sets A to D and A6 to C6).  Sets E and
# E6 are C and C6 with lambda_min = 0.375 = the rung 0.75 times scale_down, exact in every binary format: with `<` the ladder
# and so the whole reference are C's, bit for bit; with `<=` lambda drops to 0 one accepted step earlier and most lanes end
# elsewhere (tests/test_limits_parity_cases.py asserts both).
SETS["E"] = dict(SETS["C"], lambda_min=0.375)
SETS["E6"] = dict(SETS["C6"], lambda_min=0.375)
LOWERS_B_X = ("B", "D", "B6")                     # the sets that lower b_x_limit
LADDER_SETS = ("A", "C", "D", "E")                # the 4-state sets that must show two termination states, MAX_LAMBDA at 40/10
# shape -> what it reaches in the kernels (4-state)
SHAPES4 = [(40, 10), (40, 5), (20, 5), (40, 4), (30, 6), (21, 7), (80, 10)]
SPLIT_ONLY = [(21, 7)]                            # linearize_dyn_kernel: no fused kernel for 3 intervals
SHAPES6 = [(40, 10), (40, 5), (30, 6)]
B4, B6 = 192, 96
SEED4, SEED6 = 7, 61
SET_POINT4, SET_POINT6 = 0.05, dp.SET_POINT
ITERATIONS4, ITERATIONS6 = 8, 4
INSPECTED = 32                                    # lanes whose final z is looked at (one oracle.Optimization per lane)
MIN_SETTLED, MIN_AT_U_LIMIT, MIN_AT_B_X_LIMIT, MIN_STATE_LANES = 0.95, 0.20, 0.25, 3
PP_SEED = 5
REFINE_U_COST_WEIGHT = 0.01                       # below the library's 0.05: the REFINE instantiation is the default

_X0 = {}


def x0_single(seed=SEED4, B=B4):
    """random_states of a seed, drawn once and read-only."""
    if (seed, B) not in _X0:
        x0 = random_states(np.random.default_rng(seed), B)
        x0.setflags(write=False)
        _X0[seed, B] = x0
    return _X0[seed, B]


def per_problem_inputs(B=B4):
    """dyn [9, B] and set_point [B] of the per-problem case: masses and length times uniform(0.7 .. 1.3), frictions drawn,
    set-points in +-0.1 (tests/test_gpu_parity.py::test_per_problem_parameters_and_set_points, narrower set-points so that
    the limits stay live)."""
    rng = np.random.default_rng(PP_SEED)
    dyn = np.tile(np.array(DYN_UI).reshape(9, 1), (1, B))
    dyn[0] *= rng.uniform(0.7, 1.3, B)
    dyn[1] *= rng.uniform(0.7, 1.3, B)
    dyn[2] *= rng.uniform(0.8, 1.2, B)
    dyn[4] = rng.uniform(0.0, 0.2, B)
    dyn[6] = rng.uniform(0.0, 0.3, B)
    return dyn, rng.uniform(-0.1, 0.1, B)


class Case:
    """One problem definition, one option set and its inputs.  kind: "" (shared dyn and set-point), "pp" (per-problem dyn and
    set-points: the non-SHARED instantiation), "refine" (u_cost_weight = 0.01: the REFINE instantiation)."""

    def __init__(self, model, N, sp, set_name, kind="", moved=None, inspect="first"):
        """moved: limits of the set that this case moves (the table says why).  inspect: which INSPECTED lanes at_limits
        looks at: "first", or "far" = those whose cart starts farthest from the centre, from x0 alone."""
        self.model, self.N, self.sp, self.set_name, self.kind = model, N, sp, set_name, kind
        self.moved, self.inspect = dict(moved or {}), inspect
        self.B = B4 if model == "single" else B6
        self.nx = 4 if model == "single" else 6

    @property
    def id(self):
        return "%dx%d-%s%s" % (self.N, self.sp, self.set_name, "-" + self.kind if self.kind else "")

    @property
    def sopts(self):
        return dict(SETS[self.set_name], **self.moved)

    @property
    def inspected(self):
        """The lanes at_limits looks at, chosen from the inputs alone."""
        if self.inspect == "first":
            return np.arange(INSPECTED)
        return np.sort(np.argsort(-np.abs(self.x0[0]), kind="stable")[:INSPECTED])

    @property
    def over(self):
        o = dict(window_length=self.N, state_spacing=self.sp)
        if self.model == "single":
            o.update(max_iterations=ITERATIONS4)
            if self.kind == "refine":
                o.update(u_cost_weight=REFINE_U_COST_WEIGHT)
        else:
            o.update(dp.OVER, max_iterations=ITERATIONS6)
        return o

    @property
    def x0(self):
        return x0_single() if self.model == "single" else dp.x0_of(SEED6, B6, 0.05)

    @property
    def dyn(self):
        if self.kind == "pp":
            return per_problem_inputs(self.B)[0]
        return DYN_UI if self.model == "single" else dp.DYN

    @property
    def set_point(self):
        if self.kind == "pp":
            return per_problem_inputs(self.B)[1]
        return SET_POINT4 if self.model == "single" else SET_POINT6

    @property
    def pipelines(self):
        return ("split",) if (self.N, self.sp) in SPLIT_ONLY else ("fused", "split")

    def amplitude(self, orc):
        """The cold guess's sinusoid amplitude: the largest |u| of a lane that never accepts a step."""
        return orc.default_opt_params(**self.over).u_guess_sinusoid_amplitude

    def reference(self, orc):
        """double_parity.settled of the case: ((u, pred, status, iters), settled mask, distance, extended-precision u)."""
        return dp.settled(orc, self.over, self.dyn, self.set_point, self.x0, opts=orc.default_solver_opts(**self.sopts),
                          model=self.model)

    def at_limits(self, orc):
        return at_limits(orc, self)


# THE TABLE.  No case is dropped and no seed moved.  Measured on the CPU with the inputs above: every lane of every case is
# settled but one (30/6 C6: 95 of 96); 26 to 98 % of a case's lanes end with a control on the limit; MAX_LAMBDA holds 5 to
# 176 lanes of every A, C and D case but 80/10 C.  Cases that move a limit of their set, or the inspected lanes, and why:
#   - 20/5 D and 21/7 D: b_x_limit 0.1, not 0.3.  On a 0.2 s horizon with two line-search trials 173 and 168 of the 192 lanes
#     reject every step and stay at the unclamped guess; 6 and 7 of the 32 inspected lanes have a node on 0.3 (19 and 22 %;
#     seeds 8 and 9: 22 to 28 %; 0.25 and 0.2: 22 and 25 %).  With 0.1: 10 and 11 of 32, MAX_ITERATIONS 16 / 22 lanes.
#   - 80/10 C: u_limit 12, not 20.  With 20 (and 30; seeds 7, 8, 9) 191 or 192 lanes end in MAX_ITERATIONS, so the case had
#     one termination state; with 12: MAX_ITERATIONS 186, SATISFIED_RELATIVE_TOL 4, MAX_LAMBDA 2, 94 % of lanes on the limit.
#   - B6 (all shapes): the inspected lanes are the 32 whose cart starts farthest from the centre.  x0[0] is uniform in
#     +-0.06 and the cart moves less than 0.02 in 4 iterations over 0.4 s, so only a lane that starts next to 0.05 can end on
#     it: 13, 13 and 15 of the 96 lanes do whatever the seed (60 to 79: 0 to 7 of the first 32) or the limit (0.01 to 0.15:
#     fewer; a lane that starts beyond the limit rejects every step), too few among the first 32 (5, 5, 8).  Of the 32
#     farthest: 9, 9 and 14.
_SHORT_D = dict(b_x_limit=0.1)
_MOVED = {(20, 5, "D"): _SHORT_D, (21, 7, "D"): _SHORT_D, (80, 10, "C"): dict(u_limit=12.0)}
CASES4 = [Case("single", N, sp, s, moved=_MOVED.get((N, sp, s))) for (N, sp) in SHAPES4 for s in "ABCD"]
SITE_CASES = [Case("single", 40, 10, "A", "pp"), Case("single", 40, 10, "A", "refine")]
CASES6 = [Case("double", N, sp, s, inspect="far" if s == "B6" else "first") for (N, sp) in SHAPES6 for s in ("A6", "B6", "C6")]
RUNG_CASES = [Case("single", 40, 10, "E"), Case("double", 40, 10, "E6")]
ALL_CASES = CASES4 + SITE_CASES + CASES6 + RUNG_CASES


def u_at_limit(u, u_limit):
    """u [N, B] -> mask [B] of the lanes with a control exactly on +-u_limit."""
    return (np.abs(u) == u_limit).any(axis=0)


def nodes_at_limit(z, nx, S, b_x_limit):
    """z [dim, lanes] -> mask [lanes] of the lanes with a node position (state 0 of a node) exactly on +-b_x_limit."""
    return (np.abs(z[0:nx * S:nx]) == b_x_limit).any(axis=0)


_LIMITS = {}


def at_limits(orc, case):
    """From the oracle's final z of the lanes case.inspected (one Optimization per lane, cold): -> (mask [lanes] of the lanes
    with a node b_x exactly on +-b_x_limit, mask [lanes] of those with a control exactly on +-u_limit, z [dim, lanes])."""
    lanes = case.inspected
    assert lanes.size <= INSPECTED
    if (case.id, case.model) not in _LIMITS:
        o = orc.default_solver_opts(**case.sopts)
        p = orc.default_opt_params(**case.over)
        dyn, sp, zs = np.asarray(case.dyn, dtype=np.float64), case.set_point, []
        for b in lanes:
            out = orc.Optimization(p, opts=o, model=case.model).step(
                case.x0[:, b], dyn[:, b] if dyn.ndim == 2 else dyn, float(sp[b]) if np.ndim(sp) == 1 else sp)
            zs.append(out.z)
        z = np.stack(zs, axis=1)
        S = case.N // case.sp + 1
        assert z.shape[0] == case.nx * S + case.N
        res = (nodes_at_limit(z, case.nx, S, o.b_x_limit), u_at_limit(z[case.nx * S:], o.u_limit), z)
        for a in res:
            a.setflags(write=False)
        _LIMITS[case.id, case.model] = res
    return _LIMITS[case.id, case.model]


def histogram(orc, status):
    """{termination state's name: lanes}."""
    return {orc.TERM_NAMES[int(k)]: int(v) for k, v in zip(*np.unique(status, return_counts=True))}


def rungs_of(o, iterations=8):
    """Every value of lambda the ladder of the oracle SolverOpts o can take in `iterations` iterations, each of which
    multiplies once: lambda_failure_init * scale_up^k after k + 1 failures, and lambda_initial * scale_up^j * scale_down^k
    after j failures and k accepted steps, j + k <= iterations (the zeros left out)."""
    r = [o.lambda_failure_init * o.lambda_scale_up ** k for k in range(iterations)]
    r += [o.lambda_initial * o.lambda_scale_up ** j * o.lambda_scale_down ** k
          for j in range(iterations + 1) for k in range(iterations + 1 - j)]
    return np.array(sorted({v for v in r if v > 0.0}))


# ---------------------------------------------------------------------------------------------------------------------------
# warm steps: set B, two ticks of one controller per lane
# ---------------------------------------------------------------------------------------------------------------------------
WARM_SET, WARM_LANES = "B", 16
WARM_SEEDS = {"single": (7, 8), "double": (61, 66)}
WARM_SETS = {"single": "B", "double": "B6"}


def warm_case(model):
    return Case(model, 40, 10, WARM_SETS[model])


def warm_states(model):
    c = warm_case(model)
    if model == "single":
        return tuple(x0_single(s, c.B) for s in WARM_SEEDS[model])
    return tuple(dp.x0_of(s, c.B, 0.05) for s in WARM_SEEDS[model])


def warm_reference(orc, model):
    """Two steps of one controller per lane, cold from x0 and warm from x1, for the first WARM_LANES lanes: the double
    Optimization and the extended-precision one, each warm-started from its own first solution (double_parity.warm_reference
    with solver options) -> (u of the warm step [N, lanes], status [lanes], iterations [lanes], mask of the lanes settled in
    both steps, mask of the lanes whose FIRST solution has a control on the limit, z of the warm step [dim, lanes])."""
    key = ("warm", model)
    if key not in dp._CACHE:
        c = warm_case(model)
        p, o = orc.default_opt_params(**c.over), orc.default_solver_opts(**c.sopts)
        xs = warm_states(model)
        u2, st2, it2, mask, first, z2 = [], [], [], [], [], []
        for b in range(WARM_LANES):
            d, l = orc.Optimization(p, opts=o, model=model), orc.OptimizationLd(p, opts=o, model=model)
            ok = True
            for t, x in enumerate(xs):
                a, (u_ld, st_ld, it_ld) = d.step(x[:, b], c.dyn, c.set_point), l.step(x[:, b], c.dyn, c.set_point)
                s = a.solver_outputs
                ok = ok and s.termination_state == st_ld and s.iterations == it_ld and np.abs(a.u - u_ld).max() <= dp.SETTLED_TOL
                if t == 0:
                    first.append(bool((np.abs(a.u) == o.u_limit).any()))
            u2.append(a.u)
            z2.append(a.z)
            st2.append(s.termination_state)
            it2.append(s.iterations)
            mask.append(ok)
        dp._CACHE[key] = (np.stack(u2, axis=1), np.array(st2), np.array(it2), np.array(mask), np.array(first), np.stack(z2, axis=1))
    return dp._CACHE[key]
