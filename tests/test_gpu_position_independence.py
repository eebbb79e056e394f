"""Batch-position independence, bitwise, for every SQP kernel form.

A problem's arithmetic must not depend on where it sits in the batch: staging compacts the active problems through an atomic
counter (the order of that list is arbitrary), a sharded handle gives a problem another position in each shard, and the HIP
graph replay relies on it.  So the same 77 problems are solved in natural order, reversed, rotated by one, shuffled, as the
prefixes of 1 and 13 problems, on a handle whose workspace stride is not the batch, and (fused pipeline) staged with a
compaction in between -- and every output of every problem must have the SAME BITS each time, cold and warm.  No reference and
no tolerance: the check is exact in float32 too.

B = 77 is odd -- a multiple of none of the problems-per-wave counts 32, 16, 12, 8, 6, 4 -- with two full waves and a ragged tail
at L = 2 and 19 waves plus one problem at L = 16.  With max_iterations = 8 and the default exit tolerances the problems stop at
different iterations, so the wave-uniform loops must freeze finished problems while their neighbours go on; every case asserts
that its natural-order run is mixed in that way (_assert_mixed) before it compares anything.

Case list against launch_fused (csrc/engine_impl.hpp): the seven compiled (L, SP) pairs and the six run-time-spacing interval
counts all appear for the 4-state model, each in its SHARED, per-problem and REFINE / WIDE instantiations and both dtypes; no
entry is left out (set_pipeline("fused") raises ERR_UNSUPPORTED for none of the shapes below).  The 6-state model runs the same
five forms at five of the compiled pairs, shapes that test_gpu_double.py::test_double_fused_layouts_across_shapes shows built."""
import numpy as np
import pytest

from conftest import DYN_UI, random_states
from helpers import batch_position as bp
from test_gpu_round6 import DYN_D, near_upright

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = 77
CAP = 8                      # max_iterations; the exit tolerances stay the defaults
SHUFFLE_SEED = 11
PREFIXES = (1, 13)
MODELS = {"single": dict(nx=4, dyn=DYN_UI, x0_seed=2026), "double": dict(nx=6, dyn=DYN_D, x0_seed=2027)}
# Another seed for x0 where the model's own misses the precondition (_assert_mixed) on the GPU, per (model, N, spacing) and
# shared by every form of the shape.  With seed 2027 the float64 and the wide float32 6-state kernels reproduce the CPU check's
# iteration counts exactly (40/10: 1, 2, 5, 7 and 73 x 8), but the float32 kernels with wide_qp off -- the SHARED form needs
# that -- stop early on one problem of 77 at 40/10 and 40/5 and on three with one count at 20/10.  Seed 2028 is the next one at
# which all forms of these shapes are mixed (fused, split and the derivative test's handles; measured on an MI355X).
X0_SEED = {("double", 40, 10): 2028, ("double", 40, 5): 2028, ("double", 20, 10): 2028}

# the forms of a shape: (dtype, per-problem inputs, wide_qp, refine_qp)
FORMS = {
    "f32-shared": (torch.float32, False, False, None),   # dyn a list: the SHARED instantiation (6-state: needs wide_qp off)
    "f32-per-problem": (torch.float32, True, False, None),
    "f32-wide": (torch.float32, True, True, None),
    "f64-plain": (torch.float64, True, None, False),
    "f64-refine": (torch.float64, True, None, True),
}
FUSED_SHAPES = {
    # 4-state: the compiled specialisations (N, spacing) -> (L, SP) = (4,10) (8,5) (2,10) (4,5) (2,20) (5,8) (10,4) ...
    "single": [(40, 10), (40, 5), (20, 10), (20, 5), (40, 20), (40, 8), (40, 4),
               # ... and the run-time-spacing kernel, one shape per interval count L = 2, 4, 5, 8, 10, 16
               (30, 15), (16, 4), (30, 6), (8, 1), (30, 3), (80, 5)],
    "double": [(40, 10), (40, 5), (20, 10), (20, 5), (40, 8)],
}
SPLIT_SHAPES = {"single": [(40, 10), (40, 8), (21, 7)],     # 21/7: three intervals, no fused kernel, linearize_dyn_kernel
                "double": [(40, 10), (40, 8)]}
SPLIT_FORMS = {"f32-plain": (torch.float32, False, False, None), "f32-wide": (torch.float32, False, True, None),
               "f64-per-problem": (torch.float64, True, None, None)}

STEP_FIELDS = ("u", "predicted_states", "status", "iterations", "ls_evals", "final_cost", "final_eq_l1", "guess")


def _terminal_defaults(params, nx):
    """The handle's terminal weights in state order (csrc/engine_impl.hpp: fill_args)."""
    nq = nx // 2
    return np.array([params.b_x_final_cost_weight if t == 0 else params.th_final_cost_weight if t < nq
                     else params.b_x_dot_final_cost_weight if t == nq else params.th_dot_final_cost_weight for t in range(nx)])


_INPUTS = {}


def _inputs(pkg, model, seed):
    """The 77 problems of a model, drawn once per seed (float64, on the host; never modified): x0, and the per-problem dyn,
    set_point, terminal_weights that are permuted together with it."""
    if (model, seed) not in _INPUTS:
        m = MODELS[model]
        rng = np.random.default_rng(seed)
        if model == "single":
            x0 = random_states(rng, B)
            x0[1, ::3] = np.pi / 2 + rng.uniform(-0.3, 0.3, x0[1, ::3].shape)
        else:
            x0 = near_upright(rng, B, spread=0.15)
        rng = np.random.default_rng(seed + 100)     # the per-problem inputs: a generator of their own
        dyn = np.array(m["dyn"]).reshape(-1, 1) * rng.uniform(0.8, 1.2, (len(m["dyn"]), B))
        sp = rng.uniform(-0.2, 0.2, B)
        tw = _terminal_defaults(pkg.default_params(), m["nx"]).reshape(-1, 1) * rng.uniform(0.5, 2.0, (m["nx"], B))
        _INPUTS[model, seed] = dict(x0=torch.tensor(x0), dyn=torch.tensor(dyn), set_point=torch.tensor(sp),
                                    terminal_weights=torch.tensor(tw))
    return _INPUTS[model, seed]


def _arranged(t, idx, dtype):
    return bp.take(t.to(dtype), idx).to(DEV)


def _make(pkg, model, N, sp, form, max_batch, pipeline):
    dtype, _, wide, refine = form
    opt = pkg.BatchOptimization(pkg.default_params(window_length=N, state_spacing=sp, max_iterations=CAP), max_batch=max_batch,
                                dtype=dtype, device=0, model=model, wide_qp=wide, refine_qp=refine)
    if pipeline is not None:
        opt.set_pipeline(pipeline)
        assert opt.pipeline() == pipeline
    if wide is not None:
        assert opt.wide_qp == wide
    if refine is not None:
        assert opt.refines_qp == refine
    return opt


def _step_inputs(pkg, model, N, sp, form, idx):
    """(cold x0, warm x0, keyword arguments of step()) of the arrangement idx."""
    dtype, per_problem = form[0], form[1]
    inp = _inputs(pkg, model, X0_SEED.get((model, N, sp), MODELS[model]["x0_seed"]))
    x0 = inp["x0"].to(dtype)
    kw = dict(dyn=MODELS[model]["dyn"], set_point=0.0, terminal_weights=None)
    if per_problem:
        kw = {k: _arranged(inp[k], idx, dtype) for k in ("dyn", "set_point", "terminal_weights")}
    return _arranged(x0, idx, dtype), _arranged(x0 + 0.01, idx, dtype), kw


def _run(pkg, model, N, sp, form, idx, max_batch=B, pipeline="fused", compaction=(0, 0), after_cold=None):
    """Two steps on a fresh handle with the problems idx: cold, then warm from x0 + 0.01 (the previous solution sits in the
    workspace in the arrangement's order).  -> [{output name: tensor}] per step, in the arrangement's order; after_cold
    (opt, arranged cold x0, step keywords) may add entries to the cold step's."""
    opt = _make(pkg, model, N, sp, form, max_batch, pipeline)
    opt.set_compaction(*compaction)
    x_cold, x_warm, kw = _step_inputs(pkg, model, N, sp, form, idx)
    res = []
    for x in (x_cold, x_warm):
        o = opt.step(x, kw["dyn"], kw["set_point"], want_predicted=True, want_stats=True, want_guess=True,
                     out=pkg.BatchOutputs(), terminal_weights=kw["terminal_weights"])
        r = {f: getattr(o, f) for f in STEP_FIELDS}
        r["solution"] = opt.get_solution(len(idx))
        if after_cold is not None and not res:
            r.update(after_cold(opt, x, kw))
        res.append(r)
    if compaction != (0, 0):
        assert len(opt.stage_plan()) > 2, opt.stage_plan()     # several launches, a compaction between them
    torch.cuda.synchronize()
    opt.close()
    return res


def _assert_mixed(ref, L):
    """The precondition of a case, on the cold natural-order run: problems stop at different iterations, inside one wave too,
    so that no case passes emptily; and every output of the run is finite."""
    for step in ref:
        for name, t in step.items():
            assert bool(torch.isfinite(t).all()) if t.is_floating_point() else True, name
    its, ls = ref[0]["iterations"].cpu().numpy(), ref[0]["ls_evals"].cpu().numpy()
    assert len(set(its.tolist())) >= 3, np.bincount(its)
    assert int((its < CAP).sum()) >= 3, np.bincount(its)
    ppw = 64 // L
    assert any(len(set(its[w:w + ppw].tolist())) > 1 for w in range(0, B, ppw)), its
    assert len(set(ls.tolist())) >= 2, np.bincount(ls)


def _assert_same_bits(ref, got, idx, L, what):
    """Every output of both steps of an arrangement against the natural-order reference, bit for bit."""
    full = len(idx) == B
    assert len(ref) == len(got) == 2
    for tick, (want, have) in enumerate(zip(ref, got)):
        assert sorted(want) == sorted(have)
        if full and not np.array_equal(idx, np.arange(B)):   # the arrangement did move the problems
            assert not torch.equal(want["u"], have["u"])
        for name in want:
            a = want[name] if full else want[name][..., :len(idx)].contiguous()
            b = bp.put_back(have[name], idx) if full else have[name]
            msg = bp.first_difference(a, b, L, idx=idx, name="%s, %s step, %s" % (what, ("cold", "warm")[tick], name))
            assert msg is None, msg


def _check_case(pkg, model, N, sp, form, pipeline, L, staged):
    natural = np.arange(B)
    ref = _run(pkg, model, N, sp, form, natural, pipeline=pipeline)
    _assert_mixed(ref, L)
    perms = bp.permutations(B, SHUFFLE_SEED)
    for name, idx in perms.items():
        _assert_same_bits(ref, _run(pkg, model, N, sp, form, idx, pipeline=pipeline), idx, L, name)
    for n in PREFIXES:
        idx = np.arange(n)
        _assert_same_bits(ref, _run(pkg, model, N, sp, form, idx, pipeline=pipeline), idx, L, "prefix of %d" % n)
    _assert_same_bits(ref, _run(pkg, model, N, sp, form, natural, max_batch=2 * B + 3, pipeline=pipeline), natural, L,
                      "workspace stride 2 B + 3")
    if staged:
        for name, compaction in (("reverse", (2, 1)), ("shuffle", (1, 3))):
            got = _run(pkg, model, N, sp, form, perms[name], pipeline=pipeline, compaction=compaction)
            _assert_same_bits(ref, got, perms[name], L, "%s staged %d + %d" % ((name,) + compaction))


def _ids(shapes, forms):
    return [pytest.param(model, N, sp, f, id="%s-%dx%d-%s" % (model, N, sp, f))
            for model in ("single", "double") for (N, sp) in shapes[model] for f in forms]


@pytest.mark.parametrize("model,N,sp,form", _ids(FUSED_SHAPES, FORMS))
def test_fused_kernels_do_not_depend_on_the_batch_position(pkg, model, N, sp, form):
    """fused_sqp_kernel / fused_sqp_dyn_kernel: all eight arrangements, the staged ones included."""
    _check_case(pkg, model, N, sp, FORMS[form], "fused", N // sp, staged=True)


@pytest.mark.parametrize("model,N,sp,form", _ids(SPLIT_SHAPES, SPLIT_FORMS))
def test_split_kernels_do_not_depend_on_the_batch_position(pkg, model, N, sp, form):
    """linearize_kernel / linearize_dyn_kernel ((problem, interval) -> thread by gid / B) and qp_ls_kernel, plain and wide, one
    lane per problem: the unstaged arrangements."""
    _check_case(pkg, model, N, sp, SPLIT_FORMS[form], "split", 1, staged=False)


def _derivative_calls(N, gbar):
    """after_cold of _run: the four plan-derivative calls at the handle's own solution (z=None: read at the workspace stride)."""
    def calls(opt, x0, kw):
        dyn, tw = kw["dyn"], kw["terminal_weights"]
        res = {"feedback_gain": opt.feedback_gain(dyn, n_rows=N, terminal_weights=tw)}
        for k, v in opt.plan_sensitivity(dyn, n_rows=N, terminal_weights=tw).items():
            res["plan_sensitivity." + k] = v
        for k, v in opt.plan_vjp(dyn, gbar, terminal_weights=tw).items():
            res["plan_vjp." + k] = v
        for k, v in opt.plan_weight_vjp(x0, dyn, gbar, set_point=kw["set_point"], terminal_weights=tw, want_du=True).items():
            res["plan_weight_vjp." + k] = v
        return res
    return calls


@pytest.mark.parametrize("model,N,sp", [("single", 40, 10), ("single", 20, 5), ("double", 40, 10)])
@pytest.mark.parametrize("form", ["f32-per-problem", "f32-wide", "f64-plain"])
def test_plan_derivative_calls_do_not_depend_on_the_batch_position(pkg, model, N, sp, form):
    """feedback_gain, plan_sensitivity, plan_vjp and plan_weight_vjp after the cold step, with per-problem inputs and a
    cotangent that moves with its problem: natural order, shuffled, and on a handle whose stride is not the batch."""
    f = FORMS[form]
    gbar = torch.tensor(np.random.default_rng(7).standard_normal((N, B)))
    natural, shuffle = np.arange(B), bp.permutations(B, SHUFFLE_SEED)["shuffle"]

    def run(idx, max_batch=B):
        return _run(pkg, model, N, sp, f, idx, max_batch=max_batch, pipeline=None,
                    after_cold=_derivative_calls(N, _arranged(gbar, idx, f[0])))
    ref = run(natural)
    assert len(ref[0]) == len(STEP_FIELDS) + 1 + 1 + 3 + 3 + 4
    _assert_mixed(ref, N // sp)
    _assert_same_bits(ref, run(shuffle), shuffle, 1, "shuffle")
    _assert_same_bits(ref, run(natural, max_batch=2 * B + 3), natural, 1, "workspace stride 2 B + 3")
