"""Cases, inputs and runner shared by tests/test_gpu_fused_lds_order.py and tools/fused_lds_order_golden.py.

The fused SQP kernel's float 4-state instantiations read the controls of the linearisation and of the line search from LDS
one step ahead of the arithmetic that uses them (csrc/mpc_fused_body.inc: kUAhead).  That is a reordering of reads, never of
arithmetic, so every output keeps the bits it had before the change.  The fixture tests/golden/fused_lds_order.json holds a digest of each
output of each case below, recorded once from a build of the commit before the change; the test asserts equality of digests,
i.e. exact equality of the outputs.

Shapes: the (N, spacing) pairs give the Gamma accumulation's j-loop every trip count from 0 to 19 (spacing 20), odd and even,
with and without the remainder column, on the compiled kernels and (30, 6) on the run-time-spacing one.  Batches of 1, 17 and
65 problems leave partial waves at every problems-per-wave count.  Two runs per case: `cold`, three iterations with the exits
disabled from the benchmark's state distribution, and `warm`, a warm step of a handle with the exits enabled that has settled near
upright, where steps are tiny and taken without a merit evaluation (fewer line-search evaluations than iterations)."""
import hashlib

import numpy as np
import torch

DEV = "cuda:0"
DYN_UI = [1.0, 0.1, 0.25, 9.81, 0.05, 0.1, 0.02, 0.8, 100.0]
SHAPES = [(40, 10), (40, 5), (20, 10), (40, 8), (40, 4), (40, 20), (30, 6)]
BATCHES = (1, 17, 65)
ITERS = 3
WARM_UP_STEPS = 6      # steps of the warm handle before the recorded one: the plan has converged by then
FIELDS = ("u", "predicted_states", "status", "iterations", "ls_evals")
# form -> (dtype, per-problem dyn, wide_qp, parameter overrides, the handle must refine the whole QP)
FORMS = {
    "f32-shared": (torch.float32, False, False, {}, False),
    "f32-per-problem": (torch.float32, True, False, {}, False),
    "f32-wide": (torch.float32, True, True, {}, False),
    "f64-shared": (torch.float64, False, None, {}, False),
    "f64-per-problem": (torch.float64, True, None, {}, False),
    "f64-refine": (torch.float64, False, None, dict(u_cost_weight=0.01), True),   # below the library's 0.05: REFINE
}
RUNS = ("cold", "warm")


def case_id(N, sp, form):
    return "%dx%d-%s" % (N, sp, form)


def inputs():
    """Host float64 inputs of the largest batch; smaller batches take its first problems."""
    B = max(BATCHES)
    rng = np.random.default_rng(707)
    cold = np.stack([rng.uniform(-0.6, 0.6, B), rng.uniform(-np.pi, np.pi, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B)])
    upright = np.stack([rng.uniform(-0.05, 0.05, B), np.pi / 2 + rng.uniform(-0.02, 0.02, B), rng.uniform(-0.05, 0.05, B),
                        rng.uniform(-0.05, 0.05, B)])
    dyn = np.array(DYN_UI).reshape(-1, 1) * rng.uniform(0.8, 1.2, (len(DYN_UI), B))
    return dict(cold=cold, upright=upright, dyn=dyn)


def digest(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return "%s%s:%s" % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()[:16])


def run_case(pkg, inp, N, sp, form, B):
    """-> {run: {field: tensor}} of one case at batch B, on fresh handles, fused pipeline."""
    dtype, per_problem, wide, over, refines = FORMS[form]

    def handle(**exits):
        params = pkg.default_params(window_length=N, state_spacing=sp, max_iterations=ITERS, **over, **exits)
        opt = pkg.BatchOptimization(params, max_batch=B, dtype=dtype, device=0, wide_qp=wide)
        opt.set_pipeline("fused")
        assert opt.pipeline() == "fused"
        if wide is not None:
            assert opt.wide_qp == wide
        if dtype == torch.float64:
            assert opt.refines_qp == refines
        return opt

    def T(a):
        return torch.tensor(np.ascontiguousarray(a[..., :B]), dtype=dtype, device=DEV)

    dyn = T(inp["dyn"]) if per_problem else DYN_UI

    def step(opt, x0):
        o = opt.step(T(x0), dyn, 0.0, want_predicted=True, want_stats=True, out=pkg.BatchOutputs())
        return {f: getattr(o, f).clone() for f in FIELDS}

    res = {}
    opt = handle(relative_exit_tol=0.0, absolute_first_derivative_tol=0.0)
    res["cold"] = step(opt, inp["cold"])
    opt.close()
    opt = handle()
    for _ in range(WARM_UP_STEPS):
        step(opt, inp["upright"])
    res["warm"] = step(opt, inp["upright"] + 0.001)
    torch.cuda.synchronize()
    opt.close()
    return res
