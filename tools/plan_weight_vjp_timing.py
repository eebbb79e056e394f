"""Times the weight-gradient call of DESIGN.md section 5d beside what it is expected to cost, on cuda:0 with device events, 20
calls after 5 warm-ups, 262 144 4-state problems, fp32 and fp64, in one session: cpmpc_plan_weight_vjp_batch (the three
gradients and du) at n_rows = 1 and N, the three gradients alone and g_tw alone (no ascending pass) at n_rows = N,
cpmpc_plan_vjp_batch (three outputs) at n_rows = N, and one split-pipeline iteration (linearize + qp_ls) as the difference
between a whole step with max_iterations = 2 and one with max_iterations = 1 on split-pipeline handles with the exit tests
off.  z is the handle's solution after one cold-start step.  The expectation to confirm or refute: the call costs about
plan_vjp plus one qp_ls pass, being two passes over Phi, Gamma and Wk.  A report, not a test.  Prints one JSON line.
Usage: python tools/plan_weight_vjp_timing.py [--batch B]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_sensitivity_timing import DYN, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=262144)
    args = ap.parse_args()
    pkg = importlib.import_module("cart-pole-mpc_amd")
    capi = pkg.capi
    B, dev = args.batch, "cuda:0"
    rng = np.random.default_rng(7)
    xs = np.stack([rng.uniform(-0.3, 0.3, B), np.pi / 2 + rng.uniform(-0.4, 0.4, B), rng.uniform(-0.5, 0.5, B),
                   rng.uniform(-1, 1, B)])
    res = {"batch": B, "calls": 20, "warmup": 5}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        opt = pkg.BatchOptimization(pkg.default_params(), max_batch=B, dtype=dt, device=0)
        x0 = torch.tensor(xs, dtype=dt, device=dev)
        opt.step(x0, DYN, 0.0, want_predicted=False)
        x1 = x0 + 0.01
        N, nx = opt.N, opt.nx
        lib = capi.load()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        arr = capi.dbl_array(DYN, len(DYN))
        gin = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
        gin.dyn_shared_host = C.cast(arr, C.POINTER(C.c_double))
        win = capi.WeightVjpInputs(struct_size=C.sizeof(capi.WeightVjpInputs))
        win.lin.struct_size = C.sizeof(capi.GainInputs)
        win.lin.dyn_shared_host = C.cast(arr, C.POINTER(C.c_double))
        u_prev = torch.full((B,), 0.7, dtype=dt, device=dev)
        win.x0, win.set_point_shared, win.u_prev = x1.data_ptr(), 0.3, u_prev.data_ptr()
        gbar = torch.tensor(rng.uniform(-1, 1, (N, B)), dtype=dt, device=dev)
        g_tw, g_x0 = torch.empty((nx, B), dtype=dt, device=dev), torch.empty((nx, B), dtype=dt, device=dev)
        g_a, g_b = torch.empty((B,), dtype=dt, device=dev), torch.empty((B,), dtype=dt, device=dev)
        du = torch.empty((N, B), dtype=dt, device=dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev)
        pg, ptw, px0, pa, pb, pdu, pok = (C.c_void_p(t.data_ptr()) for t in (gbar, g_tw, g_x0, g_a, g_b, du, ok))

        def weight(n, tw=True, sums=True, with_du=True):
            capi.check(lib.cpmpc_plan_weight_vjp_batch(opt._h, B, C.byref(win), n, pg, ptw if tw else None,
                                                       pa if sums else None, pb if sums else None, pdu if with_du else None,
                                                       pok, stream))

        def vjp(n):
            capi.check(lib.cpmpc_plan_vjp_batch(opt._h, B, C.byref(gin), n, pg, px0, pa, pb, pok, stream))
        r = {"wide_qp": bool(opt.wide_qp)}
        for n in (1, N):
            r["plan_weight_vjp_all_outputs_rows_%d" % n] = timed(lambda: weight(n))
        r["plan_weight_vjp_gradients_rows_%d" % N] = timed(lambda: weight(N, with_du=False))
        r["plan_weight_vjp_terminal_only_rows_%d" % N] = timed(lambda: weight(N, sums=False, with_du=False))
        r["plan_vjp_rows_%d" % N] = timed(lambda: vjp(N))
        opt.close()
        steps = {}
        for iters in (1, 2):   # whole steps on the split pipeline, exit tests off: their difference is linearize + qp_ls
            h = pkg.BatchOptimization(pkg.default_params(max_iterations=iters, relative_exit_tol=0.0,
                                                         absolute_first_derivative_tol=0.0), max_batch=B, dtype=dt, device=0)
            h.set_pipeline("split")
            out = pkg.BatchOutputs()

            def step():
                h.reset()
                h.step(x0, DYN, 0.0, want_predicted=False, want_stats=False, out=out)
            steps[iters] = timed(step)
            h.close()
        r["split_step_1_iteration"], r["split_step_2_iterations"] = steps[1], steps[2]
        r["one_split_iteration_linearize_plus_qp_ls"] = {k: steps[2][k] - steps[1][k] for k in ("mean_ms", "min_ms")}
        res[name] = r
        del gbar, du, opt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
