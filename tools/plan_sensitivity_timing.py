"""Times the sensitivity calls of DESIGN.md section 5d on cuda:0 with device events, 20 calls after 5 warm-ups, 262 144
4-state problems, fp32 and fp64: cpmpc_plan_sensitivity_batch with all three outputs and cpmpc_feedback_gain_batch at
n_rows = 1 and N, cpmpc_plan_update_batch at n_rows = N, and beside them a settled closed-loop tick (300 untimed ticks, then
50 timed, as bench.py's closed_loop_settled).  Prints one JSON line.  Usage: python tools/plan_sensitivity_timing.py [--batch B]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DYN = [1.0, 0.1, 0.25, 9.81, 0.05, 0.1, 0.02, 0.8, 100.0]


def timed(fn, calls=20, warmup=5):
    """Mean and least milliseconds of `calls` calls of fn, each between its own pair of events."""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms))}


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
        sim = pkg.BatchSimulator(B, dtype=dt, device=0)
        sim.set_state(torch.tensor(xs, dtype=dt, device=dev))
        opt = pkg.BatchOptimization(pkg.default_params(), max_batch=B, dtype=dt, device=0)
        out = pkg.BatchOutputs()

        def tick():
            o = opt.step(sim.get_state(), DYN, 0.0, want_predicted=False, want_stats=True, out=out)
            sim.step(DYN, 0.01, o.u[0].contiguous())
        for _ in range(310):
            tick()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            tick()
        torch.cuda.synchronize()
        r = {"wide_qp": bool(opt.wide_qp), "settled_tick_ms": (time.perf_counter() - t0) / 50 * 1e3}
        # the C entry points themselves, every output and argument struct made before the clock: between two events there is
        # one ctypes call (a few microseconds of host time, hidden behind the kernels of the call before it)
        N, nx = opt.N, opt.nx
        lib, cdt = capi.load(), capi.F32 if dt == torch.float32 else capi.F64
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        arr = capi.dbl_array(DYN, len(DYN))
        inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
        inp.dyn_shared_host = C.cast(arr, C.POINTER(C.c_double))
        K = torch.empty((N, nx, B), dtype=dt, device=dev)
        k_sp, k_up = torch.empty((N, B), dtype=dt, device=dev), torch.empty((N, B), dtype=dt, device=dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev)
        pK, psp, pup, pok = (C.c_void_p(t.data_ptr()) for t in (K, k_sp, k_up, ok))

        def sens(n, a, b, c):
            capi.check(lib.cpmpc_plan_sensitivity_batch(opt._h, B, C.byref(inp), n, a, b, c, pok, stream))

        def gain(n):
            capi.check(lib.cpmpc_feedback_gain_batch(opt._h, B, C.byref(inp), n, pK, pok, stream))
        for n in (1, N):
            r["plan_sensitivity_all_rows_%d" % n] = timed(lambda: sens(n, pK, psp, pup))
            r["feedback_gain_rows_%d" % n] = timed(lambda: gain(n))
            r["plan_sensitivity_K_only_rows_%d" % n] = timed(lambda: sens(n, pK, None, None))
            r["plan_sensitivity_k_sp_k_up_rows_%d" % n] = timed(lambda: sens(n, None, psp, pup))
        sens(N, pK, psp, pup)
        x = sim.get_state()
        x_nom = x + 0.01
        sp_nom, sp = torch.zeros(B, dtype=dt, device=dev), torch.full((B,), 0.3, dtype=dt, device=dev)
        up_nom, up = torch.zeros(B, dtype=dt, device=dev), torch.full((B,), 5.0, dtype=dt, device=dev)
        u_nom, u_out = out.u.contiguous(), torch.empty_like(out.u)
        a = capi.PlanUpdate(struct_size=C.sizeof(capi.PlanUpdate), u_limit=300.0)
        for field, t in (("u_nom", u_nom), ("K", K), ("x_nom", x_nom), ("x", x), ("k_sp", k_sp), ("sp_nom", sp_nom), ("sp", sp),
                         ("k_up", k_up), ("u_prev_nom", up_nom), ("u_prev", up), ("u_out", u_out)):
            setattr(a, field, t.data_ptr())
        r["plan_update_rows_%d" % N] = timed(
            lambda: capi.check(lib.cpmpc_plan_update_batch(cdt, capi.MODEL_SINGLE, B, N, C.byref(a), stream)))
        res[name] = r
        opt.close()
        del K, k_sp, k_up, u_nom, u_out, sim, opt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
