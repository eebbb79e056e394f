"""Times the reverse-mode call of DESIGN.md section 5d beside the forward calls it replaces, on cuda:0 with device events, 20
calls after 5 warm-ups, 262 144 4-state problems, fp32 and fp64, in one session: cpmpc_plan_vjp_batch (three outputs) at
n_rows = 1 and N, cpmpc_feedback_gain_batch at n_rows = 1 and N, and the three-output cpmpc_plan_sensitivity_batch at
n_rows = N followed by the contraction of K, k_sp, k_up with the cotangent in torch -- the only way to the same NX + 2 numbers
per problem before the reverse-mode kernel.  z is the handle's solution after one cold-start step.  Prints one JSON line.
Usage: python tools/plan_vjp_timing.py [--batch B]"""
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
        opt.step(torch.tensor(xs, dtype=dt, device=dev), DYN, 0.0, want_predicted=False)
        N, nx = opt.N, opt.nx
        lib = capi.load()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        arr = capi.dbl_array(DYN, len(DYN))
        inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
        inp.dyn_shared_host = C.cast(arr, C.POINTER(C.c_double))
        gbar = torch.tensor(rng.uniform(-1, 1, (N, B)), dtype=dt, device=dev)
        K = torch.empty((N, nx, B), dtype=dt, device=dev)
        k_sp, k_up = torch.empty((N, B), dtype=dt, device=dev), torch.empty((N, B), dtype=dt, device=dev)
        g_x0 = torch.empty((nx, B), dtype=dt, device=dev)
        g_sp, g_up = torch.empty((B,), dtype=dt, device=dev), torch.empty((B,), dtype=dt, device=dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev)
        pg, pK, psp, pup, px0, pgs, pgu, pok = (C.c_void_p(t.data_ptr()) for t in (gbar, K, k_sp, k_up, g_x0, g_sp, g_up, ok))

        def vjp(n):
            capi.check(lib.cpmpc_plan_vjp_batch(opt._h, B, C.byref(inp), n, pg, px0, pgs, pgu, pok, stream))

        def gain(n):
            capi.check(lib.cpmpc_feedback_gain_batch(opt._h, B, C.byref(inp), n, pK, pok, stream))

        def forward_and_contract():
            capi.check(lib.cpmpc_plan_sensitivity_batch(opt._h, B, C.byref(inp), N, pK, psp, pup, pok, stream))
            return (K * gbar[:, None, :]).sum(0), (k_sp * gbar).sum(0), (k_up * gbar).sum(0)
        r = {"wide_qp": bool(opt.wide_qp)}
        for n in (1, N):
            r["plan_vjp_rows_%d" % n] = timed(lambda: vjp(n))
            r["feedback_gain_rows_%d" % n] = timed(lambda: gain(n))
        r["plan_sensitivity_all_rows_%d_plus_torch_contraction" % N] = timed(forward_and_contract)
        # the two routes agree (a sanity figure, not a test): worst difference relative to the largest gradient
        vjp(N)
        fx, fs, fu = forward_and_contract()
        scale = max(fx.abs().max().item(), fs.abs().max().item(), fu.abs().max().item())
        r["vjp_vs_forward_contraction_max_rel"] = max((g_x0 - fx).abs().max().item(), (g_sp - fs).abs().max().item(),
                                                      (g_up - fu).abs().max().item()) / scale
        res[name] = r
        opt.close()
        del K, k_sp, k_up, gbar, opt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
