"""Times the plant step with derivatives of DESIGN.md section 5e beside the plant step itself, on cuda:0 with device events, 20
calls after 5 warm-ups, 262 144 4-state problems, fp32 and fp64, in one session, dt = 0.01 (ten sub-steps):
cpmpc_sim_step_batch, cpmpc_sim_step_jac_batch with x_new, A and Bu, and the same call with gx and gu alone (the VJP).  For the
expectation of section 5e -- the VJP costs about one linearize pass over n_sub sub-steps -- cpmpc_linearize_batch of the default
horizon (40 RK4 steps with sensitivities per problem, with its pack and unpack kernels) is timed too, and both are reported per
problem and RK4 step.  Prints one JSON line.
Usage: python tools/sim_jac_timing.py [--batch B] [--dt DT]"""
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
    ap.add_argument("--dt", type=float, default=0.01)
    args = ap.parse_args()
    pkg = importlib.import_module("cart-pole-mpc_amd")
    capi = pkg.capi
    lib = capi.load()
    B, dev, step_dt = args.batch, "cuda:0", args.dt
    n_sub, rem = 0, step_dt
    while rem > 0.0:
        n_sub, rem = n_sub + 1, rem - 0.001
    rng = np.random.default_rng(7)
    xs = np.stack([rng.uniform(-0.3, 0.3, B), np.pi / 2 + rng.uniform(-0.4, 0.4, B), rng.uniform(-0.5, 0.5, B),
                   rng.uniform(-1, 1, B)])
    us = rng.uniform(-20, 20, B)
    res = {"batch": B, "calls": 20, "warmup": 5, "dt": step_dt, "n_sub": n_sub}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        arr = capi.dbl_array(DYN, len(DYN))
        x = torch.tensor(xs, dtype=dt, device=dev)
        u = torch.tensor(us, dtype=dt, device=dev)
        state = x.clone()
        gbar = torch.tensor(rng.uniform(-1, 1, (4, B)), dtype=dt, device=dev)
        x_new, A, Bu = (torch.empty(s, dtype=dt, device=dev) for s in ((4, B), (16, B), (4, B)))
        gx, gu = torch.empty((4, B), dtype=dt, device=dev), torch.empty((B,), dtype=dt, device=dev)
        jac = capi.SimJac(struct_size=C.sizeof(capi.SimJac), state=x.data_ptr(), u=u.data_ptr(), x_new=x_new.data_ptr(),
                          A=A.data_ptr(), Bu=Bu.data_ptr())
        vjp = capi.SimJac(struct_size=C.sizeof(capi.SimJac), state=x.data_ptr(), u=u.data_ptr(), gbar=gbar.data_ptr(),
                          gx=gx.data_ptr(), gu=gu.data_ptr())
        cd = capi.F32 if dt == torch.float32 else capi.F64

        def sim():
            capi.check(lib.cpmpc_sim_step_batch(cd, B, arr, step_dt, C.c_void_p(u.data_ptr()), None, None,
                                                C.c_void_p(state.data_ptr()), stream))

        def call(a):
            capi.check(lib.cpmpc_sim_step_jac_batch(capi.MODEL_SINGLE, cd, B, arr, step_dt, C.byref(a), stream))
        r = {"sim_step_batch": timed(sim), "sim_step_jac_all_outputs": timed(lambda: call(jac)),
             "sim_step_vjp": timed(lambda: call(vjp))}
        # the two routes agree (a sanity figure, not a test): worst difference relative to the largest gradient
        call(jac)
        call(vjp)
        fx = (A.reshape(4, 4, B) * gbar[:, None, :]).sum(0)
        fu = (Bu * gbar).sum(0)
        r["vjp_vs_jacobian_contraction_max_rel"] = max((gx - fx).abs().max().item(), (gu - fu).abs().max().item()) / max(
            fx.abs().max().item(), fu.abs().max().item())
        # one linearisation of the default horizon: N RK4 steps with sensitivities per problem
        opt = pkg.BatchOptimization(pkg.default_params(), max_batch=B, dtype=dt, device=0)
        opt.step(x, DYN, 0.0, want_predicted=False)
        z = opt.get_solution(B)
        r["linearize_batch_N_%d" % opt.N] = timed(lambda: opt.linearize(z, DYN))
        r["vjp_us_per_million_rk4_steps"] = 1e3 * r["sim_step_vjp"]["min_ms"] / (B * n_sub / 1e6)
        r["linearize_us_per_million_rk4_steps"] = 1e3 * r["linearize_batch_N_%d" % opt.N]["min_ms"] / (B * opt.N / 1e6)
        res[name] = r
        opt.close()
        del opt, z, A, x_new
    print(json.dumps(res))


if __name__ == "__main__":
    main()
