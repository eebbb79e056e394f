"""Times the plant step's parameter Jacobian of DESIGN.md section 5f beside the calls it is built next to, on cuda:0 with
device events, 20 calls after 5 warm-ups, 262 144 problems, fp32 and fp64, both models, in one session, dt = 0.01 (ten
sub-steps): cpmpc_sim_step_param_jac_batch with P alone, with gp alone (the parameter VJP), with gp, gx and gu (every
gradient of a backward pass), each with the shared parameter set and with per-problem parameters; the per-problem plain step
cpmpc_sim_step_dyn_batch; and, for comparison in the same session, the shared plain step cpmpc_sim_step_batch_model and
cpmpc_sim_step_jac_batch (Bu alone, gx and gu alone).  The expectation of section 5f to confirm or refute: the parameter
columns cost about what the same number of control columns would -- reported as the time of the P call above the plain step,
per parameter column, against the same figure of cpmpc_sim_step_jac_batch per column of the five it carries (Phi's and the
control column).  Prints one JSON line.
Usage: python tools/sim_param_jac_timing.py [--batch B] [--dt DT]"""
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

DYN_DOUBLE = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]


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
    res = {"batch": B, "calls": 20, "warmup": 5, "dt": step_dt, "n_sub": n_sub}
    for model, m, nx, dyn in (("single", capi.MODEL_SINGLE, 4, DYN), ("double", capi.MODEL_DOUBLE, 6, DYN_DOUBLE)):
        nq, npar = nx // 2, len(dyn)
        xs = np.concatenate([rng.uniform(-0.3, 0.3, (1, B)), np.pi / 2 + rng.uniform(-0.4, 0.4, (nq - 1, B)),
                             rng.uniform(-0.5, 0.5, (1, B)), rng.uniform(-1, 1, (nq - 1, B))])
        us = rng.uniform(-20, 20, B)
        cols = np.array(dyn)[:, None] * rng.uniform(0.9, 1.1, (npar, B))
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            arr = capi.dbl_array(dyn, npar)
            x = torch.tensor(xs, dtype=dt, device=dev)
            u = torch.tensor(us, dtype=dt, device=dev)
            dynt = torch.tensor(cols, dtype=dt, device=dev)
            state = x.clone()
            gbar = torch.tensor(rng.uniform(-1, 1, (nx, B)), dtype=dt, device=dev)
            P = torch.empty((nx * npar, B), dtype=dt, device=dev)
            gp = torch.empty((npar, B), dtype=dt, device=dev)
            gx, Bu = (torch.empty((nx, B), dtype=dt, device=dev) for _ in range(2))
            gu = torch.empty((B,), dtype=dt, device=dev)
            cd = capi.F32 if dt == torch.float32 else capi.F64

            def par(per_problem, **outs):
                a = capi.SimParamJac(struct_size=C.sizeof(capi.SimParamJac), state=x.data_ptr(), u=u.data_ptr())
                if per_problem:
                    a.dyn = dynt.data_ptr()
                for k, t in outs.items():
                    setattr(a, k, t.data_ptr())
                return lambda: capi.check(lib.cpmpc_sim_step_param_jac_batch(m, cd, B, arr, step_dt, C.byref(a), stream))

            def jac(**outs):
                a = capi.SimJac(struct_size=C.sizeof(capi.SimJac), state=x.data_ptr(), u=u.data_ptr())
                for k, t in outs.items():
                    setattr(a, k, t.data_ptr())
                return lambda: capi.check(lib.cpmpc_sim_step_jac_batch(m, cd, B, arr, step_dt, C.byref(a), stream))

            def plain(per_problem):
                d = C.c_void_p(dynt.data_ptr()) if per_problem else None
                return lambda: capi.check(lib.cpmpc_sim_step_dyn_batch(m, cd, B, arr, d, step_dt, C.c_void_p(u.data_ptr()), None,
                                                                       None, C.c_void_p(state.data_ptr()), stream))

            r = {"sim_step_shared": timed(plain(False)), "sim_step_per_problem": timed(plain(True)),
                 "sim_step_jac_Bu": timed(jac(Bu=Bu)), "sim_step_jac_gx_gu": timed(jac(gbar=gbar, gx=gx, gu=gu))}
            for tag, pp in (("shared", False), ("per_problem", True)):
                r["param_P_" + tag] = timed(par(pp, P=P))
                r["param_gp_" + tag] = timed(par(pp, gbar=gbar, gp=gp))
                r["param_gp_gx_gu_" + tag] = timed(par(pp, gbar=gbar, gp=gp, gx=gx, gu=gu))
            # a sanity figure, not a test: gp against the contraction of the stored P
            par(False, P=P)()
            par(False, gbar=gbar, gp=gp)()
            f = (P.reshape(nx, npar, B) * gbar[:, None, :]).sum(0)
            r["gp_vs_P_contraction_max_rel"] = (gp - f).abs().max().item() / f.abs().max().item()
            # the expectation: cost above the primal step, per tangent column, parameters against the control
            base = r["sim_step_shared"]["min_ms"]
            r["ms_per_parameter_column"] = (r["param_P_shared"]["min_ms"] - base) / npar
            # sim_jac_kernel always carries Phi beside the control column gamma: 4 + 1 tangent columns for both models (the
            # 6-state Phi has two columns in closed form, models.hpp: trivial_cols)
            r["ms_per_state_or_control_column"] = (r["sim_step_jac_Bu"]["min_ms"] - base) / 5
            res[model + "_" + name] = r
            del P, gp, gx, gu, Bu, x, u, dynt, state
    print(json.dumps(res))


if __name__ == "__main__":
    main()
