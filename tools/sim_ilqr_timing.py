"""Times the two iLQR passes of DESIGN.md section 5o on cuda:0 with device events, least of 20 calls after 5 warm-ups,
B = 262 144, T = 10 ticks, shared parameters, fp32 and fp64, both models, at dt = 0.01 (ten sub-steps a tick) and dt = 0.001 (one):
  (a) sim_ilqr_backward (K, kff, dV) against sim_lqr (K, P0) on the same trajectory: the same tick pass and Riccati step, plus the
      half-gradient vector, the scalar box QP and the reference's loads;
  (b) sim_ilqr_forward (xs, us, cost, a step per lane) against sim_rollout_feedback (xs, us) under the same gains: the same loop,
      plus the feedforward term and the cost.
Each pair is timed in the order new, old, new: the difference between the two runs of the new call is the spread a comparison has
to beat.  Every (dtype, model) pair runs in a child process of its own under its own time limit, and the first one that fails ends
the run.  Prints one JSON line.
Usage: python tools/sim_ilqr_timing.py [--ticks T] [--batch B] [--limit SECONDS]"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_sensitivity_timing import DYN, timed  # noqa: E402
from sim_lqr_timing import DYN_DOUBLE, Q, R  # noqa: E402


def one(name, model, B, T):
    pkg = importlib.import_module("cart-pole-mpc_amd")
    dt = torch.float32 if name == "f32" else torch.float64
    dev = "cuda:0"
    nx = 4 if model == "single" else 6
    nq = nx // 2
    dyn = DYN if model == "single" else DYN_DOUBLE
    rng = np.random.default_rng(7)
    x0 = torch.tensor(np.concatenate([rng.uniform(-0.3, 0.3, (1, B)), np.pi / 2 + rng.uniform(-0.4, 0.4, (nq - 1, B)),
                                      rng.uniform(-0.5, 0.5, (nq, B))]), dtype=dt, device=dev)
    u = torch.tensor(rng.uniform(-20, 20, (T, B)), dtype=dt, device=dev)
    target = [0.0] + [float(np.pi / 2)] * (nq - 1) + [0.0] * nq
    x_ref = torch.tensor(target, dtype=dt, device=dev).reshape(1, nx, 1).expand(T + 1, nx, B).contiguous()
    alpha = torch.full((B,), 0.5, dtype=dt, device=dev)
    r, out = {}, {}
    for step_dt in (0.01, 0.001):
        xs = pkg.sim_rollout_states(dyn, step_dt, x0, u, model=model)["xs"]
        bw = pkg.sim_ilqr_backward(dyn, step_dt, x0, u, xs, x_ref, None, Q[model], R, model=model, want=("K", "kff"))

        def backward():
            out["bw"] = pkg.sim_ilqr_backward(dyn, step_dt, x0, u, xs, x_ref, None, Q[model], R, model=model, want=("K", "kff", "dV"))

        def lqr():
            out["lqr"] = pkg.sim_lqr(dyn, step_dt, x0, u, xs, Q[model], R, model=model)

        def forward():
            out["fw"] = pkg.sim_ilqr_forward(dyn, step_dt, x0, u, bw["kff"], bw["K"], x0, xs, x_ref, None, Q[model], R, alpha=alpha,
                                             u_limit=300.0, model=model, want=("xs", "us", "cost"))

        def feedback():
            out["fb"] = pkg.sim_rollout_feedback(dyn, step_dt, x0, u, bw["K"], x0, xs, u_limit=300.0, model=model, want=("xs", "us"))

        tag = "dt%g" % step_dt
        for key, new, old, old_name in (("backward_", backward, lqr, "sim_lqr"), ("forward_", forward, feedback, "sim_rollout_feedback")):
            a, o, b = timed(new), timed(old), timed(new)
            first, second = a["min_ms"], b["min_ms"]
            r[key + tag] = {"new_first": a, old_name: o, "new_second": b, "new_over_old": min(first, second) / o["min_ms"],
                            "new_spread": abs(first - second) / min(first, second)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a (dtype, model) pair may take")
    ap.add_argument("--one", nargs=2, metavar=("DTYPE", "MODEL"), help="(internal) time one pair in this process")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(one(args.one[0], args.one[1], args.batch, args.ticks)))
        return 0
    res = {"ticks": args.ticks, "batch": args.batch, "calls": 20, "warmup": 5}
    for name in ("f32", "f64"):
        for model in ("single", "double"):
            cmd = [sys.executable, os.path.abspath(__file__), "--ticks", str(args.ticks), "--batch", str(args.batch), "--one",
                   name, model]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
            if p.returncode != 0:   # nothing more is started on the device after a failure
                print(json.dumps(res))
                return p.returncode
            res["%s_%s" % (name, model)] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
