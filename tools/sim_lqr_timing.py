"""Times the two tracking calls of DESIGN.md section 5n on cuda:0 with device events, 20 calls after 5 warm-ups, B = 262 144,
T = 10 ticks, shared parameters, fp32 and fp64, both models:
  (a) sim_rollout_feedback over the T ticks, at dt = 0.001 (one sub-step a tick) and dt = 0.01 (ten), against what the calls
      before it offer for the same work: T pairs of feedback_apply (the tick's gain row on the plant's current state) and
      BatchSimulator.step -- 2 T launches, the state through HBM between them;
  (b) sim_lqr at dt = 0.01 against sim_rollout_vjp asked for g_x0 and g_u on the same inputs: the same tick pass (Phi and gamma
      of every tick, reverse over the ticks) with O(NX) algebra where sim_lqr has O(NX^2).
A "call" is the whole chain, between one pair of events.  The chain of (a) is timed twice, before and after the launch it is
compared with: the difference between its two runs is the spread a comparison has to beat.  Every (dtype, model) pair runs in a
child process of its own under its own time limit, and the first one that fails ends the run.  Prints one JSON line.
Usage: python tools/sim_lqr_timing.py [--ticks T] [--batch B] [--limit SECONDS]"""
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

DYN_DOUBLE = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]
Q = {"single": [1.0, 10.0, 0.1, 0.1], "double": [1.0, 10.0, 10.0, 0.1, 0.1, 0.1]}
R = 0.01


def one(name, model, B, T):
    pkg = importlib.import_module("cart-pole-mpc_amd")
    dt = torch.float32 if name == "f32" else torch.float64
    dev = "cuda:0"
    nx = 4 if model == "single" else 6
    nq = nx // 2
    dyn = DYN if model == "single" else DYN_DOUBLE
    rng = np.random.default_rng(7)
    x_nom = torch.tensor(np.concatenate([rng.uniform(-0.3, 0.3, (1, B)), np.pi / 2 + rng.uniform(-0.4, 0.4, (nq - 1, B)),
                                         rng.uniform(-0.5, 0.5, (nq, B))]), dtype=dt, device=dev)
    u = torch.tensor(rng.uniform(-20, 20, (T, B)), dtype=dt, device=dev)
    x0 = (x_nom + 0.01).contiguous()
    rows = [u[t] for t in range(T)]
    r, out = {}, {}
    for step_dt in (0.001, 0.01):
        xs_nom = pkg.sim_rollout_states(dyn, step_dt, x_nom, u, model=model)["xs"]
        K = pkg.sim_lqr(dyn, step_dt, x_nom, u, xs_nom, Q[model], R, model=model, want="K")["K"]
        noms = [x_nom] + [xs_nom[t] for t in range(T - 1)]
        gains = [K[t] for t in range(T)]
        sim = pkg.BatchSimulator(B, dtype=dt, device=0, model=model)

        def chain():
            sim.set_state(x0)
            for t in range(T):
                ut = pkg.feedback_apply(rows[t], gains[t], noms[t], sim.get_state(), u_limit=300.0, model=model)
                sim.step(dyn, step_dt, ut)
            out["chain"] = sim.get_state()

        def single():
            out["single"] = pkg.sim_rollout_feedback(dyn, step_dt, x0, u, K, x_nom, xs_nom, u_limit=300.0, model=model,
                                                     want="x_final")["x_final"]

        tag = "dt%g" % step_dt
        a, s, b = timed(chain), timed(single), timed(chain)
        first, second = a["min_ms"], b["min_ms"]
        r["fb_" + tag] = {"chain_first": a, "sim_rollout_feedback": s, "chain_second": b,
                          "chain_over_single": min(first, second) / s["min_ms"],
                          "chain_spread": abs(first - second) / min(first, second),
                          # a sanity figure, not a test: the chain wraps the difference as an angle, the launch to the nearest turn
                          "vs_chain_max_abs": (out["single"] - out["chain"]).abs().max().item()}
        if step_dt == 0.01:
            gbar = torch.ones((nx, B), dtype=dt, device=dev)

            def lqr():
                out["lqr"] = pkg.sim_lqr(dyn, step_dt, x_nom, u, xs_nom, Q[model], R, model=model)

            def vjp():
                out["vjp"] = pkg.sim_rollout_vjp(dyn, step_dt, x_nom, u, xs_nom, gbar_final=gbar, model=model, want=("x", "u"))

            tl, tv = timed(lqr), timed(vjp)
            r["lqr_" + tag] = {"sim_lqr": tl, "sim_rollout_vjp": tv, "lqr_over_vjp": tl["min_ms"] / tv["min_ms"],
                               "lqr_ms_per_tick": tl["min_ms"] / T}
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
