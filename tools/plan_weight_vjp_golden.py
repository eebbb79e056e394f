"""Regenerates tests/golden/plan_weight_vjp_sample.json: per configuration of the feedback-gain sample (same seeds, so the same
z; x0 shifted, set-point and u_prev non-zero so that the QP's step and residuals are generic) and per seeded cotangent the
worst difference between the condensed form of csrc/plan_weight_vjp_kernels.hpp and the dense KKT solves -- the figure the
GPU test's bound is 100 times (tests/test_gpu_plan_weight_vjp.py) -- and the dense outputs of 16 lanes.  CPU only.
Usage: python tools/plan_weight_vjp_golden.py [--check]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import plan_weight_vjp_ref as pw  # noqa: E402
from oracle import oracle as orc  # noqa: E402

if __name__ == "__main__":
    data = pw.make_golden(orc)
    for key, cfg in data["configs"].items():
        print("%-22s condensed vs dense, worst of %d: uniform %.3e (du %.3e)  e0 %.3e (du %.3e)"
              % (key, cfg["sample_lanes"], cfg["worst_rel_uniform"], cfg["worst_rel_du_uniform"], cfg["worst_rel_e0"],
                 cfg["worst_rel_du_e0"]))
    if "--check" not in sys.argv:
        pw.dump_golden(data)
        print("wrote %s (%d bytes)" % (pw.GOLDEN_PATH, os.path.getsize(pw.GOLDEN_PATH)))
