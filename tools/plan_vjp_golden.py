"""Regenerates tests/golden/plan_vjp_sample.json: per configuration of the feedback-gain sample (same seeds, so the same x0
and z) and per seeded cotangent the worst relative difference between the condensed adjoint of csrc/plan_vjp_kernels.hpp and
the dense KKT solve -- the figure the GPU test's bound is 100 times (tests/test_gpu_plan_vjp.py) -- and the dense outputs of
16 lanes.  CPU only.  Usage: python tools/plan_vjp_golden.py [--check]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import plan_vjp_ref as pv  # noqa: E402
from oracle import oracle as orc  # noqa: E402

if __name__ == "__main__":
    data = pv.make_golden(orc)
    for key, cfg in data["configs"].items():
        print("%-22s condensed vs dense, worst of %d: uniform %.3e  e0 %.3e" % (key, cfg["sample_lanes"],
                                                                                cfg["worst_rel_uniform"], cfg["worst_rel_e0"]))
    if "--check" not in sys.argv:
        pv.dump_golden(data)
        print("wrote %s (%d bytes)" % (pv.GOLDEN_PATH, os.path.getsize(pv.GOLDEN_PATH)))
