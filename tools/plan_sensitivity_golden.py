"""Regenerates tests/golden/plan_sensitivity_sample.json: per configuration of the feedback-gain sample (same seeds, so the
same x0 and z) the worst relative difference between the condensed closed forms of k_sp = du/dset_point, k_up = du/du_prev
and the dense KKT solve -- the figure the GPU test's bound is 100 times (tests/test_gpu_plan_sensitivity.py) -- and rows 0..1
of both on 16 lanes.  CPU only.  Usage: python tools/plan_sensitivity_golden.py [--check]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import plan_sensitivity_ref as ps  # noqa: E402
from oracle import oracle as orc  # noqa: E402

if __name__ == "__main__":
    data = ps.make_golden(orc)
    for key, cfg in data["configs"].items():
        print("%-22s condensed vs dense, worst of %d: k_sp %.3e  k_up %.3e" % (key, cfg["sample_lanes"], cfg["k_sp_worst_rel"],
                                                                             cfg["k_up_worst_rel"]))
    if "--check" not in sys.argv:
        ps.dump_golden(data)
        print("wrote %s (%d bytes)" % (ps.GOLDEN_PATH, os.path.getsize(ps.GOLDEN_PATH)))
