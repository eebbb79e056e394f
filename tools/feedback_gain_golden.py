"""Regenerates tests/golden/feedback_gain_sample.json: the seeded sample of the feedback-gain tests (states, the CPU oracle's
solutions z of two lanes, rows K[0..1] of the dense reference on 16 lanes per configuration) and, per configuration, the worst relative
difference between the condensed closed form and the dense KKT solve on the sample -- the figure the GPU test's bound is
100 times (tests/test_gpu_feedback.py).  CPU only.  Usage: python tools/feedback_gain_golden.py [--check]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import feedback_ref as fr  # noqa: E402
from oracle import oracle as orc  # noqa: E402

if __name__ == "__main__":
    data = fr.make_golden(orc)
    for key, cfg in data["configs"].items():
        print("%-22s condensed vs dense, worst of %d: %.3e" % (key, cfg["sample_lanes"], cfg["condensed_vs_dense_worst_rel"]))
    if "--check" not in sys.argv:
        fr.dump_golden(data)
        print("wrote %s (%d bytes)" % (fr.GOLDEN_PATH, os.path.getsize(fr.GOLDEN_PATH)))
