"""Makes tests/golden/plan_derivative_shapes.json: the reference figures and the float emulation's percentiles of the
plan-derivative calls off the default shape (tests/helpers/plan_shapes.py says what they are).  CPU only, a few minutes.
Run from the repository root: python tests/golden/gen_plan_derivative_shapes.py
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from helpers import plan_shapes as sh  # noqa: E402
from oracle import oracle  # noqa: E402


def main():
    t0 = time.time()

    def progress(c, entry):
        print("%-34s %s  (%.0f s)" % (sh.case_key(c), "  ".join("%s %.2e" % (k, v["figure"]) for k, v in entry["calls"].items()),
                                      time.time() - t0), flush=True)
    data = sh.make_golden(oracle, progress)
    sh.dump_golden(data)
    pairs = len(data["cases"]) * len(sh.CALLS)
    print("%d cases, %d pairs, %d excluded -> %s" % (len(data["cases"]), pairs, len(data["excluded"]), sh.GOLDEN_PATH))
    for e in data["excluded"]:
        print("  excluded: %(case)s %(call)s %(figure).3e" % e)


if __name__ == "__main__":
    main()
