#!/usr/bin/env python3
"""Record tests/golden/fused_lds_order.json: a digest of every output of every case of tests/helpers/fused_lds_order.py.

Run ONCE on a GPU from a build of the commit BEFORE a change that must keep the fused SQP kernel's results bit for bit (the
fixture in the tree was recorded from the parent of the commit that reordered the kernel's LDS reads); CPMPC_LIB selects that
build's libcpmpc.so when the tree already holds the changed source.  tests/test_gpu_fused_lds_order.py then holds the
changed kernel to it.
usage: fused_lds_order_golden.py [--out PATH] [--check]     (--check: compare with the file instead of writing it)"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fused_lds_order.json"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    pkg = importlib.import_module("cart-pole-mpc_amd")
    from helpers import fused_lds_order as flo

    inp = flo.inputs()
    cases = {}
    early = 0
    for (N, sp) in flo.SHAPES:
        for form in flo.FORMS:
            per_b = {}
            for B in flo.BATCHES:
                res = flo.run_case(pkg, inp, N, sp, form, B)
                per_b[str(B)] = {run: {f: flo.digest(res[run][f]) for f in flo.FIELDS} for run in flo.RUNS}
                if B == max(flo.BATCHES):
                    it = res["warm"]["iterations"].cpu().numpy()
                    early += int((it < flo.ITERS).any())
                    print("%-22s cold ls_evals %s  warm iterations %s" % (flo.case_id(N, sp, form),
                          sorted(set(res["cold"]["ls_evals"].cpu().numpy().tolist())), sorted(set(it.tolist()))), flush=True)
            cases[flo.case_id(N, sp, form)] = per_b
    doc = dict(lib=os.path.basename(os.path.dirname(pkg.capi.LIB_PATH)), iterations=flo.ITERS, fields=list(flo.FIELDS),
               cases=cases)
    print("cases with an early exit in the warm run: %d of %d" % (early, len(cases)))
    if args.check:
        want = json.load(open(args.out))["cases"]
        bad = [(c, b, r, f) for c in want for b in want[c] for r in want[c][b] for f in want[c][b][r]
               if cases[c][b][r][f] != want[c][b][r][f]]
        print("differences: %d" % len(bad))
        for x in bad[:20]:
            print("  ", x)
        return 1 if bad else 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
