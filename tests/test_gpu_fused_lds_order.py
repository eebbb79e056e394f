"""The fused SQP kernel's reordered LDS reads leave every result bit for bit what it was.

The float 4-state instantiations of fused_sqp_kernel / fused_sqp_dyn_kernel read the linearisation's u and the line search's
(u, du) one step ahead of the RK4 step that uses them (csrc/mpc_fused_body.inc: kUAhead).  No arithmetic moved, so u, the predicted states,
status, iterations and ls_evals must equal, exactly, what the commit before the change computed: tests/golden/
fused_lds_order.json holds a digest of each of them per case, recorded from that commit's build by
tools/fused_lds_order_golden.py.  No tolerance: a digest matches or it does not.  The double kernels and the REFINE / wide
handles share the source file and are held to the same fixture.  Cases, shapes and the two runs: tests/helpers/fused_lds_order.py."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from helpers import fused_lds_order as flo  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_lds_order.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    assert doc["iterations"] == flo.ITERS and tuple(doc["fields"]) == flo.FIELDS
    assert sorted(doc["cases"]) == sorted(flo.case_id(N, sp, f) for (N, sp) in flo.SHAPES for f in flo.FORMS)
    return doc["cases"]


@pytest.fixture(scope="module")
def inp():
    return flo.inputs()


@pytest.mark.parametrize("form", list(flo.FORMS))
@pytest.mark.parametrize("N,sp", flo.SHAPES)
def test_outputs_keep_their_bits(pkg, golden, inp, N, sp, form):
    want = golden[flo.case_id(N, sp, form)]
    for B in flo.BATCHES:
        res = flo.run_case(pkg, inp, N, sp, form, B)
        if B == max(flo.BATCHES):
            # the runs reach what they are there for: backtracking trials in the cold run (the line search's step loop more
            # than once per iteration), finite results
            assert int(res["cold"]["ls_evals"].max()) > flo.ITERS
            assert bool(torch.isfinite(res["cold"]["u"]).all()) and bool(torch.isfinite(res["warm"]["u"]).all())
        for run in flo.RUNS:
            for f in flo.FIELDS:
                got = flo.digest(res[run][f])
                print("%s B=%d %s %s: %s (recorded %s)" % (flo.case_id(N, sp, form), B, run, f, got, want[str(B)][run][f]))
                assert got == want[str(B)][run][f], (B, run, f)


def test_warm_runs_take_the_early_exit(pkg, inp):
    """The warm run is in the fixture for the `tiny` / skip-merit branches: at the headline shape problems of it stop before
    the iteration cap or take steps without a merit evaluation (fewer line-search evaluations than iterations)."""
    res = flo.run_case(pkg, inp, 40, 10, "f32-shared", max(flo.BATCHES))["warm"]
    it, ev = res["iterations"].cpu().numpy(), res["ls_evals"].cpu().numpy()
    print("warm iterations", sorted(set(it.tolist())), "ls_evals", sorted(set(ev.tolist())))
    assert (it < flo.ITERS).any() or (ev < it).any()
