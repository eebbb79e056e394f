"""Admission of the plan-derivative cases off the default shape (tests/helpers/plan_shapes.py), on the CPU: per (case, call) the
reference figure -- the larger of the numpy condensed form against the dense KKT solve and of the condensed form's change under
a relative perturbation of 1e-12 of Phi and Gamma, the worst of 70 lanes -- is what tests/golden/plan_derivative_shapes.json
holds, and it meets the cap: 1e-9 with soft terminal rows, 1e-7 with the default rows.  The cap is a condition, not a
tolerance: the GPU tests bound every lane by 100 x the figure, so it keeps that bound at or below 1e-7 / 1e-5.  A pair above
its cap is listed under "excluded" with its figure and carries no bound; at most one pair in five, and no shape, weight set
or call as a whole.  CPU only."""
import numpy as np
import pytest

from helpers import feedback_ref as fr
from helpers import plan_shapes as sh

CASES = sh.cases()
GRID_A = set(sh.grid_a())


@pytest.fixture(scope="module")
def golden():
    return sh.load_golden()


def test_the_grid_is_the_one_the_golden_file_holds(golden):
    assert list(golden["cases"]) == [sh.case_key(c) for c in CASES] and golden["lanes"] == sh.LANES == 70
    assert len(set(CASES)) == len(CASES) == 47 and len({sh.case_seed(c) for c in CASES}) == len(CASES)
    # grid A: every shape in both models but double 100/10; B and C as counted
    assert len(sh.grid_a()) == 2 * len(sh.SHAPES) - 1 and len(sh.grid_b()) == 16 and len(sh.grid_c()) == 14
    for c in CASES:
        entry = golden["cases"][sh.case_key(c)]
        assert entry["seed"] == sh.case_seed(c) and tuple(entry["calls"]) == sh.CALLS
        for call in sh.CALLS:
            assert ("emulation" in entry["calls"][call]) == (c in GRID_A)
        assert c.N % c.sp == 0 and {1, c.sp, c.N - 1, c.N} <= set(sh.n_rows_of(c)) | {0}
    assert sh.n_rows_of(sh.Case("single", 8, 8, "soft", "D")) == [1, 8, 7]
    assert sh.n_rows_of(sh.Case("single", 6, 1, "soft", "D")) == [1, 2, 5, 6]
    assert sh.n_rows_of(sh.Case("single", 12, 4, "soft", "D")) == [1, 4, 5, 11, 12]


def test_exclusions_are_few_and_leave_every_shape_weight_set_and_call(golden):
    excluded = sh.excluded_pairs(golden)
    pairs = [(sh.case_key(c), call) for c in CASES for call in sh.CALLS]
    assert excluded <= set(pairs) and len(excluded) == len(golden["excluded"])
    assert 5 * len(excluded) <= len(pairs), (len(excluded), len(pairs))
    by_key = {sh.case_key(c): c for c in CASES}
    for e in golden["excluded"]:   # listed with its figure, and only because of it
        c = by_key[e["case"]]
        assert e["figure"] == golden["cases"][e["case"]]["calls"][e["call"]]["figure"] > sh.CAP[c.rows]
    kept = [(by_key[k], call) for k, call in pairs if (k, call) not in excluded]
    assert {(c.N, c.sp) for c, _ in kept} == {(c.N, c.sp) for c in CASES}
    assert {c.weights for c, _ in kept} == set(sh.WEIGHTS)
    for call in sh.CALLS:   # no call loses a shape, a weight set or a model
        mine = [c for c, k in kept if k == call]
        assert {(c.N, c.sp) for c in mine} == {(c.N, c.sp) for c in CASES}, call
        assert {c.weights for c in mine} == set(sh.WEIGHTS) and {c.model for c in mine} == {"single", "double"}, call


@pytest.mark.parametrize("case", CASES, ids=[sh.case_key(c) for c in CASES])
def test_reference_figures_are_the_stored_ones_and_meet_the_cap(orc, golden, case):
    key = sh.case_key(case)
    stored = golden["cases"][key]["calls"]
    excluded = sh.excluded_pairs(golden)
    smp = sh.sample(orc, case)
    N, nx = case.N, 4 if case.model == "single" else 6
    assert smp.z.shape == (nx * (N // case.sp + 1) + N, sh.LANES) and np.isfinite(smp.z).all()
    wu, wd = sh.WEIGHTS[case.weights]
    assert (smp.p.window_length, smp.p.state_spacing, smp.p.u_cost_weight, smp.p.u_derivative_cost_weight) == (N, case.sp, wu, wd)
    Rw, Dg = fr.terminal_rows(orc, smp.p, case.model)
    assert Dg.all() if case.rows == "soft" else (Dg.sum() == 1 and Dg[0] == 1)
    figs = sh.reference_figures(orc, case)
    for call in sh.CALLS:
        f, s = figs[call], stored[call]
        print("%s %s: condensed vs dense %.3e, perturbation %.3e, figure %.3e (stored %.3e, cap %.0e%s)"
              % (key, call, f["condensed_vs_dense"], f["perturbation"], f["figure"], s["figure"], sh.CAP[case.rows],
                 ", excluded" if (key, call) in excluded else ""))
        assert s["figure"] == max(s["condensed_vs_dense"], s["perturbation"])
        assert 0.5 * s["figure"] <= f["figure"] <= 2.0 * s["figure"], (call, f, s)
        if (key, call) not in excluded:
            assert f["figure"] <= sh.CAP[case.rows] and s["figure"] <= sh.CAP[case.rows], (call, f["figure"])
    if case in GRID_A:
        emu = sh.float_emulation(orc, case)
        for call in sh.CALLS:
            for part in sh.PARTS[call]:
                got, want = emu[call][part], stored[call]["emulation"][part]
                print("%s %s %s: float emulation median %.3e p99 %.3e (stored %.3e / %.3e)"
                      % (key, call, part, got[0], got[1], want[0], want[1]))
                for g, w in zip(got, want):
                    assert 0.5 * w <= g <= 2.0 * w, (call, part, got, want)


@pytest.mark.parametrize("model", ["single", "double"])
def test_float_blocks_are_computed_in_float_not_rounded(orc, model):
    """fr.blocks_of(precision="f32") reads the single-precision oracle's A: float values, within float rounding of the double
    blocks through the RK4 steps of an interval, and not those blocks rounded; the default stays the double oracle's."""
    case = sh.Case(model, 12, 4, "soft", "D")
    smp = sh.sample(orc, case)
    z = smp.z[:, 0].astype(np.float32).astype(np.float64)
    Phi, Gam = fr.blocks_of(orc, smp.p, fr.DYN[model], z, model)
    Phi2, Gam2 = fr.blocks_of(orc, smp.p, fr.DYN[model], z, model, precision="f64")
    Pf, Gf = fr.blocks_of(orc, smp.p, fr.DYN[model], z, model, precision="f32")
    assert np.array_equal(Phi, Phi2) and np.array_equal(Gam, Gam2)
    assert Pf.shape == Phi.shape and Gf.shape == Gam.shape
    for f, d in ((Pf, Phi), (Gf, Gam)):
        assert np.array_equal(f, f.astype(np.float32).astype(np.float64))
        assert not np.array_equal(f, d.astype(np.float32).astype(np.float64))
        assert np.abs(f - d).max() <= 200 * np.finfo(np.float32).eps * np.abs(d).max()
    with pytest.raises(AssertionError):
        fr.blocks_of(orc, smp.p, fr.DYN[model], z, model, precision="f16")


def test_generalised_sample_keeps_the_default_samples(orc):
    """fr.solve_sample with its new arguments spelled out at their defaults is the sample the four golden files were made from,
    bit for bit (their own tests hold the stored lanes to it)."""
    for model, sp, mix in (("single", 10, "default"), ("double", 5, "mix")):
        p0, tw0, x0, z0 = fr.solve_sample(orc, model, sp, mix, 4)
        p1, tw1, x1, z1 = fr.solve_sample(orc, model, sp, mix, 4, window_length=40, u_cost_weight=0.1,
                                          u_derivative_cost_weight=0.1, seed=fr.config_seed(model, sp, mix),
                                          terminal_weights=None if tw0 is None else list(tw0))
        assert bytes(p0) == bytes(p1) and tw0 == tw1 and np.array_equal(x0, x1) and np.array_equal(z0, z1)
