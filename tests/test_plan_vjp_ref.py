"""The reverse mode of the plan's sensitivities on the CPU: the dense adjoint (one solve of the symmetric KKT system) and the
condensed adjoint the kernel implements agree on the seeded sample of the feedback-gain tests -- both models, default terminal
rows and a mix of cost / equality rows, state_spacing 5, 10, 20 -- the committed figures (tests/golden/plan_vjp_sample.json)
are what the generator makes, and the adjoint identity holds against the forward forms.  CPU only.

Bounds: the condensed adjoint is held to the figure the generator recorded for the configuration, with the regeneration
margin of tests/test_plan_sensitivity_ref.py (10 x: the same order of magnitude on any IEEE machine).  The adjoint identity
compares two sums of NX + 2 products g_i d_i; each g_i is off by at most the recorded figure times max |g|, so the two sides
differ by at most that times sum |d_i| each -- the test allows 10 x the recorded figure times max |g| sum |d_i|."""
import numpy as np
import pytest

from helpers import feedback_ref as fr
from helpers import plan_sensitivity_ref as ps
from helpers import plan_vjp_ref as pv

CONFIGS = fr.configs()
IDS = [fr.config_key(*c) for c in CONFIGS]


@pytest.fixture(scope="module")
def golden():
    return pv.load_golden()


@pytest.fixture(scope="module")
def samples(orc):
    """The 64-lane sample of every configuration, solved once and shared (never modified)."""
    cache = {}

    def get(model, sp, mix):
        key = (model, sp, mix)
        if key not in cache:
            cache[key] = fr.solve_sample(orc, model, sp, mix, fr.SAMPLE_LANES)
        return cache[key]
    return get


@pytest.mark.parametrize("model,sp,mix", CONFIGS, ids=IDS)
def test_condensed_adjoint_matches_dense_and_golden(orc, golden, samples, model, sp, mix):
    p, tw, x0, z = samples(model, sp, mix)
    cfg = golden["configs"][fr.config_key(model, sp, mix)]
    gain_cfg = fr.load_golden()["configs"][fr.config_key(model, sp, mix)]
    assert cfg["seed"] == gain_cfg["seed"] == fr.config_seed(model, sp, mix) and cfg["sample_lanes"] == fr.SAMPLE_LANES
    assert cfg["gbar_seed"] == cfg["seed"] + 1
    nx, N = x0.shape[0], int(p.window_length)
    cots = pv.cotangents(model, sp, mix, fr.SAMPLE_LANES, N)
    assert np.abs(cots["uniform"]).max() <= 1.0 and np.array_equal(cots["e0"][:, 3], np.eye(N)[0])
    for b in range(pv.GOLDEN_GBAR_LANES):   # the stored cotangents pin the generator
        assert np.array_equal(cots["uniform"][:, b], np.array(cfg["gbar_uniform"][b]))
    for name in pv.COTANGENTS:
        worst = 0.0
        for b in range(fr.SAMPLE_LANES):   # every lane: none is skipped
            gd = pv.dense_vjp(orc, p, fr.DYN[model], z[:, b], cots[name][:, b], model=model)
            gc = pv.condensed_ref(orc, p, fr.DYN[model], z[:, b], cots[name][:, b], model=model)
            assert gd.shape == gc.shape == (nx + 2,) and np.isfinite(gd).all()
            worst = max(worst, pv.rel_err(gc, gd))
            if tw is not None and b < 4:   # the per-problem form of the terminal rows gives the same reference
                gt = pv.dense_vjp(orc, fr.params_for(orc, model, sp), fr.DYN[model], z[:, b], cots[name][:, b],
                                  terminal_weights=tw, model=model)
                assert np.array_equal(gt, gd)
            if b < fr.GOLDEN_LANES:   # the committed rows (12 digits; z is regenerated from the seed)
                assert pv.rel_err(np.array(cfg["dense_" + name][b]), gd) <= 1e-9, (name, b)
        print("%s %s: condensed vs dense adjoint, worst of %d lanes %.3e (recorded %.3e)"
              % (fr.config_key(model, sp, mix), name, fr.SAMPLE_LANES, worst, cfg["worst_rel_" + name]))
        assert worst <= 10.0 * cfg["worst_rel_" + name] + 1e-15, (name, worst)
    assert cfg["condensed_vs_dense_worst_rel"] == max(cfg["worst_rel_" + n] for n in pv.COTANGENTS)


@pytest.mark.parametrize("model,sp,mix", CONFIGS, ids=IDS)
def test_adjoint_identity_against_the_forward_forms(orc, golden, samples, model, sp, mix):
    """<gbar, K dx + k_sp dsp + k_up dup> = <(g_x0, g_sp, g_up), (dx, dsp, dup)> on every lane, for both cotangents, the
    forward forms plan_sensitivity_ref's and the perturbation seeded."""
    p, tw, x0, z = samples(model, sp, mix)
    cfg = golden["configs"][fr.config_key(model, sp, mix)]
    nx, N = x0.shape[0], int(p.window_length)
    cots = pv.cotangents(model, sp, mix, fr.SAMPLE_LANES, N)
    delta = np.random.default_rng(fr.config_seed(model, sp, mix) + 2).uniform(-1.0, 1.0, (fr.SAMPLE_LANES, nx + 2))
    worst = 0.0
    for b in range(fr.SAMPLE_LANES):
        K, k_sp, k_up = ps.condensed_ref(orc, p, fr.DYN[model], z[:, b], model=model)
        du = K @ delta[b, :nx] + k_sp * delta[b, nx] + k_up * delta[b, nx + 1]
        for name in pv.COTANGENTS:
            gbar = cots[name][:, b]
            g = pv.condensed_ref(orc, p, fr.DYN[model], z[:, b], gbar, model=model)
            lhs, rhs = float(gbar @ du), float(g @ delta[b])
            tol = 10.0 * cfg["condensed_vs_dense_worst_rel"] * np.abs(g).max() * np.abs(delta[b]).sum()
            worst = max(worst, abs(lhs - rhs) / tol)
            assert abs(lhs - rhs) <= tol, (name, b, lhs, rhs, tol)
    print("%s: adjoint identity, worst |lhs - rhs| / tolerance %.3e" % (fr.config_key(model, sp, mix), worst))


@pytest.mark.parametrize("model,sp", [("single", 10), ("double", 20)])
def test_leading_rows_equal_the_zero_padded_cotangent(orc, samples, model, sp):
    p, _, _, z = samples(model, sp, "default")
    N = int(p.window_length)
    gbar = pv.cotangents(model, sp, "default", 4, N)["uniform"]
    for b in range(4):
        for n in (1, 3, N):
            padded = np.zeros(N)
            padded[:n] = gbar[:n, b]
            for fn in (pv.dense_vjp, pv.condensed_ref):
                assert np.array_equal(fn(orc, p, fr.DYN[model], z[:, b], gbar[:n, b], model=model),
                                      fn(orc, p, fr.DYN[model], z[:, b], padded, model=model)), (fn.__name__, b, n)


def test_float_emulation_is_the_double_form_at_float_precision(orc, samples):
    """The float32 precision split stays within the bound of plan_sensitivity_ref's emulation test of the double form: the
    yardstick of the fp32 GPU test is a sane one."""
    model, sp = "single", 10
    p, _, _, z = samples(model, sp, "default")
    gbar = pv.cotangents(model, sp, "default", 8, int(p.window_length))["uniform"]
    for b in range(8):
        gd = pv.dense_vjp(orc, p, fr.DYN[model], z[:, b], gbar[:, b], model=model)
        gf = pv.condensed_ref(orc, p, fr.DYN[model], z[:, b], gbar[:, b], model=model, lin=np.float32)
        assert 1e-9 < pv.rel_err(gf, gd) < 3e6 * np.finfo(np.float32).eps
