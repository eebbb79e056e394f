"""Sensitivities of the plan to the set-point and to u_prev on the CPU: the dense KKT reference, the condensed closed forms
the kernel implements and differences of the oracle's QP solver agree on the seeded sample of the feedback-gain tests --
both models, default terminal rows and a mix of cost / equality rows, state_spacing 5, 10, 20 -- and the committed figures
(tests/golden/plan_sensitivity_sample.json) are what the generator makes.  CPU only.

Bounds, as tests/test_feedback_gain_ref.py: a solve of the KKT system loses at most cond(KKT) * eps relative to its largest
entry, so two exact methods may differ by that much and no more; the difference of two QP solves additionally cancels
max |dz| against max |k|."""
import numpy as np
import pytest

from helpers import feedback_ref as fr
from helpers import plan_sensitivity_ref as ps

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return ps.load_golden()


@pytest.mark.parametrize("model,sp,mix", fr.configs(), ids=[fr.config_key(*c) for c in fr.configs()])
def test_condensed_dense_and_qp_differences_agree(orc, golden, model, sp, mix):
    p, tw, x0, z = fr.solve_sample(orc, model, sp, mix, fr.SAMPLE_LANES)
    cfg = golden["configs"][fr.config_key(model, sp, mix)]
    gain_cfg = fr.load_golden()["configs"][fr.config_key(model, sp, mix)]
    assert cfg["seed"] == gain_cfg["seed"] == fr.config_seed(model, sp, mix) and cfg["sample_lanes"] == fr.SAMPLE_LANES
    worst = {"k_sp": 0.0, "k_up": 0.0}
    for b in range(fr.SAMPLE_LANES):   # every lane: none is skipped
        sd, ud, cond = ps.sensitivity_ref(orc, p, fr.DYN[model], z[:, b], model=model, want_cond=True)
        Kc, sc, uc = ps.condensed_ref(orc, p, fr.DYN[model], z[:, b], model=model)
        sq, uq, codes, dz_max = ps.sensitivity_qp_diff(orc, p, fr.DYN[model], z[:, b], model=model)
        assert all(c == 0 for c in codes), (b, codes)
        assert sd.shape == ud.shape == (40,) and np.isfinite(sd).all() and np.isfinite(ud).all()
        bound = cond * EPS
        for name, kd, kc, kq in (("k_sp", sd, sc, sq), ("k_up", ud, uc, uq)):
            e_c, e_q = ps.rel_err(kc, kd), ps.rel_err(kq, kd)
            assert e_c <= bound, (name, b, e_c, bound)
            assert e_q <= bound * (1.0 + dz_max / np.abs(kd).max()), (name, b, e_q, bound)
            worst[name] = max(worst[name], e_c)
        # the gain columns of the same recurrences are feedback_ref's, bitwise: one closed form, restated
        assert np.array_equal(Kc, fr.condensed_gain_ref(orc, p, fr.DYN[model], z[:, b], model=model))
        if tw is not None:   # the per-problem form of the terminal rows gives the same reference
            st, ut = ps.sensitivity_ref(orc, fr.params_for(orc, model, sp), fr.DYN[model], z[:, b], terminal_weights=tw,
                                        model=model)
            assert np.array_equal(st, sd) and np.array_equal(ut, ud)
        if b < fr.GOLDEN_LANES:   # the committed rows (9 digits; z is regenerated from the seed)
            row = np.array(cfg["k01"][b])
            assert ps.rel_err(row[:2], sd[:2]) <= 1e-6 and ps.rel_err(row[2:], ud[:2]) <= 1e-6
    print("%s: condensed vs dense, worst of %d lanes: k_sp %.3e (recorded %.3e), k_up %.3e (recorded %.3e)"
          % (fr.config_key(model, sp, mix), fr.SAMPLE_LANES, worst["k_sp"], cfg["k_sp_worst_rel"], worst["k_up"],
             cfg["k_up_worst_rel"]))
    # the recorded figures are this computation's: the same order of magnitude on any IEEE machine
    assert worst["k_sp"] <= 10.0 * cfg["k_sp_worst_rel"] + 1e-15
    assert worst["k_up"] <= 10.0 * cfg["k_up_worst_rel"] + 1e-15
    assert cfg["condensed_vs_dense_worst_rel"] == max(cfg["k_sp_worst_rel"], cfg["k_up_worst_rel"])


def test_sensitivities_predict_the_qp_step_and_have_the_expected_size(orc):
    """The QP is linear in both inputs: the step at (set-point + 0.3 m, u_prev + 5 N) is the step at (0, 0) plus
    0.3 k_sp + 5 k_up.  At the defaults max |k_sp| is tens to hundreds of N/m, max |k_up| a fraction of one, and k_up[0] > 0
    (a larger applied control pulls u_0 up through the derivative row)."""
    model, sp = "single", 10
    p, _, x0, z = fr.solve_sample(orc, model, sp, "default", 4)
    for b in range(4):
        k_sp, k_up = ps.sensitivity_ref(orc, p, fr.DYN[model], z[:, b], model=model)
        assert 10 < np.abs(k_sp).max() < 1000 and 0.05 < np.abs(k_up).max() < 1.0 and k_up[0] > 0
        r, c, J, A = fr.problem_eval(orc, model, p, fr.DYN[model], z[:4, b], 0.0, 0.0, z[:, b])
        r2, c2, _, _ = fr.problem_eval(orc, model, p, fr.DYN[model], z[:4, b], 0.3, 5.0, z[:, b])
        _, dz = orc.qp_solve(J, r, A, c, 40, 0.0)
        _, dz2 = orc.qp_solve(J, r2, A, c2, 40, 0.0)
        np.testing.assert_allclose((dz2 - dz)[20:], 0.3 * k_sp + 5.0 * k_up, rtol=0, atol=1e-7 * np.abs(k_sp).max())


def test_float_emulation_is_the_double_form_at_float_precision(orc):
    """The float32 precision split stays within cond(S + Dg) * eps_float of the double form (the bound of the gains' test):
    the yardstick of the fp32 GPU test is a sane one."""
    model, sp = "single", 10
    p, _, _, z = fr.solve_sample(orc, model, sp, "default", 8)
    for b in range(8):
        sd, ud = ps.sensitivity_ref(orc, p, fr.DYN[model], z[:, b], model=model)
        _, sf, uf = ps.condensed_ref(orc, p, fr.DYN[model], z[:, b], model=model, lin=np.float32)
        assert 1e-9 < ps.rel_err(sf, sd) < 3e6 * np.finfo(np.float32).eps
        assert 1e-9 < ps.rel_err(uf, ud) < 3e6 * np.finfo(np.float32).eps
