"""Feedback gains K = du / dx0 of the plan on the CPU: the dense KKT reference, the condensed closed form the kernel
implements and differences of the oracle's QP solver agree on the seeded sample -- both models, default terminal rows and a
mix of cost / equality rows, state_spacing 5, 10, 20 -- and the committed sample (tests/golden/feedback_gain_sample.json)
is what the generator makes.  CPU only.

Bounds: a solve of the KKT system loses at most cond(KKT) * eps relative to its largest entry (measured on the sample:
cond 5e6 .. 6e11, differences 1e-13 .. 1e-8, i.e. far inside), so two exact methods may differ by that much and no more;
the difference of two QP solves additionally cancels max |dz| against max |K|."""
import numpy as np
import pytest

from helpers import feedback_ref as fr

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return fr.load_golden()


@pytest.mark.parametrize("model,sp,mix", fr.configs(), ids=[fr.config_key(*c) for c in fr.configs()])
def test_condensed_dense_and_qp_differences_agree(orc, golden, model, sp, mix):
    p, tw, x0, z = fr.solve_sample(orc, model, sp, mix, fr.SAMPLE_LANES)
    cfg = golden["configs"][fr.config_key(model, sp, mix)]
    assert cfg["seed"] == fr.config_seed(model, sp, mix) and cfg["sample_lanes"] == fr.SAMPLE_LANES
    worst = 0.0
    for b in range(fr.SAMPLE_LANES):   # every lane: none is skipped
        Kd, cond = fr.feedback_gain_ref(orc, p, fr.DYN[model], z[:, b], model=model, want_cond=True)
        Kc = fr.condensed_gain_ref(orc, p, fr.DYN[model], z[:, b], model=model)
        Kq, codes, dz_max = fr.feedback_gain_qp_diff(orc, p, fr.DYN[model], z[:, b], model=model)
        assert all(c == 0 for c in codes), (b, codes)   # the sample's condition: every orc.qp_solve succeeds
        assert Kd.shape == (40, 4 if model == "single" else 6) and np.isfinite(Kd).all()
        bound = cond * EPS
        e_c, e_q = fr.rel_err(Kc, Kd), fr.rel_err(Kq, Kd)
        assert e_c <= bound, (b, e_c, bound)
        assert e_q <= bound * (1.0 + dz_max / np.abs(Kd).max()), (b, e_q, bound)
        worst = max(worst, e_c)
        if tw is not None:   # the per-problem form of the terminal rows gives the same reference
            Kt = fr.feedback_gain_ref(orc, fr.params_for(orc, model, sp), fr.DYN[model], z[:, b], terminal_weights=tw,
                                      model=model)
            assert np.array_equal(Kt, Kd)
        if b < fr.GOLDEN_LANES:   # the committed lanes (stored to 12 / 9 digits)
            np.testing.assert_allclose(np.array(cfg["x0"][b]), x0[:, b], rtol=0, atol=1e-11)
            if b < fr.GOLDEN_Z_LANES:
                np.testing.assert_allclose(np.array(cfg["z"][b]), z[:, b], rtol=0, atol=1e-9 * max(1.0, np.abs(z[:, b]).max()))
            assert fr.rel_err(np.array(cfg["K01"][b]).reshape(2, -1), Kd[:2]) <= 1e-6   # z to 1e-9, K sensitive to z by < 1e3
    print("%s: condensed vs dense, worst of %d lanes: %.3e (recorded %.3e)"
          % (fr.config_key(model, sp, mix), fr.SAMPLE_LANES, worst, cfg["condensed_vs_dense_worst_rel"]))
    # the recorded figure is this computation's: the same order of magnitude on any IEEE machine
    assert worst <= 10.0 * cfg["condensed_vs_dense_worst_rel"] + 1e-15


def test_gain_predicts_the_qp_step_and_the_first_row_is_a_stabilising_law(orc):
    """u(x0 + d) = u + K d exactly for the (linear) QP; K[0] pushes the cart under a falling pole: about
    [100, -100, 28, -12] N per unit of {b_x, th, b_x', th'} at the defaults."""
    model, sp = "single", 10
    p, _, x0, z = fr.solve_sample(orc, model, sp, "default", 4)
    for b in range(4):
        K = fr.feedback_gain_ref(orc, p, fr.DYN[model], z[:, b], model=model)
        assert 30 < K[0, 0] < 300 and -300 < K[0, 1] < -30 and 5 < K[0, 2] < 100 and -50 < K[0, 3] < -2
        d = np.array([0.01, -0.02, 0.03, 0.05])
        r, c, J, A = fr.problem_eval(orc, model, p, fr.DYN[model], z[:4, b], 0.0, 0.0, z[:, b])
        r2, c2, _, _ = fr.problem_eval(orc, model, p, fr.DYN[model], z[:4, b] + d, 0.0, 0.0, z[:, b])
        _, dz = orc.qp_solve(J, r, A, c, 40, 0.0)
        _, dz2 = orc.qp_solve(J, r2, A, c2, 40, 0.0)
        np.testing.assert_allclose((dz2 - dz)[20:], K @ d, rtol=0, atol=1e-7 * np.abs(K).max())


def test_float_emulation_is_the_double_form_at_float_precision(orc):
    """The float32 precision split (Phi, Gamma, Psi, w_k in float32; S and its solve in double) stays within
    cond(S + Dg) * eps_float of the double form: the yardstick of the fp32 GPU test is a sane one."""
    model, sp = "single", 10
    p, _, _, z = fr.solve_sample(orc, model, sp, "default", 8)
    for b in range(8):
        Kd = fr.feedback_gain_ref(orc, p, fr.DYN[model], z[:, b], model=model)
        Kf = fr.condensed_gain_ref(orc, p, fr.DYN[model], z[:, b], model=model, lin=np.float32)
        assert 1e-9 < fr.rel_err(Kf, Kd) < 3e6 * np.finfo(np.float32).eps
