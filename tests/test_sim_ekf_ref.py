"""CPU: the numpy reference of the extended Kalman filter (tests/helpers/sim_ekf_ref.py) pinned, and the conditions the GPU
test's inputs must meet.

1. Sequential against joint: the filter restated as the kernel runs it -- one measured state at a time, no inverse -- agrees with
   the joint update in the Joseph form to 1e-12 of the lane's largest entry on the GPU test's inputs: the same filter.
2. A constant state (dt = 0, diagonal P0, q = 0): P_final = (P0^-1 + sum_t om_t W)^-1 and the matching weighted mean, to 1e-13.
3. The rolling-prior twin of WindowEstimator at dt = 0, window 3, 8 ticks: with the prior it equals that full-information closed
   form over ALL 8 samples; without, the mean of the last 3 samples only -- what the rolling prior adds, made visible.
4. Admissibility of every case the GPU test uses (a condition, not a measurement): every reference P_t has its smallest
   eigenvalue > 0, in the float32 algebra too, and max_i rho_i P_ii <= 1e3 before any update."""
import numpy as np
import pytest

from helpers import sim_ekf_ref as ek
from helpers import sim_jac_ref as sj

NB = 16   # lanes of the CPU checks: the first 16 of the GPU test's draws hold the wrapping and the bumper blocks (nb // 4 each)


def _lane_rel(a, b):
    ax = tuple(range(b.ndim - 1))
    s = np.abs(b).max(axis=ax)
    return float((np.abs(a - b).max(axis=ax) / np.where(s > 0, s, 1.0)).max())


@pytest.mark.parametrize("case", ek.CASES, ids=ek.IDS)
def test_sequential_scalar_updates_are_the_joint_update(orc, case):
    i = ek.inputs(orc, case, NB)
    args = (orc, case[0], i["prm"], case[1], i["x0"], i["P0"], i["us"], i["ys"], i["w"], i["q"], i["om"], i["f"])
    joint = ek.run_batch(*args)
    seq = ek.run_batch(*args, update=ek.sequential_update)
    d = {n: _lane_rel(seq[n], joint[n]) for n in ("xs", "Ps")}
    d["nis"] = float((np.abs(seq["nis"] - joint["nis"]) / np.maximum(np.abs(joint["nis"]), 1.0)).max())
    print("ekf ref %s: sequential against joint, worst lane relative to its largest entry: %s" % (
        ek.IDS[ek.CASES.index(case)], "  ".join("%s %.2e" % kv for kv in d.items())))
    assert max(d.values()) <= 1e-12
    if case[3] != "w0":
        assert (joint["nis"] > 0).all() and not np.array_equal(joint["Ps"], joint["Pms"])   # the update did act


@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("weighted", [False, True])
def test_constant_state_is_the_information_sum(orc, model, weighted):
    nx, nt, nb = sj.NX[model], 6, 8
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-0.5, 0.5, (nx, nb))
    p0 = rng.uniform(0.5, 2.0, (nx, nb)) * ek.prior_covariance(model)[:, None]
    ys = x0[None] + rng.uniform(-0.05, 0.05, (nt, nx, nb))
    w = ek.weights(model)
    w[-1] = 25.0                                   # one velocity measured too, at another variance
    om = rng.uniform(0.0, 2.0, (nt, nb)) if weighted else None
    P0 = np.zeros((nx, nx, nb))
    P0[np.arange(nx), np.arange(nx)] = p0
    got = ek.run_batch(orc, model, sj.DYN[model], 0.0, x0, P0, rng.uniform(-20, 20, (nt, nb)), ys, w, np.zeros(nx), om)
    worst = 0.0
    for b in range(nb):
        mean, var = ek.constant_state(x0[:, b], p0[:, b], ys[:, :, b], w, None if om is None else om[:, b])
        worst = max(worst, np.abs(got["P_final"][:, :, b] - np.diag(var)).max() / var.max(),
                    np.abs(got["x_final"][:, b] - mean).max())
    print("ekf ref %s dt = 0: worst distance from the closed form %.2e" % (model, worst))
    assert worst <= 1e-13


def test_rolling_prior_twin_carries_the_dropped_samples(orc):
    model, window, ticks = "single", 3, 8
    nx = sj.NX[model]
    rng = np.random.default_rng(5)
    guess = np.array([0.2, -1.0, 0.3, -0.4])
    ys = guess[None] + rng.uniform(-0.05, 0.05, (ticks, nx))
    us = rng.uniform(-20, 20, ticks)
    w = np.full(nx, 1.0 / ek.SIGMA ** 2)
    p0 = ek.prior_covariance(model)
    rolling = ek.window_prior_estimates(orc, model, sj.DYN[model], 0.0, guess, us, ys, window, w, iterations=1,
                                        prior_cov=np.diag(p0))
    plain = ek.window_prior_estimates(orc, model, sj.DYN[model], 0.0, guess, us, ys, window, w, iterations=1)
    for t in range(ticks):
        full, _ = ek.constant_state(guess, p0, ys[:t + 1], w)
        assert np.abs(rolling[t] - full).max() <= 1e-12, t
        assert np.abs(plain[t] - ys[max(0, t + 1 - window):t + 1].mean(axis=0)).max() <= 1e-12, t
    # and the two differ by far more than that once samples have been dropped
    assert np.abs(rolling[-1] - plain[-1]).max() >= 1e-3


@pytest.mark.parametrize("case", ek.CASES, ids=ek.IDS)
def test_gpu_cases_are_admissible(orc, case):
    i = ek.inputs(orc, case)   # the GPU test's 130 lanes
    w, om = i["w"], i["om"]
    worst_rho = 0.0
    for dtype in (np.float64, np.float32):
        ref = ek.reference(orc, case, dtype=dtype)
        for name in ("Ps", "Pms"):
            P = np.moveaxis(ref[name], -1, 1)             # [T, B, nx, nx]
            assert np.linalg.eigvalsh(P).min() > 0.0, (name, dtype)
        diag = np.einsum("tiib->tib", ref["Pms"])
        rho = w[None, :, None] * (np.ones_like(diag[:, :1]) if om is None else om[:, None, :])
        worst_rho = max(worst_rho, float((rho * diag).max()))
    print("ekf ref %s: max rho_i P_ii before an update %.1f" % (ek.IDS[ek.CASES.index(case)], worst_rho))
    assert worst_rho <= 1e3
