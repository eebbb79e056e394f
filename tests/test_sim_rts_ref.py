"""CPU: the numpy reference of the Rauch-Tung-Striebel smoother (tests/helpers/sim_rts_ref.py) pinned, and the conditions the GPU
test's inputs must meet.

1. A linear plant (dt = 0: A = I) with process noise on every state: the smoother's means and covariances are the marginals of
   the joint Gaussian of x_0 .. x_T, solved as one block-tridiagonal information system -- another formulation altogether.
2. A constant state (dt = 0, diagonal P0, q = 0): the smoothed state at EVERY index is sim_ekf_ref.constant_state's mean and
   variances, to the EKF test's 8 (T + 1) eps of the sums plus T eps pi on the pole angles (compared modulo 2 pi).  The sum
   behind a smoothed variance is P_t + G (P^s_{t+1} - P-_{t+1}) G^T with G = I here: its terms have the size of the FILTERED
   variance of index t, which at index 0 is P0_ii, a thousand times the result -- so the variances of index t are held to
   8 (T + 1) eps of that index's filtered variance (helpers.sim_rts_ref.filtered_variances), the largest term that enters,
   where the filter's own test has the result's size.
3. P0 = 0: the first tick's P- = diag(q) is not positive definite, that tick takes G = 0, so index 0 is smoothed = filtered and
   ok is 0; the later indices are smoothed as ever.
4. Admissibility of every case the GPU test uses, on its first 16 lanes (conditions, not measurements): the smallest pivot of
   the scaled P- at least 1e-3 (the floor is 5.7e-6 in float32), every P^s positive definite, max |G| <= 16, the
   float32-algebra gap at most 1e-5 of the lane's largest entry, and tr P^s_0 / tr P0 below 0.9 where something is measured
   and exactly 1 where nothing is: smoothing visibly acts, so the GPU comparison is not vacuous.
5. The GPU test's float32 bound on the covariances, made here from the helper alone exactly as that test makes it (8 x the
   float32-algebra gap of the lane's largest entry plus e reach_P entry by entry), is a small fraction of what it bounds: at
   every index at most 1e-2 of the lane's largest entry of P^s AT THAT INDEX (at most 5.1e-3 came out), so a covariance of
   zeros, of the wrong sign or of another magnitude is beyond it.  Where ticks go unmeasured ("w0", and the lanes of "tw" whose
   tick weights are mostly exact zeros) the limit is 1e-1: there P^s - P- is an exact zero and the reach, which adds the
   errors of P^s and P- as if independent, overstates (6.1e-2 at index 0 of "w0"; on all 130 lanes of the GPU test 7.1e-2, and
   2.0e-2 for "tw"); the GPU test holds unmeasured covariances to the filter's, bit for bit, besides.  The states' bound is held the same way to 1e-2 of
   max(1, |x|)."""
import numpy as np
import pytest

from helpers import sim_ekf_ref as ek
from helpers import sim_jac_ref as sj
from helpers import sim_rts_ref as rt

NB = 16


def _lane_rel(a, b):
    ax = tuple(range(b.ndim - 1))
    s = np.abs(b).max(axis=ax)
    return float((np.abs(a - b).max(axis=ax) / np.where(s > 0, s, 1.0)).max())


@pytest.mark.parametrize("model", ["single", "double"])
def test_linear_plant_is_the_joint_gaussians_marginals(orc, model):
    nx, nt, nb = sj.NX[model], 5, 4
    rng = np.random.default_rng(11)
    x0 = rng.uniform(-0.3, 0.3, (nx, nb))
    P0 = ek.covariances(model, nb)
    ys = x0[None] + rng.uniform(-0.05, 0.05, (nt, nx, nb))
    us = rng.uniform(-20, 20, (nt, nb))
    w = ek.weights(model)
    w[-1] = 25.0
    q = np.full(nx, 1e-4)
    om = rng.uniform(0.0, 2.0, (nt, nb))
    om[2] = 0.0                                   # one sample missing altogether
    got = rt.run_batch(orc, model, sj.DYN[model], 0.0, x0, P0, us, ys, w, q, om)
    assert (got["ok"] == 1).all()
    worst = 0.0
    Qi = np.diag(1.0 / q)
    for b in range(nb):
        n = nx * (nt + 1)
        J, h = np.zeros((n, n)), np.zeros(n)
        Pi = np.linalg.inv(P0[:, :, b])
        J[:nx, :nx] += Pi
        h[:nx] += Pi @ x0[:, b]
        for t in range(nt):
            a, c = slice(t * nx, (t + 1) * nx), slice((t + 1) * nx, (t + 2) * nx)
            J[a, a] += Qi
            J[c, c] += Qi
            J[a, c] -= Qi
            J[c, a] -= Qi
            J[c, c] += np.diag(om[t, b] * w)
            h[c] += om[t, b] * w * ys[t, :, b]
        cov = np.linalg.inv(J)
        mean = cov @ h
        for t in range(nt + 1):
            a = slice(t * nx, (t + 1) * nx)
            worst = max(worst, np.abs(got["xs_smooth"][t, :, b] - mean[a]).max(),
                        np.abs(got["Ps_smooth"][t, :, :, b] - cov[a, a]).max() / np.abs(cov[a, a]).max())
    print("rts ref %s, linear plant: worst distance from the joint Gaussian's marginals %.2e" % (model, worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("weighted", [False, True])
def test_constant_state_is_the_information_sum_at_every_index(orc, model, weighted):
    nx, nt, nb = sj.NX[model], 6, 8
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-0.5, 0.5, (nx, nb))
    p0 = rng.uniform(0.5, 2.0, (nx, nb)) * ek.prior_covariance(model)[:, None]
    ys = x0[None] + rng.uniform(-0.05, 0.05, (nt, nx, nb))
    w = ek.weights(model)
    w[-1] = 25.0
    om = rng.uniform(0.0, 2.0, (nt, nb)) if weighted else None
    P0 = np.zeros((nx, nx, nb))
    P0[np.arange(nx), np.arange(nx)] = p0
    got = rt.run_batch(orc, model, sj.DYN[model], 0.0, x0, P0, rng.uniform(-20, 20, (nt, nb)), ys, w, np.zeros(nx), om)
    eps = np.finfo(np.float64).eps
    tol = 8 * (nt + 1) * eps
    wrap = np.array([nt * eps * np.pi if 1 <= i < nx // 2 else 0.0 for i in range(nx)])
    worst_x = worst_p = 0.0
    for b in range(nb):
        o = None if om is None else om[:, b]
        mean, var = ek.constant_state(x0[:, b], p0[:, b], ys[:, :, b], w, o)
        mag, _ = ek.constant_state(np.abs(x0[:, b]), p0[:, b], np.abs(ys[:, :, b]), w, o)
        filtered = rt.filtered_variances(p0[:, b], w, o, nt)
        assert np.abs(filtered[0] / p0[:, b] - 1.0).max() <= 1e-12 and np.abs(filtered[nt] / var - 1.0).max() <= 1e-12
        for t in range(nt + 1):
            d = got["xs_smooth"][t, :, b] - mean
            d[1:nx // 2] -= 2 * np.pi * np.round(d[1:nx // 2] / (2 * np.pi))
            worst_x = max(worst_x, (np.abs(d) / (tol * mag + wrap)).max())
            P = got["Ps_smooth"][t, :, :, b]
            worst_p = max(worst_p, (np.abs(np.diag(P) - var) / (tol * filtered[t])).max())
            assert np.abs(P - np.diag(np.diag(P))).max() <= tol * filtered[t].max()
    print("rts ref %s dt = 0 weighted=%s: worst distance from the closed form / bound: x %.3f, P %.3f" % (
        model, weighted, worst_x, worst_p))
    assert worst_x <= 1.0 and worst_p <= 1.0


@pytest.mark.parametrize("case", [ek.CASES[0], ek.CASES[4]], ids=[ek.IDS[0], ek.IDS[4]])
def test_a_known_start_falls_back_to_the_filtered_values(orc, case):
    i = ek.inputs(orc, case, NB)
    P0 = np.zeros_like(i["P0"])
    got = rt.run_batch(orc, case[0], i["prm"], case[1], i["x0"], P0, i["us"], i["ys"], i["w"], i["q"], i["om"], i["f"])
    assert (got["ok"] == 0).all()
    assert np.array_equal(got["xs_smooth"][0], i["x0"]) and (got["Ps_smooth"][0] == 0).all()
    assert (got["G"][0] == 0).all() and (np.abs(got["G"][1:]).max(axis=(0, 1, 2)) > 0).all()     # the later ticks do smooth
    assert not np.array_equal(got["xs_smooth"][1:-1], got["xs"][:-1])


@pytest.mark.parametrize("case", ek.CASES, ids=ek.IDS)
def test_gpu_cases_are_admissible(orc, case):
    i = ek.inputs(orc, case, NB)
    args = (orc, case[0], i["prm"], case[1], i["x0"], i["P0"], i["us"], i["ys"], i["w"], i["q"], i["om"], i["f"])
    ref, r32 = rt.run_batch(*args), rt.run_batch(*args, dtype=np.float32)
    assert (ref["ok"] == 1).all() and (r32["ok"] == 1).all()
    eig = np.linalg.eigvalsh(np.moveaxis(ref["Ps_smooth"], -1, 1)).min()
    gaps = {n: _lane_rel(r32[n], ref[n]) for n in ("xs_smooth", "Ps_smooth")}
    ratio = np.einsum("iib->b", ref["Ps_smooth"][0]) / np.einsum("iib->b", i["P0"])
    print("rts ref %s: smallest pivot of the scaled P- %.2e, smallest eigenvalue of a P^s %.2e, max |G| %.2f, float32-algebra gap "
          "%s, tr P^s_0 / tr P0 in [%.3f, %.3f]" % (ek.IDS[ek.CASES.index(case)], ref["min_pivot"].min(), eig,
                                                    np.abs(ref["G"]).max(), "  ".join("%s %.2e" % kv for kv in gaps.items()),
                                                    ratio.min(), ratio.max()))
    assert ref["min_pivot"].min() >= 1e-3 and r32["min_pivot"].min() >= 1e-3
    assert eig > 0.0
    assert np.abs(ref["G"]).max() <= 16.0
    assert max(gaps.values()) <= 1e-5
    if case[3] == "w0":
        assert np.array_equal(ref["xs_smooth"][1:], ref["xs"]) and np.array_equal(ref["xs_smooth"][0], i["x0"])
        assert np.abs(ratio - 1.0).max() <= 1e-12
    else:
        assert ratio.max() < 0.9


@pytest.mark.parametrize("case", ek.CASES, ids=ek.IDS)
def test_the_float32_bound_is_a_small_fraction_of_what_it_bounds(orc, case):
    model, dt, nt, kind = case
    i = ek.inputs(orc, case, NB)
    held = {k: v.astype(np.float32).astype(np.float64) if isinstance(v, np.ndarray) and k not in ("w", "q") else v
            for k, v in i.items()}                                # what float tensors hold, as the GPU test's reference takes them
    args = (orc, model, held["prm"], dt, held["x0"], held["P0"], held["us"], held["ys"], held["w"], held["q"], held["om"], held["f"])
    ref, r32 = rt.run_batch(*args), rt.run_batch(*args, dtype=np.float32)
    state = 4 * nt * max(len(sj.sub_steps(dt)), 1) * np.finfo(np.float32).eps
    P, x = ref["Ps_smooth"], ref["xs_smooth"]
    lane = np.abs(P).max(axis=(0, 1, 2))
    gap = (np.abs(r32["Ps_smooth"] - P).max(axis=(0, 1, 2)) / lane).max()
    bound = 8 * gap * lane + state * ref["reach_P"]                                 # [T+1, nx, nx, B], as the GPU test makes it
    frac = (bound.max(axis=(1, 2)) / np.abs(P).max(axis=(1, 2))).max(axis=1)        # per index, worst lane
    gap_x = (np.abs(r32["xs_smooth"] - x).max(axis=(0, 1)) / np.abs(x).max(axis=(0, 1))).max()
    frac_x = ((8 * gap_x * np.abs(x).max(axis=(0, 1)) + state * ref["reach_x"]) / np.maximum(1.0, np.abs(x))).max(axis=(1, 2))
    print("rts ref %s: the float32 bound on Ps_smooth[t] over the lane's largest entry of index t = 0 .. T: %s; on xs_smooth[t] "
          "over max(1, |x|): %s" % (ek.IDS[ek.CASES.index(case)], " ".join("%.1e" % v for v in frac),
                                    " ".join("%.1e" % v for v in frac_x)))
    assert (bound > 0).all() and np.isfinite(bound).all()
    assert frac.max() <= (1e-1 if kind in ("w0", "tw") else 1e-2)
    assert frac_x.max() <= 1e-2
