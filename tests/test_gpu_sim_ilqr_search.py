"""On the GPU: the line search of an iLQR iteration in one launch (cpmpc_sim_ilqr_search_batch; sim_ilqr_search,
sim_ilqr(search="fused"), BatchSimulator.ilqr(search="fused")) against the trial ladder of public calls it replaces.  Every
comparison is GPU against GPU and BIT FOR BIT, so there is no tolerance anywhere in this file: the kernel's roll is
sim_ilqr_forward's own text, and its accept test is written so that it decides as elementwise torch in the same dtype does.
B = 130 (two full waves and a ragged third) for the cases, the loop test's 32 lanes for the loop.

1. The call is the ladder of public calls.  For every case of sim_ilqr_ref.CASES (per-problem parameters and forces, a tensor P_T,
   mu per lane, the binding 2 N limit, T = 1, dt = 0) and both dtypes, with kff, K, dV from sim_ilqr_backward on the GPU's own
   rollout and cost_nom from sim_ilqr_forward: alpha equals, on every lane, the one of the torch ladder written out here from
   sim_ilqr_forward(want="cost") as test_gpu_sim_ilqr.py: test_the_loop_is_the_public_calls_in_its_order writes it, and xs,
   x_final, us, cost equal sim_ilqr_forward with that alpha.  trials = 1, 6 and 32, and K = None.  The distribution of alpha is
   printed: on these cases, whose controls are random, every lane accepts alpha = 1.  So the cases with dt > 0 run once more under
   a prediction that spreads the lanes over the ladder (dV2 = 0, dV1 scaled per lane, armijo = 0.9; the reasoning is at the test):
   the same identities, with failure and at least four rungs present (on an MI355X: all six rungs and failure in every case).
2. The loop.  For the four loop configurations and both dtypes every entry of sim_ilqr(search="fused") equals search="trials"
   (the existing test's bounds against the reference's converged costs then hold for the fused loop with no new figure);
   `accepted` has both values; the replay of the fused loop from public calls, one sim_ilqr_search per iteration, reproduces it
   and its accepted steps take at least four distinct values per configuration.  BatchSimulator.ilqr(search="fused") is
   sim_ilqr's result and leaves the plant's state where it was.
3. Structure.  Failed lanes (forced by handing in dV1 = +1) return the nominal's bits; each output is the same whichever others
   are asked for; inputs are unchanged; a lane's bits do not depend on its place in the batch, under arrangements that move lanes
   between waves that run different numbers of trials; a lane with NaN in kff, K or dV and a finite nominal gets alpha = 0 and its
   nominal's bits back, and every other lane's bits are those of the unpoisoned run; a lane with a non-finite start returns its
   (non-finite) nominal and no other lane is affected."""
import numpy as np
import pytest

from helpers import batch_position as bp
from helpers import sim_ilqr_ref as il
from helpers import sim_jac_ref as sj

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = il.B
CASES, IDS = il.CASES, il.IDS
DTYPES = [torch.float64, torch.float32]
OUTS = ("xs", "x_final", "us", "cost", "alpha")
FW_OUTS = ("xs", "x_final", "us", "cost")
ARMIJO = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    assert pkg.capi.load().cpmpc_device_count() >= 1
    assert callable(pkg.sim_ilqr_search)                                        # fails on a tree without the call


def Tn(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def same_bits(a, b, name="output", idx=None):
    msg = bp.first_difference(a, b, 1, idx, name)
    assert msg is None, msg


_N = {}


def nominal(pkg, orc, case, dtype):
    """-> dict: the case's plant and cost as tensors (p: params, dt, x0, x_ref, u_ref, q, r; kw: model, u_limit, fext, terminal),
    its nominal trajectory from sim_ilqr_forward (us, xs, cost) and sim_ilqr_backward's K, kff, dV along it (with the case's
    mu).  Made once per (case, dtype) and left unchanged."""
    key = (case, dtype)
    if key not in _N:
        i = il.inputs(orc, case)
        kw = dict(model=case[0], u_limit=float(i["u_limit"]))
        if i["f"] is not None:
            kw["fext"] = Tn(i["f"], dtype)
        params = Tn(i["prm"], dtype) if i["prm"].ndim == 2 else [float(v) for v in i["prm"]]
        if i["PT"] is not None:
            kw["terminal"] = Tn(i["PT"], dtype)
        p = dict(params=params, dt=case[1], x0=Tn(i["x0"], dtype), x_ref=Tn(i["x_ref"], dtype), u_ref=Tn(i["u_ref"], dtype),
                 q=[float(v) for v in i["q"]], r=float(i["r"]))
        nom = pkg.sim_ilqr_forward(params, case[1], p["x0"], Tn(i["us"], dtype), None, None, None, None, p["x_ref"], p["u_ref"],
                                   p["q"], p["r"], want=("xs", "us", "cost"), **kw)
        mu = {} if i["mu"] is None else dict(mu=Tn(i["mu"], dtype))
        bw = pkg.sim_ilqr_backward(params, case[1], p["x0"], nom["us"], nom["xs"], p["x_ref"], p["u_ref"], p["q"], p["r"],
                                   want=("K", "kff", "dV"), **kw, **mu)
        _N[key] = dict(p=p, kw=kw, us=nom["us"], xs=nom["xs"], cost=nom["cost"], K=bw["K"], kff=bw["kff"], dV=bw["dV"])
        assert all(torch.isfinite(v).all() for v in _N[key].values() if isinstance(v, torch.Tensor))
    return _N[key]


def forward(pkg, n, alpha, want, **over):
    """sim_ilqr_forward from the nominal start under the nominal's kff and K with a step per lane"""
    a = dict(n, **over)
    p = a["p"]
    return pkg.sim_ilqr_forward(p["params"], p["dt"], a.get("x0", p["x0"]), a["us"], a["kff"], a["K"], a.get("x0", p["x0"]), a["xs"],
                                p["x_ref"], p["u_ref"], p["q"], p["r"], alpha=alpha, want=want, **a["kw"])


def search(pkg, n, trials=6, want=OUTS, armijo=ARMIJO, **over):
    a = dict(n, **over)
    p = a["p"]
    return pkg.sim_ilqr_search(p["params"], p["dt"], a.get("x0", p["x0"]), a["us"], a["xs"], a["cost"], a["kff"], a["K"], a["dV"],
                               p["x_ref"], p["u_ref"], p["q"], p["r"], trials=trials, armijo=armijo, want=want, **a["kw"])


def ladder(pkg, n, trials, ARMIJO=ARMIJO, **over):
    """the trial ladder of sim_ilqr's default loop, from public calls and elementwise torch -> alpha [B] (0: no step)"""
    a = dict(n, **over)
    dtype = a["cost"].dtype
    alpha = torch.ones(B, dtype=dtype, device=DEV)
    done = torch.zeros(B, dtype=torch.bool, device=DEV)
    for _ in range(trials):
        J_try = forward(pkg, n, alpha, "cost", **over)["cost"]
        pred = a["dV"][0] * alpha + a["dV"][1] * alpha * alpha
        done = done | ((pred < 0) & (J_try - a["cost"] <= ARMIJO * pred))
        alpha = torch.where(done, alpha, 0.5 * alpha)
    return torch.where(done, alpha, torch.zeros_like(alpha))


def rolls(alpha, trials):
    """the rolls a lane took: 1 at alpha = 1, j + 1 at 2^-j, `trials` where it took no step"""
    a = alpha.detach().cpu().numpy().astype(np.float64)
    return np.where(a > 0, 1 - np.log2(np.where(a > 0, a, 1.0)), trials).astype(int)


def distribution(alpha):
    v, c = np.unique(alpha.detach().cpu().numpy().astype(np.float64), return_counts=True)
    return "  ".join("%g: %d" % (x, k) for x, k in sorted(zip(v, c), reverse=True))


# ---- 1. the call is the ladder of public calls ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_search_is_the_ladder_of_public_calls(pkg, orc, case, dtype):
    n = nominal(pkg, orc, case, dtype)
    for trials, over in ((1, {}), (6, {}), (32, {}), (6, dict(K=None))):
        alpha = ladder(pkg, n, trials, **over)
        got = search(pkg, n, trials, **over)
        print("ilqr search %s %s trials %d%s: alpha %s" % (IDS[CASES.index(case)], dtype, trials, " K None" if over else "",
                                                          distribution(got["alpha"])))
        same_bits(alpha, got["alpha"], "alpha, trials %d" % trials)
        fin = forward(pkg, n, alpha, FW_OUTS, **over)
        for name in FW_OUTS:
            same_bits(fin[name], got[name], "%s, trials %d" % (name, trials))
        assert all(torch.isfinite(v).all() for v in got.values())
        a = got["alpha"].cpu().numpy()
        assert np.isin(a, [0.0] + [0.5 ** j for j in range(trials)]).all()
        assert (got["cost"] <= n["cost"]).all() and ((got["cost"] < n["cost"]).cpu().numpy() == (a > 0)).all()


# The cases' controls are random, far from any minimum, so there every lane accepts alpha = 1 (the distributions printed above
# show it).  The same cases with a prediction that spreads the lanes over the ladder: dV2 = 0 and dV1 scaled by c per lane, under
# armijo = 0.9.  Where the model is accurate the cost falls by about |dV1| alpha (1 - alpha / 2), so a lane accepts at the first
# alpha with 1 - alpha / 2 >= 0.9 c: c = 0.5 at 1, 0.6 at 1/2, 0.9 at 1/4, 1 at 1/8, 1.05 at 1/16, 1.09 at 1/32, and 1.2 never.
SPREAD_C, SPREAD_ARMIJO = (0.5, 0.6, 0.9, 1.0, 1.05, 1.09, 1.2), 0.9


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in CASES if c[1] > 0], ids=lambda c: "%s-%g-%d-%s" % c)
def test_the_search_is_the_ladder_on_every_rung(pkg, orc, case, dtype):
    n = nominal(pkg, orc, case, dtype)
    c = torch.tensor([SPREAD_C[b % len(SPREAD_C)] for b in range(B)], dtype=dtype, device=DEV)
    dV = torch.stack([n["dV"][0] * c, torch.zeros_like(c)])
    alpha = ladder(pkg, n, 6, ARMIJO=SPREAD_ARMIJO, dV=dV)
    got = search(pkg, n, 6, armijo=SPREAD_ARMIJO, dV=dV)
    print("ilqr search %s %s, the spread prediction: alpha %s" % (IDS[CASES.index(case)], dtype, distribution(got["alpha"])))
    same_bits(alpha, got["alpha"], "alpha")
    fin = forward(pkg, n, alpha, FW_OUTS)
    for name in FW_OUTS:
        same_bits(fin[name], got[name], name)
    took = set(np.unique(got["alpha"].cpu().numpy()))
    assert 0.0 in took and len(took - {0.0}) >= 4                               # failure and at least four rungs


# ---- 2. the loop ------------------------------------------------------------------------------------------------------------
LOOPS =[(m, c) for m in ("single", "double") for c in (False, True)]
LOOP_IDS = ["%s-%s" % (m, "clamped" if c else "free") for m, c in LOOPS]
_LOOP = {}


def loop_run(pkg, model, clamped, dtype):
    key = (model, clamped, dtype)
    if key not in _LOOP:
        x0, u0, target, qf = il.loop_draws(model)
        args = ([float(v) for v in sj.DYN[model]], il.LOOP_DT, Tn(x0, dtype), Tn(u0, dtype), [float(v) for v in target], il.Q[model],
                il.R)
        kw = dict(terminal=qf, u_limit=float(il.loop_limit(model, clamped)), iterations=il.LOOP_ITERS, trials=il.LOOP_TRIALS,
                  model=model)
        _LOOP[key] = (args, kw, pkg.sim_ilqr(*args, search="trials", **kw), pkg.sim_ilqr(*args, search="fused", **kw))
    return _LOOP[key]


def _comparable(t):
    return t.to(torch.int32) if t.dtype == torch.bool else t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model,clamped", LOOPS, ids=LOOP_IDS)
def test_the_fused_loop_is_the_trial_loop(pkg, model, clamped, dtype):
    (params, dt, x0, u0, target, q, r), kw, ref, got = loop_run(pkg, model, clamped, dtype)
    assert set(ref) == set(got)
    for name in ref:
        same_bits(_comparable(ref[name]), _comparable(got[name]), name)
    acc = got["accepted"].cpu().numpy()
    assert acc.any() and not acc.all()
    # the fused loop again from public calls, one search per iteration
    nb = il.LOOP_NB
    ckw = dict(terminal=kw["terminal"], u_limit=kw["u_limit"], model=model)
    first = pkg.sim_ilqr_forward(params, dt, x0, u0, None, None, None, None, target, None, q, r, want=("xs", "us", "cost"), **ckw)
    u, xs, J = first["us"], first["xs"], first["cost"]
    mu = torch.zeros(nb, dtype=dtype, device=DEV)
    hist, steps = [J], []
    for it in range(kw["iterations"]):
        bw = pkg.sim_ilqr_backward(params, dt, x0, u, xs, target, None, q, r, mu=mu, want=("K", "kff", "dV"), **ckw)
        fin = pkg.sim_ilqr_search(params, dt, x0, u, xs, J, bw["kff"], bw["K"], bw["dV"], target, None, q, r, trials=kw["trials"],
                                  **ckw)
        done = fin["alpha"] > 0
        same_bits(got["accepted"][it].to(torch.int32), done.to(torch.int32), "accepted[%d]" % it)
        u, xs, J = fin["us"], fin["xs"], fin["cost"]
        down = mu / 10.0
        mu = torch.where(done, torch.where(down < 1e-6, torch.zeros_like(mu), down), torch.clamp(10.0 * mu, min=1e-3))
        hist.append(J)
        steps.append(fin["alpha"])
    last = pkg.sim_ilqr_backward(params, dt, x0, u, xs, target, None, q, r, mu=mu, want=("K", "hmax"), **ckw)
    for name, mine in (("u", u), ("xs", xs), ("cost", J), ("mu", mu), ("K", last["K"]), ("hmax", last["hmax"]),
                       ("cost_history", torch.stack(hist))):
        same_bits(got[name], mine, name)
    steps = torch.stack(steps)
    print("ilqr fused loop %s %s %s: steps over %d lanes x %d iterations: %s" % (
        model, "clamped" if clamped else "free", dtype, nb, kw["iterations"], distribution(steps)))
    assert len(np.unique(steps[steps > 0].cpu().numpy())) >= 4


def test_the_simulators_fused_ilqr_is_sim_ilqr_on_its_state(pkg):
    (params, dt, x0, u0, target, q, r), kw, _, run = loop_run(pkg, "single", True, torch.float64)
    sim = pkg.BatchSimulator(il.LOOP_NB, dtype=torch.float64, device=0, model="single")
    sim.set_state(x0)
    got = sim.ilqr(params, dt, u0, target, q, r, search="fused", **{k: v for k, v in kw.items() if k != "model"})
    for name in run:
        same_bits(_comparable(run[name]), _comparable(got[name]), name)
    assert torch.equal(sim.get_state(), x0)                                     # a plan: the plant does not move


# ---- 3. structure -----------------------------------------------------------------------------------------------------------
STRUCT = [c for c in CASES if c[1] == 0.0105 and c[2] == 5 and c[3] in ("dyn", "PT", "mu", "limit")]
STRUCT_IDS = ["%s-%g-%d-%s" % c for c in STRUCT]


def forced(n, every):
    """the nominal's dV with dV1 = +1, dV2 = 0 on every `every`-th lane: those lanes take no step"""
    lanes = np.arange(1, B, every)
    dV = n["dV"].clone()
    dV[0, lanes] = 1.0
    dV[1, lanes] = 0.0
    return dV, lanes


def nominal_bits_on(n, got, lanes, what):
    for name, nom in (("xs", n["xs"]), ("us", n["us"]), ("cost", n["cost"]), ("x_final", n["xs"][-1])):
        same_bits(bp.take(nom, lanes), bp.take(got[name], lanes), "%s of %s" % (name, what))
    assert (bp.take(got["alpha"], lanes) == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT + [c for c in CASES if c[2] == 1], ids=lambda c: "%s-%g-%d-%s" % c)
def test_failed_lanes_return_the_nominals_bits(pkg, orc, case, dtype):
    n = nominal(pkg, orc, case, dtype)
    clean = search(pkg, n)
    dV, lanes = forced(n, 3)
    got = search(pkg, n, dV=dV)
    nominal_bits_on(n, got, lanes, "the lanes forced to fail")
    others = np.setdiff1d(np.arange(B), lanes)
    for name in OUTS:
        same_bits(bp.take(clean[name], others), bp.take(got[name], others), name + " of the other lanes")
    every = search(pkg, n, dV=torch.stack([torch.ones_like(dV[0]), torch.zeros_like(dV[1])]))
    nominal_bits_on(n, every, np.arange(B), "every lane")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_outputs_do_not_depend_on_each_other_and_the_inputs_are_read_only(pkg, orc, case, dtype):
    n = nominal(pkg, orc, case, dtype)
    dV, _ = forced(n, 3)
    held = [v for v in list(n.values()) + list(n["p"].values()) + list(n["kw"].values()) + [dV] if isinstance(v, torch.Tensor)]
    before = [v.clone() for v in held]
    got = search(pkg, n, dV=dV)
    for name in OUTS:
        same_bits(got[name], search(pkg, n, dV=dV, want=name)[name], name + " alone")
    pair = search(pkg, n, dV=dV, want=("cost", "x_final"))
    same_bits(got["cost"], pair["cost"], "cost beside x_final")
    same_bits(got["x_final"], pair["x_final"], "x_final beside cost")
    same_bits(got["xs"][-1], got["x_final"], "xs[-1]")
    for a, b in zip(held, before):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT, ids=STRUCT_IDS)
def test_a_lanes_bits_do_not_depend_on_its_place_in_the_batch(pkg, orc, case, dtype):
    """trials = 32 and every fourth lane forced to fail: a wave that holds one of those rolls 32 times, one that holds none as
    often as its slowest lane needs.  `sorted` gathers the lanes by the rolls they take, so its first wave leaves early and its
    later ones late; reverse and shuffle mix them again; the prefixes end alone, below, on and above a wave boundary."""
    n = nominal(pkg, orc, case, dtype)
    trials = 32
    dV, _ = forced(n, 4)
    natural = search(pkg, n, trials, dV=dV)
    took = rolls(natural["alpha"], trials)
    by_rolls = np.argsort(took, kind="stable").astype(np.int64)
    waves = [took[by_rolls[w:w + 64]].max() for w in range(0, B, 64)]
    assert waves[0] < waves[1] == trials, waves                                 # waves that run different numbers of trials
    arrangements = dict(bp.permutations(B, 7), sorted=by_rolls)

    def arranged(idx):
        take = lambda v: bp.take(v, idx) if isinstance(v, torch.Tensor) else v  # noqa: E731
        m = {k: take(v) for k, v in n.items() if k not in ("p", "kw")}
        m["p"] = {k: take(v) for k, v in n["p"].items()}
        m["kw"] = {k: take(v) for k, v in n["kw"].items()}
        return search(pkg, m, trials, dV=take(dV))
    for name, idx in arrangements.items():
        got = arranged(idx)
        for out in OUTS:
            same_bits(natural[out], bp.put_back(got[out], idx), "%s %s" % (out, name), idx)
    for nb in (1, 63, 64, 65):
        idx = np.arange(nb, dtype=np.int64)
        got = arranged(idx)
        for out in OUTS:
            same_bits(bp.take(natural[out], idx), got[out], "%s of the first %d" % (out, nb))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT[:1] + STRUCT[4:5], ids=STRUCT_IDS[:1] + STRUCT_IDS[4:5])
def test_a_lane_with_a_poisoned_step_fails_and_keeps_its_nominal(pkg, orc, case, dtype):
    n = nominal(pkg, orc, case, dtype)
    clean = search(pkg, n)
    lane = 70
    others = np.array([b for b in range(B) if b != lane], dtype=np.int64)
    for field, at in (("kff", (2, lane)), ("K", (1, 1, lane)), ("dV", (0, lane)), ("dV", (1, lane))):
        for value in (float("nan"), float("inf")):
            bad = n[field].clone()
            bad[at] = value
            got = search(pkg, n, **{field: bad})
            nominal_bits_on(n, got, np.array([lane]), "the lane with %s = %s" % (field, value))
            for name in OUTS:
                same_bits(bp.take(clean[name], others), bp.take(got[name], others), "%s, %s poisoned" % (name, field))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", STRUCT[:1] + STRUCT[4:5], ids=STRUCT_IDS[:1] + STRUCT_IDS[4:5])
def test_a_lane_with_a_non_finite_start_returns_its_nominal_and_stays_in_its_lane(pkg, orc, case, dtype):
    n = nominal(pkg, orc, case, dtype)
    clean = search(pkg, n)
    lane = 70
    others = np.array([b for b in range(B) if b != lane], dtype=np.int64)
    p = n["p"]
    x0 = p["x0"].clone()
    x0[1, lane] = float("nan")
    # the nominal and the step of that start, as a loop would have them: the lane's are non-finite, the others' are the clean ones
    nom = pkg.sim_ilqr_forward(p["params"], p["dt"], x0, n["us"], None, None, None, None, p["x_ref"], p["u_ref"], p["q"], p["r"],
                               want=("xs", "us", "cost"), **n["kw"])
    bw = pkg.sim_ilqr_backward(p["params"], p["dt"], x0, nom["us"], nom["xs"], p["x_ref"], p["u_ref"], p["q"], p["r"],
                               want=("K", "kff", "dV"), **n["kw"])
    assert torch.isnan(nom["cost"][lane]) and torch.isnan(nom["xs"][:, :, lane]).any()
    got = search(pkg, n, x0=x0, us=nom["us"], xs=nom["xs"], cost=nom["cost"], K=bw["K"], kff=bw["kff"], dV=bw["dV"])
    for name in OUTS:
        same_bits(bp.take(clean[name], others), bp.take(got[name], others), name)
    assert got["alpha"][lane] == 0
    for name, nominal_value in (("xs", nom["xs"]), ("us", nom["us"]), ("cost", nom["cost"]), ("x_final", nom["xs"][-1])):
        same_bits(nominal_value[..., lane:lane + 1].contiguous(), got[name][..., lane:lane + 1].contiguous(), name + " of the lane")
    assert torch.isnan(got["cost"][lane]) and torch.isnan(got["xs"][:, :, lane]).any() and torch.isnan(got["x_final"][:, lane]).any()
