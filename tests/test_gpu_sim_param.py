"""Per-problem plant parameters and the plant step's derivative in them on the GPU (cpmpc_sim_step_dyn_batch,
cpmpc_sim_step_param_jac_batch; sim_step_param_jacobian, sim_step_param_vjp, sim_step / BatchSimulator with a parameter
tensor, ClosedLoop.tick(plant_dyn=...), pypendulum.Simulator.step_param_jacobian) against the numpy reference of
tests/helpers/sim_param_ref.py -- Richardson-extrapolated central differences of the CPU oracle's simulator, which
tests/test_sim_param_ref.py pins.

Shapes: B = 130 -- two full waves and a 2-lane tail -- and B = 1; dt 0, 0.001, 0.0025, 0.0105 (0 / 1 / 3 / 11 sub-steps); both
models, both dtypes; the states of sim_jac_ref.states (a block of lanes wraps inside the step; for the 4-state model a block
sits beyond the bumpers); one case with per-problem forces.
fp64: |P - P_ref| <= 1e-7 max |P_ref| per lane (the reference's own two step sizes agree to 5.6e-9 / 8.0e-10), x_new at the
simulator's 1e-12.  fp32: per lane the distance of P from the fp64 kernel's P at the same float-rounded inputs, relative to
max |P|; its median and 99th percentile at most 8 x those of the existing call's fp32 Bu against its fp64 Bu.
Every test prints its figures before it asserts; DESIGN.md section 5f is where they are recorded."""
import numpy as np
import pytest

from conftest import random_states
from helpers import sim_jac_ref as sj
from helpers import sim_param_ref as sp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = 130
DTS = (0.001, 0.0025, 0.0105)
CASES = [(m, dt, None) for m in ("single", "double") for dt in DTS] + [("single", 0.0105, "per")]
OUTS = ("x_new", "P", "gp", "gx", "gu")


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1
    assert callable(pkg.sim_step_param_jacobian)   # imports the batch module


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _forces(kind, nb):
    if kind == "per":
        return np.random.default_rng(21).uniform(-3.0, 3.0, (4, nb))
    return None


def _kw(f, dtype):
    return {} if f is None else dict(fext=T(f, dtype))


def _columns(model, nb, spread=0.0, seed=41):
    """[np, nb] parameters: DYN in every column, each entry scaled by 1 +- spread"""
    d = np.tile(np.array(sj.DYN[model])[:, None], (1, nb))
    if spread:
        d = d * np.random.default_rng(seed).uniform(1.0 - spread, 1.0 + spread, d.shape)
    return d


_REF = {}


def reference(orc, model, dt, kind, nb=B):
    """(x, u, x_new, P_ref) of the fp64 numpy reference with the shared set DYN, computed once per case, left unchanged."""
    key = (model, dt, kind, nb)
    if key not in _REF:
        x, u = sj.states(model, nb)
        f = _forces(kind, nb)
        _REF[key] = (x, u, sp.plant_batch(orc, model, sj.DYN[model], dt, x, u, f),
                     sp.param_jacobian_batch(orc, model, sj.DYN[model], dt, x, u, fext=f))
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _all_outputs(pkg, model, dt, params, x, u, g, **kw):
    """One call with every output of cpmpc_sim_param_jac asked for."""
    return pkg.batch._sim_param_call(params, dt, x, u, kw.get("fext"), (0.0, 0.0), (0.0, 0.0), model, g, OUTS)


# ---- accuracy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,dt,kind", CASES)
def test_fp64_matches_reference(pkg, orc, model, dt, kind):
    x, u, xr, Pr = reference(orc, model, dt, kind)
    res = pkg.sim_step_param_jacobian(sj.DYN[model], dt, T(x), T(u), model=model, **_kw(_forces(kind, B), torch.float64))
    P = N_(res["P"])
    e = sp.lane_err(P, Pr)
    ex = np.abs(N_(res["x_new"]) - xr).max()
    print("fp64 %s dt=%g forces=%s: |P - P_ref| / max|P_ref| worst lane %.2e, median %.2e (bound 1e-7)  |x-ref| %.2e (bound 1e-12)"
          % (model, dt, kind, e.max(), np.median(e), ex))
    wrapped = (np.abs(xr[1:sj.NX[model] // 2] - x[1:sj.NX[model] // 2]) > 3.0).any(axis=0)
    assert wrapped[:2].all(), "lanes 0 and 1 did not wrap inside the step"
    if model == "single":
        off = (Pr[:, sp.COL_XS] == 0.0).all(axis=0) & (Pr[:, sp.COL_KS] == 0.0).all(axis=0)
        assert (np.abs(x[0]) > sj.BUMPER_X).sum() >= B // 4 and off.sum() >= B // 2 and (~off).sum() >= B // 4
        assert (P[:, sp.COL_XS][:, off] == 0.0).all() and (P[:, sp.COL_KS][:, off] == 0.0).all()
    assert e.max() <= 1e-7 and ex <= 1e-12


@pytest.mark.parametrize("model", ["single", "double"])
def test_fp64_single_problem(pkg, orc, model):
    x, u, xr, Pr = reference(orc, model, 0.0105, None, nb=1)
    res = pkg.sim_step_param_jacobian(sj.DYN[model], 0.0105, T(x), T(u), model=model)
    assert sp.lane_err(N_(res["P"]), Pr).max() <= 1e-7
    assert np.abs(N_(res["x_new"]) - xr).max() <= 1e-12
    g = T(np.random.default_rng(2).uniform(-1, 1, (sj.NX[model], 1)))
    v = pkg.sim_step_param_vjp(sj.DYN[model], 0.0105, T(x), T(u), g, model=model)
    assert v["p"].shape == (sp.NP[model], 1) and v["x"].shape == (sj.NX[model], 1) and v["u"].shape == (1,)
    assert np.abs(N_(v["p"])[:, 0] - N_(res["P"])[:, :, 0].T @ N_(g)[:, 0]).max() <= 1e-12 * np.abs(Pr).max()


def _stats(e):
    return np.median(e), np.percentile(e, 99)


@pytest.mark.parametrize("model,dt", [(m, dt) for m in ("single", "double") for dt in DTS])
def test_fp32_within_eight_times_the_existing_control_column(pkg, model, dt):
    """The yardstick is the parent's own tangent column through the same chain: the existing call's fp32 Bu against its fp64
    Bu at the same float-rounded states.  8 = the project's 4 x, doubled: the stage partials da/dp are sums of several
    cancelling terms where da/du is one quotient."""
    x, u = sj.states(model, B)
    x32, u32 = T(x, torch.float32), T(u, torch.float32)
    x64, u64 = x32.double(), u32.double()
    P32 = N_(pkg.sim_step_param_jacobian(sj.DYN[model], dt, x32, u32, model=model, want="P")["P"])
    P64 = N_(pkg.sim_step_param_jacobian(sj.DYN[model], dt, x64, u64, model=model, want="P")["P"])
    B32 = N_(pkg.sim_step_jacobian(sj.DYN[model], dt, x32, u32, model=model, want="Bu")["Bu"])
    B64 = N_(pkg.sim_step_jacobian(sj.DYN[model], dt, x64, u64, model=model, want="Bu")["Bu"])
    pm, pp = _stats(sp.lane_err(P32, P64))
    bm, bp = _stats(sp.lane_err(B32, B64))
    print("fp32 %s dt=%g: P median %.2e p99 %.2e | existing Bu median %.2e p99 %.2e | ratios %.2f / %.2f (bound 8)"
          % (model, dt, pm, pp, bm, bp, pm / bm, pp / bp))
    assert pm <= 8 * bm and pp <= 8 * bp


# ---- the VJP against the same call's P ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["single", "double"])
def test_vjp_is_the_jacobians_transpose(pkg, model, dtype):
    nx = sj.NX[model]
    eps = float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)
    dt = 0.0105
    x, u = sj.states(model, B)
    xt, ut = T(x, dtype), T(u, dtype)
    P = N_(pkg.sim_step_param_jacobian(sj.DYN[model], dt, xt, ut, model=model, want="P")["P"])
    cots = [np.random.default_rng(31).uniform(-1.0, 1.0, (nx, B))]
    for r in range(nx):
        e = np.zeros((nx, B))
        e[r] = 1.0
        cots.append(e)
    worst = 0.0
    for g in cots:
        gt = T(g, dtype)
        g64 = N_(gt)
        gp = N_(pkg.sim_step_param_vjp(sj.DYN[model], dt, xt, ut, gt, model=model, want="p")["p"])
        bound = 4 * nx * eps * np.einsum("rjb,rb->jb", np.abs(P), np.abs(g64))
        d = np.abs(gp - np.einsum("rjb,rb->jb", P, g64))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, np.nanmax(np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0))))
        assert (d <= bound).all()
    print("vjp %s %s: worst |gp - P^T g| / bound %.3f" % (model, dtype, worst))


# ---- per-problem parameters against the shared set ---------------------------------------------------------------------
@pytest.mark.parametrize("model", ["single", "double"])
def test_equal_columns_are_the_shared_set(pkg, orc, model):
    dt = 0.0105
    x, u = sj.states(model, B)
    cols = _columns(model, B)
    sh = pkg.sim_step_param_jacobian(sj.DYN[model], dt, T(x), T(u), model=model)
    pl = pkg.sim_step_param_jacobian(T(cols), dt, T(x), T(u), model=model)
    ex = (pl["x_new"] - sh["x_new"]).abs().max().item()
    ep = sp.lane_err(N_(pl["P"]), N_(sh["P"])).max()
    print("fp64 %s per-problem (equal columns) against shared: |x| %.2e (bound 1e-12)  P %.2e of max|P| (bound 1e-7)" % (model, ex, ep))
    assert ex <= 1e-12 and ep <= 1e-7
    # the plain step
    a, b = T(x), T(x)
    sim = pkg.BatchSimulator(B, dtype=torch.float64, device=0, model=model)
    sim.set_state(a)
    sim.step(T(cols), dt, T(u))
    twin = pkg.BatchSimulator(B, dtype=torch.float64, device=0, model=model)
    twin.set_state(b)
    twin.step(sj.DYN[model], dt, T(u))
    assert (sim.get_state() - twin.get_state()).abs().max().item() <= 1e-12
    # fp32: each side's distance from the fp64 call at the same float-rounded inputs
    x32, u32 = T(x, torch.float32), T(u, torch.float32)
    ref = N_(pkg.sim_step_param_jacobian(sj.DYN[model], dt, x32.double(), u32.double(), model=model, want="P")["P"])
    s32 = N_(pkg.sim_step_param_jacobian(sj.DYN[model], dt, x32, u32, model=model, want="P")["P"])
    p32 = N_(pkg.sim_step_param_jacobian(T(cols, torch.float32), dt, x32, u32, model=model, want="P")["P"])
    (sm, s99), (pm, p99) = _stats(sp.lane_err(s32, ref)), _stats(sp.lane_err(p32, ref))
    print("fp32 %s from fp64: shared median %.2e p99 %.2e | per-problem median %.2e p99 %.2e | ratios %.2f / %.2f (bound 4)"
          % (model, sm, s99, pm, p99, pm / sm, p99 / s99))
    assert pm <= 4 * sm and p99 <= 4 * s99


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["single", "double"])
def test_without_dyn_the_new_calls_are_the_old_ones_bitwise(pkg, model, dtype):
    capi, lib = pkg.capi, pkg.capi.load()
    import ctypes as C
    dt = 0.0105
    x, u = sj.states(model, B)
    xt, ut = T(x, dtype), T(u, dtype)
    g = T(np.random.default_rng(4).uniform(-1.0, 1.0, x.shape), dtype)
    new = pkg.sim_step_param_vjp(sj.DYN[model], dt, xt, ut, g, model=model, want=("x", "u"))
    old = pkg.sim_step_vjp(sj.DYN[model], dt, xt, ut, g, model=model)
    assert torch.equal(new["x"], old["x"]) and torch.equal(new["u"], old["u"])
    with_p = pkg.sim_step_param_vjp(sj.DYN[model], dt, xt, ut, g, model=model)
    assert torch.equal(with_p["x"], old["x"]) and torch.equal(with_p["u"], old["u"])
    a, b = xt.clone(), xt.clone()
    m, _, npar = pkg.batch._model_dims(model)
    cd = capi.F32 if dtype == torch.float32 else capi.F64
    arr = capi.dbl_array(sj.DYN[model], npar)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(lib.cpmpc_sim_step_dyn_batch(m, cd, B, arr, None, dt, C.c_void_p(ut.data_ptr()), None, None,
                                            C.c_void_p(a.data_ptr()), st))
    capi.check(lib.cpmpc_sim_step_batch_model(m, cd, B, arr, dt, C.c_void_p(ut.data_ptr()), None, None,
                                              C.c_void_p(b.data_ptr()), st))
    assert torch.equal(a, b) and not torch.equal(a, xt)


@pytest.mark.parametrize("model", ["single", "double"])
def test_differing_columns_are_single_lane_calls_with_each_lanes_set(pkg, model):
    """Parameters +-20 % per lane: the batch equals B single-lane calls with that lane's parameters as the shared set."""
    dt = 0.0105
    x, u = sj.states(model, B)
    cols = _columns(model, B, spread=0.2)
    g = np.random.default_rng(12).uniform(-1.0, 1.0, x.shape)
    res = _all_outputs(pkg, model, dt, T(cols), T(x), T(u), T(g))
    sim = pkg.BatchSimulator(B, dtype=torch.float64, device=0, model=model)
    sim.set_state(T(x))
    sim.step(T(cols), dt, T(u))
    plain = N_(sim.get_state())
    ex = ep = eg = es = 0.0
    for b in range(B):
        one = _all_outputs(pkg, model, dt, [float(v) for v in cols[:, b]], T(x[:, b:b + 1]), T(u[b:b + 1]), T(g[:, b:b + 1]))
        ex = max(ex, (one["x_new"][:, 0] - res["x_new"][:, b]).abs().max().item())
        scale = one["P"].abs().max().item()
        ep = max(ep, (one["P"][..., 0] - res["P"][..., b]).abs().max().item() / scale)
        for name in ("gp", "gx", "gu"):
            eg = max(eg, (one[name][..., 0] - res[name][..., b]).abs().max().item() / max(one[name].abs().max().item(), 1e-300))
        lone = pkg.BatchSimulator(1, dtype=torch.float64, device=0, model=model)
        lone.set_state(T(x[:, b:b + 1]))
        lone.step([float(v) for v in cols[:, b]], dt, T(u[b:b + 1]))
        es = max(es, np.abs(N_(lone.get_state())[:, 0] - plain[:, b]).max())
    print("fp64 %s parameters +-20%%: batch against single-lane shared calls |x| %.2e, plain step %.2e (bound 1e-12)  P %.2e, "
          "gradients %.2e (bound 1e-7)" % (model, ex, es, ep, eg))
    assert ex <= 1e-12 and es <= 1e-12 and ep <= 1e-7 and eg <= 1e-7


# ---- bitwise properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model,kind,per_problem", [("single", "per", True), ("single", None, False), ("double", None, True),
                                                    ("double", None, False)])
def test_outputs_do_not_depend_on_each_other_and_the_inputs_are_read_only(pkg, model, kind, per_problem, dtype):
    dt = 0.0025
    x, u = sj.states(model, B)
    kw = _kw(_forces(kind, B), dtype)
    xt, ut = T(x, dtype), T(u, dtype)
    params = T(_columns(model, B, spread=0.2), dtype) if per_problem else sj.DYN[model]
    keep_x = xt.clone()
    keep_p = params.clone() if per_problem else None
    g = T(np.random.default_rng(5).uniform(-1.0, 1.0, x.shape), dtype)
    both = _all_outputs(pkg, model, dt, params, xt, ut, g, **kw)
    again = _all_outputs(pkg, model, dt, params, xt, ut, g, **kw)
    for name in both:
        assert torch.equal(both[name], again[name]), name
    for name in ("x_new", "P"):
        alone = pkg.sim_step_param_jacobian(params, dt, xt, ut, model=model, want=name, **kw)
        assert torch.equal(alone[name], both[name]), name
    for name in ("p", "x", "u"):
        alone = pkg.sim_step_param_vjp(params, dt, xt, ut, g, model=model, want=name, **kw)
        assert torch.equal(alone[name], both["g" + name]), name
    assert torch.equal(xt, keep_x)
    if per_problem:
        assert torch.equal(params, keep_p)
    assert all(torch.isfinite(v).all() for v in both.values())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("nb,per_problem", [(B, True), (B, False), (1, False)])
def test_dt_zero_is_the_identity(pkg, model, dtype, nb, per_problem):
    x, u = sj.states(model, nb)
    xt, ut = T(x, dtype), T(u, dtype)
    g = T(np.random.default_rng(6).uniform(-1.0, 1.0, x.shape), dtype)
    g[0, 0] = -0.0
    params = T(_columns(model, nb, spread=0.2), dtype) if per_problem else sj.DYN[model]
    res = _all_outputs(pkg, model, 0.0, params, xt, ut, g)
    bits = torch.int64 if dtype == torch.float64 else torch.int32
    assert torch.equal(res["x_new"], xt)
    assert (res["P"] == 0).all() and (res["gp"] == 0).all() and (res["gu"] == 0).all()
    assert torch.equal(res["gx"].view(bits), g.view(bits))
    if per_problem:
        sim = pkg.BatchSimulator(nb, dtype=dtype, device=0, model=model)
        sim.set_state(xt)
        sim.step(params, 0.0, ut)
        assert torch.equal(sim.get_state(), xt)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["single", "double"])
def test_a_nan_parameter_stays_in_its_lane(pkg, model, dtype):
    dt, lane = 0.0025, 37
    x, u = sj.states(model, B)
    g = T(np.random.default_rng(7).uniform(-1.0, 1.0, x.shape), dtype)
    cols = _columns(model, B, spread=0.2)
    clean = _all_outputs(pkg, model, dt, T(cols, dtype), T(x, dtype), T(u, dtype), g)
    bad_cols = cols.copy()
    bad_cols[1, lane] = np.nan   # m_1: it enters every equation of both models
    bad = _all_outputs(pkg, model, dt, T(bad_cols, dtype), T(x, dtype), T(u, dtype), g)
    others = [b for b in range(B) if b != lane]
    for name in clean:
        assert not torch.isfinite(bad[name][..., lane]).all(), name
        assert torch.equal(bad[name][..., others], clean[name][..., others]), name
    sims = []
    for c in (cols, bad_cols):
        s = pkg.BatchSimulator(B, dtype=dtype, device=0, model=model)
        s.set_state(T(x, dtype))
        s.step(T(c, dtype), dt, T(u, dtype))
        sims.append(s.get_state())
    assert not torch.isfinite(sims[1][:, lane]).all() and torch.equal(sims[1][:, others], sims[0][:, others])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["single", "double"])
def test_the_simulator_is_undisturbed(pkg, model, dtype):
    """A BatchSimulator.step after the new calls is a twin's, with shared and with per-problem parameters."""
    x, u = sj.states(model, B)
    cols = T(_columns(model, B, spread=0.2), dtype)
    sim, twin = (pkg.BatchSimulator(B, dtype=dtype, device=0, model=model) for _ in range(2))
    sim.set_state(T(x, dtype))
    twin.set_state(T(x, dtype))
    ut = T(u, dtype)
    for params in (sj.DYN[model], cols):
        for dt in (0.01, 0.0025):
            pkg.sim_step_param_jacobian(params, dt, sim.get_state(), ut, model=model)
            pkg.sim_step_param_vjp(params, dt, sim.get_state(), ut, torch.ones_like(sim.get_state()), model=model)
            sim.step(params, dt, ut)
            twin.step(params, dt, ut)
            assert torch.equal(sim.get_state(), twin.get_state())
    out = pkg.sim_step(cols, 0.003, sim.get_state(), ut, model=model)
    twin.step(cols, 0.003, ut)
    assert torch.equal(out, twin.get_state())
    got = sim.step_differentiable(cols, 0.003, ut)
    assert got is sim.get_state() and torch.equal(got, twin.get_state())


def test_facade_step_param_jacobian_is_lane_zero_of_the_batched_call(pkg):
    pp = pkg.pypendulum()
    shared = (2.0, 0.0, 0.5, -1.0)
    x, u = sj.states("single", B)
    dt = 0.0105
    res = pkg.sim_step_param_jacobian(sj.DYN["single"], dt, T(x), T(u), f_base=shared[:2], f_mass=shared[2:])
    sim = pp.Simulator()
    sim.set_state(pp.SingleCartPoleState(*[float(v) for v in x[:, 0]]))
    P, xn = sim.step_param_jacobian(pp.SingleCartPoleParams(*sj.DYN["single"]), dt, float(u[0]), pp.Vector2(*shared[:2]),
                                    pp.Vector2(*shared[2:]))
    assert np.array_equal(np.array(P).reshape(4, 9), N_(res["P"])[:, :, 0])
    assert np.array_equal(np.array(xn), N_(res["x_new"])[:, 0])
    st = sim.get_state()
    assert [st.b_x, st.th_1, st.b_x_dot, st.th_1_dot] == [float(v) for v in x[:, 0]]   # const: the state is where it was


# ---- autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model,kind", [("single", "per"), ("double", None)])
def test_sim_step_parameter_gradients_are_sim_step_param_vjps(pkg, model, kind, dtype):
    dt = 0.0105
    x, u = sj.states(model, B)
    kw = _kw(_forces(kind, B), dtype)
    g = T(np.random.default_rng(8).uniform(-1.0, 1.0, x.shape), dtype)
    cols = _columns(model, B, spread=0.2)
    xt, ut, pt = T(x, dtype).requires_grad_(), T(u, dtype).requires_grad_(), T(cols, dtype).requires_grad_()
    out = pkg.sim_step(pt, dt, xt, ut, model=model, **kw)
    gx, gu, gp = torch.autograd.grad((out * g).sum(), (xt, ut, pt))
    want = pkg.sim_step_param_vjp(pt.detach(), dt, xt.detach(), ut.detach(), g, model=model, **kw)
    assert torch.equal(gp, want["p"]) and torch.equal(gx, want["x"]) and torch.equal(gu, want["u"])
    # only what needs a gradient is computed, and the simulator's own step takes the tensor too
    pt2 = T(cols, dtype).requires_grad_()
    sim = pkg.BatchSimulator(B, dtype=dtype, device=0, model=model)
    sim.set_state(T(x, dtype))
    out2 = sim.step_differentiable(pt2, dt, T(u, dtype), **kw)
    assert torch.equal(out2, out)
    (gp2,) = torch.autograd.grad((out2 * g).sum(), (pt2,))
    assert torch.equal(gp2, want["p"])
    # a shared set as p.expand(np, B): its gradient is the sum over the batch
    p1 = T(np.array(sj.DYN[model])[:, None], dtype).requires_grad_()
    out3 = pkg.sim_step(p1.expand(-1, B).contiguous(), dt, T(x, dtype), T(u, dtype), model=model, **kw)
    (g1,) = torch.autograd.grad((out3 * g).sum(), (p1,))
    eq = pkg.sim_step_param_vjp(T(_columns(model, B), dtype), dt, T(x, dtype), T(u, dtype), g, model=model, want="p", **kw)["p"]
    eps = float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)
    assert ((g1[:, 0] - eq.sum(dim=1)).abs() <= B * eps * eq.abs().sum(dim=1)).all()


@pytest.mark.parametrize("model,kind", [("single", None), ("single", "per"), ("double", None)])
def test_sim_step_parameter_gradients_match_the_reference(pkg, orc, model, kind):
    """fp64: each entry of P is within 1e-7 max |P| of the reference's, so a gradient's entry is within that times the
    cotangent's 1-norm."""
    dt = 0.0105
    x, u, _, Pr = reference(orc, model, dt, kind)
    g = np.random.default_rng(9).uniform(-1.0, 1.0, x.shape)
    pt = T(_columns(model, B)).requires_grad_()
    out = pkg.sim_step(pt, dt, T(x), T(u), model=model, **_kw(_forces(kind, B), torch.float64))
    (gp,) = torch.autograd.grad((out * T(g)).sum(), (pt,))
    e = np.abs(N_(gp) - np.einsum("rjb,rb->jb", Pr, g)).max(axis=0) / (np.abs(Pr).max(axis=(0, 1)) * np.abs(g).sum(axis=0))
    print("sim_step parameter gradients vs P_ref^T g, %s forces=%s: %.2e (bound 1e-7)" % (model, kind, e.max()))
    assert e.max() <= 1e-7


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["single", "double"])
def test_list_parameters_take_the_parents_path(pkg, model, dtype):
    dt = 0.0105
    x, u = sj.states(model, B)
    g = T(np.random.default_rng(10).uniform(-1.0, 1.0, x.shape), dtype)
    xt, ut = T(x, dtype).requires_grad_(), T(u, dtype).requires_grad_()
    out = pkg.sim_step(sj.DYN[model], dt, xt, ut, model=model)
    gx, gu = torch.autograd.grad((out * g).sum(), (xt, ut))
    twin = pkg.BatchSimulator(B, dtype=dtype, device=0, model=model)
    twin.set_state(T(x, dtype))
    twin.step(sj.DYN[model], dt, T(u, dtype))
    want = pkg.sim_step_vjp(sj.DYN[model], dt, xt.detach(), ut.detach(), g, model=model)
    assert torch.equal(out, twin.get_state()) and torch.equal(gx, want["x"]) and torch.equal(gu, want["u"])


# ---- system identification ---------------------------------------------------------------------------------------------
def test_gauss_newton_identifies_every_plants_parameters(pkg):
    """130 plants, each with its own (m_1, l_1, mu_b) within +-10 % of DYN; 8 recorded one-step transitions per plant
    (dt = 0.0105, states and controls from random_lanes); Gauss-Newton from the nominal set on x+_obs - sim(x, u; p) with the
    three columns of P from the new call and a least-squares solve per lane, all plants in lock-step with per-problem
    parameters.  Every lane recovers its parameters to 1e-9 relative within 8 iterations.  (The CPU twin of this loop --
    the oracle and central differences, 16 plants -- converges in 4 - 5 iterations to 3e-14; the Jacobians' condition
    numbers are 9 - 33.)"""
    dt, n_obs, idx = 0.0105, 8, [1, 2, 4]
    rng = np.random.default_rng(17)
    true = _columns("single", B)
    true[idx] *= rng.uniform(0.9, 1.1, (3, B))
    obs = []
    for _ in range(n_obs):
        x, u = sj.random_lanes(rng, "single", B)
        sim = pkg.BatchSimulator(B, dtype=torch.float64, device=0)
        sim.set_state(T(x))
        sim.step(T(true), dt, T(u))
        obs.append((T(x), T(u), sim.get_state().clone()))
    est = T(_columns("single", B))
    two_pi = 2 * np.pi
    err = None
    for it in range(8):
        rows_j, rows_r = [], []
        for x, u, xo in obs:
            res = pkg.sim_step_param_jacobian(est, dt, x, u)
            r = xo - res["x_new"]
            r[1] = r[1] - two_pi * torch.round(r[1] / two_pi)   # the pole angle's difference, wrapped
            rows_r.append(r)
            rows_j.append(res["P"][:, idx, :])
        J = torch.cat(rows_j, dim=0).permute(2, 0, 1).cpu()       # [B, 4 n_obs, 3]
        r = torch.cat(rows_r, dim=0).permute(1, 0).unsqueeze(2).cpu()
        step = torch.linalg.lstsq(J, r).solution[:, :, 0]         # [B, 3]
        est[idx] = est[idx] + step.t().to(DEV)
        err = np.abs(N_(est)[idx] / true[idx] - 1.0).max(axis=0)
        print("identification iteration %d: worst relative parameter error %.2e, lanes within 1e-9: %d of %d"
              % (it + 1, err.max(), int((err <= 1e-9).sum()), B))
        if err.max() <= 1e-9:
            break
    assert err.max() <= 1e-9


# ---- the closed loop with the plants' own parameters ---------------------------------------------------------------------
def test_closed_loop_with_plant_dyn_equal_to_dyn_is_the_loop_without_it(pkg):
    dyn = sj.DYN["single"]
    x0 = T(random_states(np.random.default_rng(13), B))
    finals = {}
    for name, kw in (("none", {}), ("list", dict(plant_dyn=list(dyn))), ("tensor", dict(plant_dyn=T(_columns("single", B)))),
                     ("both", dict(plant_dyn=T(_columns("single", B))))):
        loop = pkg.ClosedLoop(pkg.default_params(), B, dtype=torch.float64, device=0)
        loop.set_state(x0)
        d = T(_columns("single", B)) if name == "both" else dyn
        for _ in range(3):
            loop.tick(d, 0.0, dt=0.01, **kw)
        finals[name] = (loop.state().clone(), loop.controls()[0].clone())
        loop.close()
    with pytest.raises(TypeError):
        loop = pkg.ClosedLoop(pkg.default_params(), B, dtype=torch.float64, device=0)
        try:
            loop.tick(T(_columns("single", B)), 0.0, dt=0.01)
        finally:
            loop.close()
    assert torch.equal(finals["list"][0], finals["none"][0]) and torch.equal(finals["list"][1], finals["none"][1])
    ex = (finals["tensor"][0] - finals["none"][0]).abs().max().item()
    print("three ticks, plant_dyn a tensor equal to dyn: |x - x without it| %.2e (bound 1e-12)" % ex)
    assert ex <= 1e-12
    assert not torch.equal(finals["none"][0], x0) and torch.isfinite(finals["both"][0]).all()
