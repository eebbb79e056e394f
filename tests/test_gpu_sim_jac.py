"""The plant step with its first derivatives on the GPU (cpmpc_sim_step_jac_batch; sim_step_jacobian, sim_step_vjp, sim_step,
BatchSimulator.step_differentiable, pypendulum.Simulator.step_jacobian) against the numpy reference of
tests/helpers/sim_jac_ref.py, which tests/test_sim_jac_ref.py pins to the CPU oracle's simulator.

Shapes: B = 130 -- two full waves and a 2-lane tail -- and B = 1; dt 0.001 (one sub-step), 0.0025 (three, a short last one),
0.0105 (eleven, a short last one), 0.02, and dt = 0; both models.  States as test_simulator_matches_oracle's, with a block of
lanes that wrap inside the step and, for the 4-state model, a block beyond the bumpers (sim_jac_ref.states).
fp64: |A - A_ref| <= n_sub 1e-13 max(1, max |A_ref|) and |Bu - Bu_ref| <= n_sub 1e-14 max(1, max |Bu_ref|) -- the suite's one-step
tolerances for A and Bm (test_rk4_matches_oracle) accumulated to first order over n_sub factors; x_new at the simulator's 1e-12.
fp32: the yardstick is n_sub chained calls of the float rk4_batch with the wrap and the products in float32 torch; per lane
the distance from the fp64 reference relative to max |A_ref|; the kernel's median and 99th percentile at most 4 x those.
Every test prints its figures before it asserts; DESIGN.md section 5e is where they are recorded."""
import numpy as np
import pytest

from conftest import random_states
from helpers import sim_jac_ref as sj

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
B = 130
DTS = (0.001, 0.0025, 0.0105, 0.02)
SHARED = (2.0, 0.0, 0.5, -1.0)
# (model, dt, forces): every dt for both models without forces, per-problem forces in one case, shared ones in another
CASES = [(m, dt, None) for m in ("single", "double") for dt in DTS] + [("single", 0.0105, "per"), ("single", 0.0025, "shared")]


@pytest.fixture(scope="module", autouse=True)
def _gpu(pkg):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the product has no CPU fallback")
    pkg.capi.load()
    assert pkg.capi.load().cpmpc_device_count() >= 1
    assert callable(pkg.sim_step)   # imports the batch module


def T(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def _forces(kind, nb):
    """-> (numpy forces for the reference, keyword arguments of the package's calls for `dtype`)"""
    if kind == "per":
        f = np.random.default_rng(21).uniform(-3.0, 3.0, (4, nb))
        return f, lambda dtype: dict(fext=T(f, dtype))
    if kind == "shared":
        return np.array(SHARED), lambda dtype: dict(f_base=SHARED[:2], f_mass=SHARED[2:])
    return None, lambda dtype: {}


_REF = {}


def reference(orc, model, dt, kind, nb=B):
    """(x, u, x_new, A, Bu) of the fp64 numpy reference, computed once per case and left unchanged."""
    key = (model, dt, kind, nb)
    if key not in _REF:
        x, u = sj.states(model, nb)
        f, _ = _forces(kind, nb)
        _REF[key] = (x, u) + sj.step_ref_batch(orc, model, sj.DYN[model], dt, x, u, f)
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _all_outputs(pkg, model, dt, x, u, g, **kw):
    """One call with every output of cpmpc_sim_jac asked for."""
    return pkg.batch._sim_jac_call(sj.DYN[model], dt, x, u, kw.get("fext"), kw.get("f_base", (0.0, 0.0)),
                                   kw.get("f_mass", (0.0, 0.0)), model, g, ("x_new", "A", "Bu", "gx", "gu"))


# ---- accuracy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,dt,kind", CASES)
def test_fp64_matches_reference(pkg, orc, model, dt, kind):
    x, u, xr, Ar, Br = reference(orc, model, dt, kind)
    n_sub = len(sj.sub_steps(dt))
    _, kw = _forces(kind, B)
    res = pkg.sim_step_jacobian(sj.DYN[model], dt, T(x), T(u), model=model, **kw(torch.float64))
    ea = np.abs(N_(res["A"]) - Ar).max()
    eb = np.abs(N_(res["Bu"]) - Br).max()
    ex = np.abs(N_(res["x_new"]) - xr).max()
    ba = n_sub * 1e-13 * max(1.0, np.abs(Ar).max())
    bb = n_sub * 1e-14 * max(1.0, np.abs(Br).max())
    print("fp64 %s dt=%g forces=%s n_sub=%d: |A-ref| %.2e (bound %.2e)  |Bu-ref| %.2e (bound %.2e)  |x-ref| %.2e (bound 1e-12)"
          % (model, dt, kind, n_sub, ea, ba, eb, bb, ex))
    wrapped = (np.abs(xr[1:sj.NX[model] // 2] - x[1:sj.NX[model] // 2]) > 3.0).any(axis=0)
    in_bumper = np.abs(x[0]) > sj.BUMPER_X
    assert wrapped[:2].all(), "lanes 0 and 1 did not wrap inside the step"
    if model == "single":
        assert in_bumper.sum() >= B // 4
    assert ea <= ba and eb <= bb and ex <= 1e-12


@pytest.mark.parametrize("model", ["single", "double"])
def test_fp64_single_problem(pkg, orc, model):
    x, u, xr, Ar, Br = reference(orc, model, 0.0105, None, nb=1)
    res = pkg.sim_step_jacobian(sj.DYN[model], 0.0105, T(x), T(u), model=model)
    assert np.abs(N_(res["A"]) - Ar).max() <= 11 * 1e-13 * max(1.0, np.abs(Ar).max())
    assert np.abs(N_(res["Bu"]) - Br).max() <= 11 * 1e-14 * max(1.0, np.abs(Br).max())
    assert np.abs(N_(res["x_new"]) - xr).max() <= 1e-12
    g = T(np.random.default_rng(2).uniform(-1, 1, (sj.NX[model], 1)))
    v = pkg.sim_step_vjp(sj.DYN[model], 0.0105, T(x), T(u), g, model=model)
    assert v["x"].shape == (sj.NX[model], 1) and v["u"].shape == (1,) and torch.isfinite(v["x"]).all()


def _wrap32(x, nq):
    """mod_pi of the pole angles in float32 torch"""
    two_pi = torch.tensor(2 * np.pi, dtype=torch.float32, device=x.device)
    for t in range(1, nq):
        a = x[t] - torch.trunc(x[t] / two_pi) * two_pi
        a = torch.where(a < 0, a + two_pi, a)
        a = torch.where(a > np.float32(np.pi), a - two_pi, a)
        x[t] = a
    return x


def _chained_rk4_f32(pkg, model, dt, x, u, fext):
    """The parent's own float code: one rk4_batch call per sub-step, A <- A_i A and Bu <- A_i Bu + B_i in float32 torch."""
    nx = sj.NX[model]
    xs = T(x, torch.float32)
    us = T(u, torch.float32)
    A = torch.eye(nx, dtype=torch.float32, device=DEV).reshape(nx, nx, 1).repeat(1, 1, x.shape[1])
    Bu = torch.zeros((nx, x.shape[1]), dtype=torch.float32, device=DEV)
    for h in sj.sub_steps(dt):
        xs, Ai, Bi = pkg.rk4_batch(sj.DYN[model], xs, us, h, fext=fext, model=model)
        xs = _wrap32(xs, nx // 2)
        A = torch.einsum("rmb,mcb->rcb", Ai, A).contiguous()
        Bu = torch.einsum("rmb,mb->rb", Ai, Bu) + Bi
    return N_(A).astype(np.float64), N_(Bu).astype(np.float64)


def _lane_err(got, ref):
    ax = tuple(range(ref.ndim - 1))
    return np.abs(got - ref).max(axis=ax) / np.abs(ref).max(axis=ax)


@pytest.mark.parametrize("model,dt,kind", [c for c in CASES if c[2] != "per"])
def test_fp32_within_four_times_the_chained_float_rk4(pkg, orc, model, dt, kind):
    x, u, _, Ar, Br = reference(orc, model, dt, kind)
    _, kw = _forces(kind, B)
    res = pkg.sim_step_jacobian(sj.DYN[model], dt, T(x, torch.float32), T(u, torch.float32), model=model, **kw(torch.float32))
    # the reference saw the float64 states; the float32 ones differ by rounding for both candidates alike
    Ae, Be = _chained_rk4_f32(pkg, model, dt, x, u, SHARED if kind == "shared" else None)
    fig = {}
    for name, got, emu, ref in (("A", N_(res["A"]).astype(np.float64), Ae, Ar), ("Bu", N_(res["Bu"]).astype(np.float64), Be, Br)):
        k, e = _lane_err(got, ref), _lane_err(emu, ref)
        fig[name] = (np.median(k), np.percentile(k, 99), np.median(e), np.percentile(e, 99))
        print("fp32 %s dt=%g forces=%s %s: kernel median %.2e p99 %.2e | chained float rk4_batch median %.2e p99 %.2e"
              % ((model, dt, kind, name) + fig[name]))
    for name, (km, kp, em, ep) in fig.items():
        assert km <= 4 * em and kp <= 4 * ep, (name, km, kp, em, ep)


# ---- the VJP against the same call's Jacobian ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["single", "double"])
def test_vjp_is_the_jacobians_transpose(pkg, orc, model, dtype):
    nx = sj.NX[model]
    eps = float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)
    dt = 0.0105
    x, u = sj.states(model, B)
    xt, ut = T(x, dtype), T(u, dtype)
    jac = pkg.sim_step_jacobian(sj.DYN[model], dt, xt, ut, model=model, want=("A", "Bu"))
    A, Bu = N_(jac["A"]).astype(np.float64), N_(jac["Bu"]).astype(np.float64)
    cots = [np.random.default_rng(31).uniform(-1.0, 1.0, (nx, B))]
    for r in range(nx):
        e = np.zeros((nx, B))
        e[r] = 1.0
        cots.append(e)
    worst_x = worst_u = 0.0
    for g in cots:
        gt = T(g, dtype)
        g64 = N_(gt).astype(np.float64)
        v = pkg.sim_step_vjp(sj.DYN[model], dt, xt, ut, gt, model=model)
        gx, gu = N_(v["x"]).astype(np.float64), N_(v["u"]).astype(np.float64)
        bx = 4 * nx * eps * np.einsum("rcb,rb->cb", np.abs(A), np.abs(g64))
        bu = 4 * nx * eps * np.einsum("rb,rb->b", np.abs(Bu), np.abs(g64))
        dx = np.abs(gx - np.einsum("rcb,rb->cb", A, g64))
        du = np.abs(gu - np.einsum("rb,rb->b", Bu, g64))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst_x = max(worst_x, np.nanmax(np.where(bx > 0, dx / bx, np.where(dx > 0, np.inf, 0.0))))
            worst_u = max(worst_u, np.nanmax(np.where(bu > 0, du / bu, np.where(du > 0, np.inf, 0.0))))
        assert (dx <= bx).all() and (du <= bu).all()
    print("vjp %s %s: worst |gx - A^T g| / bound %.3f, worst |gu - Bu.g| / bound %.3f" % (model, dtype, worst_x, worst_u))


# ---- bitwise properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model,kind", [("single", "per"), ("double", None)])
def test_outputs_do_not_depend_on_each_other_and_the_state_is_read_only(pkg, model, kind, dtype):
    dt = 0.0025
    x, u = sj.states(model, B)
    _, kw = _forces(kind, B)
    kw = kw(dtype)
    xt, ut = T(x, dtype), T(u, dtype)
    keep = xt.clone()
    g = T(np.random.default_rng(5).uniform(-1.0, 1.0, x.shape), dtype)
    both = _all_outputs(pkg, model, dt, xt, ut, g, **kw)
    again = _all_outputs(pkg, model, dt, xt, ut, g, **kw)
    for name in both:
        assert torch.equal(both[name], again[name]), name
    for name in ("x_new", "A", "Bu"):
        alone = pkg.sim_step_jacobian(sj.DYN[model], dt, xt, ut, model=model, want=name, **kw)
        assert torch.equal(alone[name], both[name]), name
    for name in ("x", "u"):
        alone = pkg.sim_step_vjp(sj.DYN[model], dt, xt, ut, g, model=model, want=name, **kw)
        assert torch.equal(alone[name], both["g" + name]), name
    assert torch.equal(xt, keep)
    assert all(torch.isfinite(v).all() for v in both.values())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["single", "double"])
@pytest.mark.parametrize("nb", [B, 1])
def test_dt_zero_is_the_identity(pkg, model, dtype, nb):
    nx = sj.NX[model]
    x, u = sj.states(model, nb)
    xt, ut = T(x, dtype), T(u, dtype)
    g = T(np.random.default_rng(6).uniform(-1.0, 1.0, x.shape), dtype)
    g[0, 0] = -0.0
    res = _all_outputs(pkg, model, 0.0, xt, ut, g)
    eye = torch.eye(nx, dtype=dtype, device=DEV).reshape(nx, nx, 1).repeat(1, 1, nb)
    assert torch.equal(res["x_new"], xt)
    assert torch.equal(res["A"], eye)
    assert (res["Bu"] == 0).all() and (res["gu"] == 0).all()
    assert torch.equal(res["gx"].view(torch.int64 if dtype == torch.float64 else torch.int32),
                       g.view(torch.int64 if dtype == torch.float64 else torch.int32))


@pytest.mark.parametrize("model", ["single", "double"])
def test_a_nan_lane_stays_in_its_lane(pkg, model):
    dt, lane = 0.0025, 37
    x, u = sj.states(model, B)
    g = T(np.random.default_rng(7).uniform(-1.0, 1.0, x.shape))
    clean = _all_outputs(pkg, model, dt, T(x), T(u), g)
    xb = x.copy()
    xb[1, lane] = np.nan   # a pole angle: it enters the dynamics of both models
    bad = _all_outputs(pkg, model, dt, T(xb), T(u), g)
    others = [b for b in range(B) if b != lane]
    for name in clean:
        assert not torch.isfinite(bad[name][..., lane]).all(), name
        assert torch.equal(bad[name][..., others], clean[name][..., others]), name


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model,kind", [("single", "per"), ("single", "shared"), ("double", None)])
def test_sim_step_forward_is_the_simulators_and_the_simulator_is_undisturbed(pkg, model, kind, dtype):
    x, u = sj.states(model, B)
    _, kw = _forces(kind, B)
    kw = kw(dtype)
    sim, twin = (pkg.BatchSimulator(B, dtype=dtype, device=0, model=model) for _ in range(2))
    sim.set_state(T(x, dtype))
    twin.set_state(T(x, dtype))
    for dt in (0.01, 0.0025):
        out = pkg.sim_step(sj.DYN[model], dt, sim.get_state(), T(u, dtype), model=model, **kw)
        twin.step(sj.DYN[model], dt, T(u, dtype), **kw)
        assert torch.equal(out, twin.get_state())
        before = sim.get_state().clone()
        got = sim.step_differentiable(sj.DYN[model], dt, T(u, dtype), **kw)
        assert got is sim.get_state() and torch.equal(got, twin.get_state())
        # Jacobian calls in between leave the simulator alone: its next step is bitwise the twin's
        pkg.sim_step_jacobian(sj.DYN[model], dt, sim.get_state(), T(u, dtype), model=model, **kw)
        pkg.sim_step_vjp(sj.DYN[model], dt, sim.get_state(), T(u, dtype), torch.ones_like(before), model=model, **kw)
    sim.step(sj.DYN[model], 0.003, T(u, dtype), **kw)
    twin.step(sj.DYN[model], 0.003, T(u, dtype), **kw)
    assert torch.equal(sim.get_state(), twin.get_state())


# ---- autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model,kind", [("single", "per"), ("double", None)])
def test_sim_step_gradients_are_sim_step_vjps(pkg, model, kind, dtype):
    dt = 0.0105
    x, u = sj.states(model, B)
    _, kw = _forces(kind, B)
    kw = kw(dtype)
    g = T(np.random.default_rng(8).uniform(-1.0, 1.0, x.shape), dtype)
    xt, ut = T(x, dtype).requires_grad_(), T(u, dtype).requires_grad_()
    out = pkg.sim_step(sj.DYN[model], dt, xt, ut, model=model, **kw)
    gx, gu = torch.autograd.grad((out * g).sum(), (xt, ut))
    want = pkg.sim_step_vjp(sj.DYN[model], dt, xt.detach(), ut.detach(), g, model=model, **kw)
    assert torch.equal(gx, want["x"]) and torch.equal(gu, want["u"])
    # only what needs a gradient is computed
    xt2 = T(x, dtype).requires_grad_()
    out = pkg.sim_step(sj.DYN[model], dt, xt2, T(u, dtype), model=model, **kw)
    (gx2,) = torch.autograd.grad((out * g).sum(), (xt2,))
    assert torch.equal(gx2, want["x"])


@pytest.mark.parametrize("model", ["single", "double"])
def test_sim_step_gradients_match_central_differences_of_the_simulator(pkg, model):
    """fp64, state step 1e-6 and control step 1e-4 as on the CPU (tests/test_sim_jac_ref.py), on the lanes that do not cross
    the wrap under the perturbation.  Each entry of A (Bu) is within 1e-7 max |A| (max |Bu|) of its central difference -- the
    CPU-measured bound -- so a gradient's entry is within that times the cotangent's 1-norm."""
    dt, hx, hu = 0.0105, 1e-6, 1e-4
    nx, nq = sj.NX[model], sj.NX[model] // 2
    x, u = sj.states(model, B)
    g = np.random.default_rng(9).uniform(-1.0, 1.0, x.shape)
    xt, ut = T(x).requires_grad_(), T(u).requires_grad_()
    out = pkg.sim_step(sj.DYN[model], dt, xt, ut, model=model)
    gx, gu = (N_(t) for t in torch.autograd.grad((out * T(g)).sum(), (xt, ut)))

    def plant(xp, up):
        sim = pkg.BatchSimulator(B, dtype=torch.float64, device=0, model=model)
        sim.set_state(T(xp))
        sim.step(sj.DYN[model], dt, T(up))
        return N_(sim.get_state())

    A = np.zeros((nx, nx, B))
    ok = np.ones(B, dtype=bool)
    for c in range(nx):
        e = np.zeros((nx, 1))
        e[c] = hx
        d = plant(x + e, u) - plant(x - e, u)
        ok &= (np.abs(d[1:nq]) < 1.0).all(axis=0)
        A[:, c] = d / (2 * hx)
    d = plant(x, u + hu) - plant(x, u - hu)
    ok &= (np.abs(d[1:nq]) < 1.0).all(axis=0)
    Bu = d / (2 * hu)
    assert ok.sum() >= B // 2
    l1 = np.abs(g).sum(axis=0)
    ex = np.abs(gx - np.einsum("rcb,rb->cb", A, g)).max(axis=0) / (np.abs(A).max(axis=(0, 1)) * l1)
    eu = np.abs(gu - np.einsum("rb,rb->b", Bu, g)) / (np.abs(Bu).max(axis=0) * l1)
    print("sim_step gradients vs central differences of BatchSimulator.step, %s, %d lanes: state %.2e  control %.2e (bound 1e-7)"
          % (model, ok.sum(), ex[ok].max(), eu[ok].max()))
    assert ex[ok].max() <= 1e-7 and eu[ok].max() <= 1e-7


def test_three_tick_closed_loop_backward_is_the_hand_written_composition(pkg):
    """Three ticks of u_t = mpc(x_t; w), x_{t+1} = plant(x_t, u_t) at B = 130, fp64, 4-state model, loss = sum x_3^2, with
    the terminal weights requiring grad: backward runs, the gradients for x_0 and the terminal weights are finite on every
    lane whose QPs are positive definite, and they are bitwise the same plan_vjp / plan_weight_vjp / sim_step_vjp calls
    composed by hand in reverse order.

    This covers the PLUMBING only.  It is not a derivative of the nonlinear solver: the controller's part is the derivative
    of the last Gauss-Newton QP of each step (BatchOptimization.step_differentiable), and the influence of one tick's
    solution on the next through the warm start is not differentiated."""
    dyn, dt = sj.DYN["single"], 0.01
    x0_np = random_states(np.random.default_rng(12), B)
    tw_np = np.tile(np.array([40.0, -1.0, 3.0, 2.0])[:, None], (1, B))
    opt = pkg.BatchOptimization(pkg.default_params(), max_batch=B, dtype=torch.float64, device=0)
    tw = T(tw_np).requires_grad_()
    x0 = T(x0_np).requires_grad_()
    xs, us, zs, u_prevs = [x0], [], [], []
    for t in range(3):
        if opt.previous_solution_batch() >= B:
            u_prevs.append(opt.get_solution(B)[opt.nx * opt.S].clone())
        else:
            u_prevs.append(torch.zeros((B,), dtype=torch.float64, device=DEV))
        u_all, _ = opt.step_differentiable(xs[t], dyn, 0.0, n_rows=1, terminal_weights=tw, weight_grad=True)
        zs.append(opt.get_solution(B))
        us.append(u_all[0])
        xs.append(pkg.sim_step(dyn, dt, xs[t], us[t]))
    loss = (xs[3] ** 2).sum()
    loss.backward()
    # by hand, in reverse
    twd = tw.detach()
    g_next = 2.0 * xs[3].detach()
    g_tw, ok_all = None, torch.ones((B,), dtype=torch.bool, device=DEV)
    for t in (2, 1, 0):
        xt, ut = xs[t].detach(), us[t].detach().contiguous()
        sv = pkg.sim_step_vjp(dyn, dt, xt, ut, g_next)
        gbar = sv["u"].reshape(1, B).contiguous()
        pv = opt.plan_vjp(dyn, gbar, z=zs[t], terminal_weights=twd, want=("x0",), want_ok=True)
        pw = opt.plan_weight_vjp(xt, dyn, gbar, set_point=0.0, u_prev=u_prevs[t], z=zs[t], terminal_weights=twd,
                                 want=("terminal",), want_ok=True)
        gx_plan = torch.where(pv["ok"] != 0, pv["x0"], torch.zeros_like(pv["x0"]))
        gt = torch.where(pw["ok"] != 0, pw["terminal"], torch.zeros_like(pw["terminal"]))
        ok_all &= (pv["ok"] != 0) & (pw["ok"] != 0)
        g_tw = gt if g_tw is None else g_tw + gt
        g_next = sv["x"] + gx_plan
    n_ok = int(ok_all.sum())
    print("three-tick loop: %d of %d lanes with every QP positive definite; max |dL/dx0| %.3e, max |dL/dw| %.3e"
          % (n_ok, B, x0.grad.abs().max().item(), tw.grad.abs().max().item()))
    assert n_ok >= B // 2
    assert torch.isfinite(x0.grad[:, ok_all]).all() and torch.isfinite(tw.grad[:, ok_all]).all()
    assert x0.grad.abs().max() > 0 and tw.grad.abs().max() > 0
    assert torch.equal(x0.grad, g_next)
    assert torch.equal(tw.grad, g_tw)
    opt.close()


# ---- the facade ------------------------------------------------------------------------------------------------------
def test_facade_step_jacobian_is_lane_zero_of_the_batched_call(pkg):
    pp = pkg.pypendulum()
    x, u = sj.states("single", B)
    dt = 0.0105
    res = pkg.sim_step_jacobian(sj.DYN["single"], dt, T(x), T(u), f_base=SHARED[:2], f_mass=SHARED[2:], want=("A", "Bu"))
    sim = pp.Simulator()
    sim.set_state(pp.SingleCartPoleState(*[float(v) for v in x[:, 0]]))
    A, Bv = sim.step_jacobian(pp.SingleCartPoleParams(*sj.DYN["single"]), dt, float(u[0]), pp.Vector2(*SHARED[:2]),
                              pp.Vector2(*SHARED[2:]))
    assert np.array_equal(np.array(A).reshape(4, 4), N_(res["A"])[:, :, 0])
    assert np.array_equal(np.array(Bv), N_(res["Bu"])[:, 0])
    st = sim.get_state()
    assert [st.b_x, st.th_1, st.b_x_dot, st.th_1_dot] == [float(v) for v in x[:, 0]]   # const: the state is where it was
