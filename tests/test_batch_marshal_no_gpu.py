"""The marshalling helpers of the torch API (batch.py) without a GPU: the `want` normaliser, the output allocator on a
ctypes struct, the per-lane Cholesky solve of sim_identify, and that the public plant functions refuse a bad `want`
before they look at a tensor.  Torch on CPU tensors only: no device, no handle."""
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

NX, NP, T, B = 4, 9, 3, 5
GN_TABLE = {"cost": ("cost", (B,)), "g": ("g", (NP, B)), "H": ("H", (NP, NP, B)), "S_final": ("S_final", (NX, NP, B)),
            "x_final": ("x_final", (NX, B))}


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("cart-pole-mpc_amd.batch")


def test_want_becomes_a_tuple_in_the_order_given(batch):
    norm = batch._want_tuple
    names = ("K", "k_sp", "k_up")
    assert norm("k_sp", names) == ("k_sp",)
    assert norm(["k_up", "K"], names) == ("k_up", "K")
    assert norm(("K", "k_sp", "k_up"), names) == names
    assert norm(iter(["k_sp", "K"]), names) == ("k_sp", "K")


def test_want_refuses_unknown_names_and_nothing(batch):
    norm = batch._want_tuple
    names = ("K", "k_sp", "k_up")
    for bad in ("k", ("K", "nope"), ["k_up", ""], "Kk_sp"):
        with pytest.raises(ValueError) as e:
            norm(bad, names)
        assert str(e.value) == "want must name at least one of 'K', 'k_sp', 'k_up'"
    for empty in ((), []):
        with pytest.raises(ValueError) as e:
            norm(empty, names)
        assert str(e.value) == "want must name at least one of 'K', 'k_sp', 'k_up'"
        assert norm(empty, names, allow_empty=True) == ()
    with pytest.raises(ValueError):                       # allowed to be empty, still not allowed to be wrong
        norm(("nope",), names, allow_empty=True)
    with pytest.raises(ValueError) as e:
        norm((), ("terminal", "u"), allow_empty=False, message="some of these (or nothing, with want_du)")
    assert str(e.value) == "some of these (or nothing, with want_du)"


@pytest.mark.parametrize("want", [("cost",), ("g",), ("H",), ("S_final",), ("x_final",), ("x_final", "g"),
                                  ("cost", "g", "H", "S_final", "x_final")])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_allocator_fills_exactly_the_wanted_fields(batch, want, dtype):
    a = batch.capi.SimRolloutGn(struct_size=64)
    res = batch._alloc_outputs(a, want, GN_TABLE, dtype, "cpu")
    assert list(res) == list(want)
    for name, (field, shape) in GN_TABLE.items():
        if name in want:
            t = res[name]
            assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cpu" and t.is_contiguous()
            assert getattr(a, field) == t.data_ptr() != 0
        else:
            assert getattr(a, field) is None              # a null void pointer
    assert a.struct_size == 64 and a.x0 is None and a.u is None and a.x_obs is None and a.tick_w is None


def test_allocator_follows_the_field_names_and_needs_no_struct(batch):
    a = batch.capi.SimRolloutVjp()
    table = {"x": ("g_x0", (NX, B)), "u": ("g_u", (T, B)), "p": ("g_p", (NP, B))}
    res = batch._alloc_outputs(a, ("p", "x"), table, torch.float64, "cpu")
    assert a.g_p == res["p"].data_ptr() and a.g_x0 == res["x"].data_ptr() and a.g_u is None
    assert tuple(res["p"].shape) == (NP, B) and tuple(res["x"].shape) == (NX, B)
    res = batch._alloc_outputs(None, ("u",), table, torch.float32, "cpu")
    assert list(res) == ["u"] and tuple(res["u"].shape) == (T, B) and res["u"].dtype == torch.float32


@pytest.mark.parametrize("k", [3, 6])
def test_cholesky_solve_lanes_against_numpy(batch, k):
    """B = 5 lanes of SPD systems A A^T + I (smallest eigenvalue >= 1, so well conditioned at these sizes: the condition
    number is printed) in float64 against numpy.linalg.solve per lane to 1e-10 relative; then one lane gets a negative
    diagonal entry: it reports pd = False and no other lane's solution moves by a bit."""
    rng = np.random.default_rng(100 + k)
    A = rng.standard_normal((B, k, k))
    M = A @ A.transpose(0, 2, 1) + np.eye(k)
    g = rng.standard_normal((B, k))
    ref = np.stack([np.linalg.solve(M[b], g[b]) for b in range(B)])

    def solve(mat):
        Hs = [[torch.tensor(mat[:, j, i].copy()) for i in range(k)] for j in range(k)]
        x, pd = batch._cholesky_solve_lanes(Hs, [torch.tensor(g[:, j].copy()) for j in range(k)])
        return torch.stack(x, dim=1).numpy(), pd.numpy()

    x, pd = solve(M)
    assert pd.dtype == np.bool_ and pd.all()
    rel = np.linalg.norm(x - ref, axis=1) / np.linalg.norm(ref, axis=1)
    print("k = %d: condition numbers %s, relative error per lane %s" % (k, np.linalg.cond(M), rel))
    assert (rel <= 1e-10).all(), rel
    bad = M.copy()
    bad[2, 1, 1] = -1.0
    x_bad, pd_bad = solve(bad)
    assert pd_bad.tolist() == [True, True, False, True, True]
    others = [0, 1, 3, 4]
    assert np.array_equal(x_bad[others], x[others])
    # only the lower triangle is read
    upper = M.copy()
    upper[:, np.triu_indices(k, 1)[0], np.triu_indices(k, 1)[1]] = np.nan
    x_up, pd_up = solve(upper)
    assert pd_up.all() and np.array_equal(x_up, x)


def test_autograd_input_names_are_the_forwards_own_arguments(batch):
    """backward finds the differentiable inputs, and builds its return tuple, from a tuple of names kept next to each
    forward: that tuple is the forward's signature."""
    import inspect
    for cls, names in ((batch._PlanVjpFunction, batch._PlanVjpFunction.INPUTS),
                       (batch._PlanWeightVjpFunction, batch._PlanWeightVjpFunction.INPUTS),
                       (batch._SimStepFunction, batch._PLANT_INPUTS), (batch._SimRolloutFunction, batch._PLANT_INPUTS)):
        assert tuple(inspect.signature(cls.forward).parameters)[1:] == names, cls.__name__
    assert set(batch._PLANT_GRADS) <= set(batch._PLANT_INPUTS)
    for cls in (batch._PlanVjpFunction, batch._PlanWeightVjpFunction):
        assert {"x0", "set_point"} <= set(cls.INPUTS)
    assert "terminal_weights" in batch._PlanWeightVjpFunction.INPUTS


def test_public_plant_functions_refuse_a_bad_want_before_any_tensor(batch):
    """CPU tensors (a GPU tensor is what every one of these requires, with TypeError): a bad `want` is a ValueError, so it
    was looked at first -- and before the library is."""
    b = batch
    dyn = [1.0, 0.1, 0.25, 9.81, 0.03, 0.1, 0.13, 0.8, 100.0]
    x, u, us = torch.zeros((NX, B)), torch.zeros(B), torch.zeros((T, B))
    xs = torch.zeros((T, NX, B))
    calls = [
        lambda w: b.sim_step_jacobian(dyn, 0.01, x, u, want=w),
        lambda w: b.sim_step_vjp(dyn, 0.01, x, u, x, want=w),
        lambda w: b.sim_step_param_jacobian(dyn, 0.01, x, u, want=w),
        lambda w: b.sim_step_param_vjp(dyn, 0.01, x, u, x, want=w),
        lambda w: b.sim_rollout_states(dyn, 0.01, x, us, want=w),
        lambda w: b.sim_rollout_vjp(dyn, 0.01, x, us, xs, gbar=xs, want=w),
        lambda w: b.sim_rollout_gauss_newton(dyn, 0.01, x, us, xs, want=w),
    ]
    for call in calls:
        for w in ((), [], "nope", ("x_new", "nope"), ("x", "y")):
            with pytest.raises(ValueError, match="want must name at least one of"):
                call(w)
