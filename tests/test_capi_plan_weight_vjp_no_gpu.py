"""The weight-gradient entry points of the C-ABI without a GPU: exported, prototyped in capi.py with the documented
signatures, the argument checks answer CPMPC_ERR_INVALID_ARG before any device is needed, and with well-formed arguments
and no device the answer is CPMPC_ERR_NO_DEVICE: the product has no CPU compute path."""
import ctypes as C

import pytest

NAMES = ("cpmpc_plan_weight_vjp_batch", "cpmpc_plan_weight_vjp_batch_host")


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.capi.load()


def _inputs(capi, buf):
    inp = capi.WeightVjpInputs(struct_size=C.sizeof(capi.WeightVjpInputs))
    inp.lin.struct_size = C.sizeof(capi.GainInputs)
    inp.x0 = C.cast(buf, C.c_void_p)
    return inp


def test_symbols_exported_and_prototyped(lib, pkg):
    capi = pkg.capi
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.cpmpc_plan_weight_vjp_batch.argtypes) == 11
    assert len(lib.cpmpc_plan_weight_vjp_batch_host.argtypes) == 10
    fields = [f[0] for f in capi.WeightVjpInputs._fields_]
    assert fields == ["struct_size", "lin", "x0", "set_point_shared", "set_point", "u_prev"]
    assert C.sizeof(capi.WeightVjpInputs) == 8 + C.sizeof(capi.GainInputs) + 4 * 8


def test_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf = (C.c_double * 64)()
    g = C.cast(buf, C.c_void_p)
    inp = _inputs(capi, buf)
    call, host = lib.cpmpc_plan_weight_vjp_batch, lib.cpmpc_plan_weight_vjp_batch_host
    bad = capi.ERR_INVALID_ARG
    assert call(None, 1, None, 1, g, g, g, g, g, None, None) == bad                    # null in
    assert host(None, 1, None, 1, buf, buf, buf, buf, buf, None) == bad
    wrong = _inputs(capi, buf)
    wrong.struct_size = C.sizeof(capi.WeightVjpInputs) - 8                              # wrong struct_size
    assert call(None, 1, C.byref(wrong), 1, g, g, g, g, g, None, None) == bad
    assert b"struct_size" in lib.cpmpc_last_error()
    assert host(None, 1, C.byref(wrong), 1, buf, buf, buf, buf, buf, None) == bad
    assert call(None, 1, C.byref(inp), 1, g, None, None, None, None, None, None) == bad   # no output
    assert b"output" in lib.cpmpc_last_error()
    assert host(None, 1, C.byref(inp), 1, buf, None, None, None, None, None) == bad
    for n_rows in (0, -3):                                                             # n_rows out of range
        assert call(None, 1, C.byref(inp), n_rows, g, g, g, g, g, None, None) == bad
        assert b"n_rows" in lib.cpmpc_last_error()
        assert host(None, 1, C.byref(inp), n_rows, buf, buf, buf, buf, buf, None) == bad
    no_x0 = _inputs(capi, buf)
    no_x0.x0 = None                                                                    # null x0
    assert call(None, 1, C.byref(no_x0), 1, g, g, g, g, g, None, None) == bad
    assert b"x0" in lib.cpmpc_last_error()
    assert host(None, 1, C.byref(no_x0), 1, buf, buf, buf, buf, buf, None) == bad
    for outs in ((g, None, None), (None, g, None), (None, None, g), (g, g, g)):        # null gbar with a gradient output
        assert call(None, 1, C.byref(inp), 1, None, outs[0], outs[1], outs[2], g, None, None) == bad
        assert b"gbar" in lib.cpmpc_last_error()
        assert host(None, 1, C.byref(inp), 1, None, outs[0] and buf, outs[1] and buf, outs[2] and buf, buf, None) == bad
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(call(None, 1, C.byref(inp), 0, g, g, None, None, None, None, None))
    assert e.value.code == bad


def test_without_a_device_the_answer_is_no_device(lib, pkg):
    """Well-formed arguments and no handle (none can be made without a device: cpmpc_create reports the same): there is no
    CPU compute path to fall back to.  With a device present the null handle is an argument error."""
    capi = pkg.capi
    buf = (C.c_double * 64)()
    g = C.cast(buf, C.c_void_p)
    inp = _inputs(capi, buf)
    expected = capi.ERR_NO_DEVICE if lib.cpmpc_device_count() == 0 else capi.ERR_INVALID_ARG
    h = C.c_void_p()
    p = pkg.default_params()
    if lib.cpmpc_device_count() == 0:
        assert lib.cpmpc_create(C.byref(p), None, capi.F64, 64, 0, C.byref(h)) == capi.ERR_NO_DEVICE
    assert lib.cpmpc_plan_weight_vjp_batch(None, 1, C.byref(inp), 1, g, g, g, g, g, None, None) == expected
    assert lib.cpmpc_plan_weight_vjp_batch(None, 1, C.byref(inp), 1, None, None, None, None, g, None, None) == expected  # du alone
    assert lib.cpmpc_plan_weight_vjp_batch_host(None, 1, C.byref(inp), 1, buf, buf, buf, buf, buf, None) == expected
    if expected == capi.ERR_NO_DEVICE:
        assert b"no CPU fallback" in lib.cpmpc_last_error() or b"not gfx950" in lib.cpmpc_last_error()


def test_pypendulum_gains_plan_weight_vjp(lib, pkg):
    """The binding of Optimization gained plan_weight_vjp and lost nothing."""
    pp = pkg.pypendulum()
    for name in ("step", "step_batch", "reset", "set_previous_solution", "get_solution_batch", "feedback_gain",
                 "plan_sensitivity", "plan_vjp", "plan_weight_vjp"):
        assert hasattr(pp.Optimization, name), name


def test_batch_api_has_the_weight_gradients(pkg):
    import inspect
    assert callable(pkg.BatchOptimization.plan_weight_vjp)
    sig = inspect.signature(pkg.BatchOptimization.plan_weight_vjp)
    assert list(sig.parameters)[1:] == ["x0", "dyn", "gbar", "set_point", "u_prev", "z", "terminal_weights", "want", "want_du",
                                        "want_ok"]
    assert sig.parameters["want"].default == ("terminal", "u", "du_dt")
    sd = inspect.signature(pkg.BatchOptimization.step_differentiable)
    assert sd.parameters["weight_grad"].default is False
