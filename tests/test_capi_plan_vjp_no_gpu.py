"""The reverse-mode plan-sensitivity entry points of the C-ABI without a GPU: exported, prototyped in capi.py, and the
argument checks answer CPMPC_ERR_INVALID_ARG before any device is needed."""
import ctypes as C

import pytest

NAMES = ("cpmpc_plan_vjp_batch", "cpmpc_plan_vjp_batch_host")


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.capi.load()


def test_symbols_exported_and_prototyped(lib, pkg):
    raw = C.CDLL(pkg.capi.LIB_PATH)
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS and hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.cpmpc_plan_vjp_batch.argtypes) == 10
    assert len(lib.cpmpc_plan_vjp_batch_host.argtypes) == 9


def test_vjp_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    buf = (C.c_double * 64)()
    g = C.cast(buf, C.c_void_p)
    call, host = lib.cpmpc_plan_vjp_batch, lib.cpmpc_plan_vjp_batch_host
    # null handle, whichever outputs are asked for
    for outs in ((g, g, g), (g, None, None), (None, g, None), (None, None, g)):
        assert call(None, 1, C.byref(inp), 1, g, outs[0], outs[1], outs[2], None, None) == capi.ERR_INVALID_ARG
        assert b"null" in lib.cpmpc_last_error()
        assert host(None, 1, C.byref(inp), 1, buf, outs[0] and buf, outs[1] and buf, outs[2] and buf,
                    None) == capi.ERR_INVALID_ARG
    assert call(None, 1, None, 1, g, g, g, g, None, None) == capi.ERR_INVALID_ARG                 # null inputs
    assert call(None, 1, C.byref(inp), 1, None, g, g, g, None, None) == capi.ERR_INVALID_ARG      # null gbar
    assert b"gbar" in lib.cpmpc_last_error()
    assert call(None, 1, C.byref(inp), 1, g, None, None, None, None, None) == capi.ERR_INVALID_ARG   # no output
    assert call(None, 1, C.byref(inp), 0, g, g, g, g, None, None) == capi.ERR_INVALID_ARG         # n_rows = 0
    assert host(None, 1, None, 1, buf, buf, buf, buf, None) == capi.ERR_INVALID_ARG
    assert host(None, 1, C.byref(inp), 1, None, buf, buf, buf, None) == capi.ERR_INVALID_ARG
    assert b"gbar" in lib.cpmpc_last_error()
    assert host(None, 1, C.byref(inp), 1, buf, None, None, None, None) == capi.ERR_INVALID_ARG
    assert host(None, 1, C.byref(inp), 0, buf, buf, None, None, None) == capi.ERR_INVALID_ARG
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(call(None, 1, C.byref(inp), 1, g, g, None, None, None, None))
    assert e.value.code == capi.ERR_INVALID_ARG


def test_pypendulum_gains_plan_vjp(lib, pkg):
    """The binding of Optimization gained plan_vjp and lost nothing."""
    pp = pkg.pypendulum()
    for name in ("step", "step_batch", "reset", "set_previous_solution", "get_solution_batch", "feedback_gain",
                 "plan_sensitivity", "plan_vjp"):
        assert hasattr(pp.Optimization, name), name


def test_batch_api_has_the_reverse_mode(pkg):
    for name in ("plan_vjp", "step_differentiable"):
        assert callable(getattr(pkg.BatchOptimization, name)), name
