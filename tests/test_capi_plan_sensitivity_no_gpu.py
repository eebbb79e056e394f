"""The plan-sensitivity and plan-update entry points of the C-ABI without a GPU: exported, prototyped in capi.py, the struct
mirrored, and the argument checks answer CPMPC_ERR_INVALID_ARG before any device is needed."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

NAMES = ("cpmpc_plan_sensitivity_batch", "cpmpc_plan_sensitivity_batch_host", "cpmpc_plan_update_batch")


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
    assert len(lib.cpmpc_plan_sensitivity_batch.argtypes) == 9
    assert len(lib.cpmpc_plan_sensitivity_batch_host.argtypes) == 8
    assert len(lib.cpmpc_plan_update_batch.argtypes) == 6


def test_plan_update_mirror_matches_the_header(lib, pkg, tmp_path):
    fields = [f for f, _ in pkg.capi.PlanUpdate._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cpmpc.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(cpmpc_plan_update));']
    lines += ['  printf("%s %%zu\\n", offsetof(cpmpc_plan_update, %s));' % (f, f) for f in fields]
    lines += ["  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(pkg.capi.PlanUpdate)
    assert len(fields) == 13
    for f in fields:
        assert int(got[f]) == getattr(pkg.capi.PlanUpdate, f).offset, f


def test_sensitivity_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    buf = (C.c_double * 64)()
    k = C.cast(buf, C.c_void_p)
    call, host = lib.cpmpc_plan_sensitivity_batch, lib.cpmpc_plan_sensitivity_batch_host
    # null handle, whichever outputs are asked for
    for outs in ((k, k, k), (k, None, None), (None, k, None), (None, None, k)):
        assert call(None, 1, C.byref(inp), 1, outs[0], outs[1], outs[2], None, None) == capi.ERR_INVALID_ARG
        assert b"null" in lib.cpmpc_last_error()
    assert call(None, 1, None, 1, k, k, k, None, None) == capi.ERR_INVALID_ARG          # null inputs
    assert call(None, 1, C.byref(inp), 1, None, None, None, None, None) == capi.ERR_INVALID_ARG   # no outputs
    assert call(None, 1, C.byref(inp), 0, k, k, k, None, None) == capi.ERR_INVALID_ARG  # n_rows = 0
    assert host(None, 1, C.byref(inp), 1, buf, buf, buf, None) == capi.ERR_INVALID_ARG
    assert host(None, 1, C.byref(inp), 1, None, None, None, None) == capi.ERR_INVALID_ARG
    assert host(None, 1, C.byref(inp), 0, buf, None, None, None) == capi.ERR_INVALID_ARG
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(call(None, 1, C.byref(inp), 1, k, None, None, None, None))
    assert e.value.code == capi.ERR_INVALID_ARG


def _full(capi, p):
    a = capi.PlanUpdate(struct_size=C.sizeof(capi.PlanUpdate), u_limit=300.0)
    for f, _ in capi.PlanUpdate._fields_:
        if f not in ("struct_size", "u_limit"):
            setattr(a, f, p)
    return a


def test_update_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    call = lib.cpmpc_plan_update_batch

    def rc(a, dtype=capi.F64, model=capi.MODEL_SINGLE, B=4, n_rows=2):
        return call(dtype, model, B, n_rows, C.byref(a) if a is not None else None, None)
    assert rc(None) == capi.ERR_INVALID_ARG
    # a sensitivity without its pair of nominal / actual arrays
    for sens, pair in (("K", ("x_nom", "x")), ("k_sp", ("sp_nom", "sp")), ("k_up", ("u_prev_nom", "u_prev"))):
        for missing in pair:
            a = _full(capi, p)
            setattr(a, missing, None)
            assert rc(a) == capi.ERR_INVALID_ARG, (sens, missing)
            assert sens.encode() in lib.cpmpc_last_error()
    for missing in ("u_nom", "u_out"):
        a = _full(capi, p)
        setattr(a, missing, None)
        assert rc(a) == capi.ERR_INVALID_ARG, missing
    for bad in (0.0, -1.0, float("nan")):
        a = _full(capi, p)
        a.u_limit = bad
        assert rc(a) == capi.ERR_INVALID_ARG
        assert b"u_limit" in lib.cpmpc_last_error()
    a = _full(capi, p)
    a.struct_size = 8
    assert rc(a) == capi.ERR_INVALID_ARG and b"struct_size" in lib.cpmpc_last_error()
    a = _full(capi, p)
    assert rc(a, n_rows=0) == capi.ERR_INVALID_ARG
    assert rc(a, n_rows=65536) == capi.ERR_INVALID_ARG   # the documented upper limit
    assert rc(a, dtype=7) == capi.ERR_INVALID_ARG
    assert rc(a, model=9) == capi.ERR_INVALID_ARG
    assert rc(a, B=0) == capi.ERR_INVALID_ARG


def test_pypendulum_gains_plan_sensitivity(lib, pkg):
    """The binding of Optimization gained plan_sensitivity and lost nothing."""
    pp = pkg.pypendulum()
    for name in ("step", "step_batch", "reset", "set_previous_solution", "get_solution_batch", "feedback_gain",
                 "plan_sensitivity"):
        assert hasattr(pp.Optimization, name), name
