"""The feedback-gain entry points of the C-ABI without a GPU: exported, prototyped in capi.py, struct mirrored, and the
argument checks answer CPMPC_ERR_INVALID_ARG before any device is needed."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

NAMES = ("cpmpc_feedback_gain_batch", "cpmpc_feedback_gain_batch_host", "cpmpc_feedback_apply_batch")


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
    assert len(lib.cpmpc_feedback_gain_batch.argtypes) == 7
    assert len(lib.cpmpc_feedback_gain_batch_host.argtypes) == 6
    assert len(lib.cpmpc_feedback_apply_batch.argtypes) == 10


def test_gain_inputs_mirror_matches_the_header(lib, pkg, tmp_path):
    fields = [f for f, _ in pkg.capi.GainInputs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cpmpc.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(cpmpc_gain_inputs));']
    lines += ['  printf("%s %%zu\\n", offsetof(cpmpc_gain_inputs, %s));' % (f, f) for f in fields]
    lines += ["  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(pkg.capi.GainInputs)
    for f in fields:
        assert int(got[f]) == getattr(pkg.capi.GainInputs, f).offset, f


def test_gain_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    inp = capi.GainInputs(struct_size=C.sizeof(capi.GainInputs))
    buf = (C.c_double * 64)()
    K = C.cast(buf, C.c_void_p)
    # null handle, null inputs, null K
    assert lib.cpmpc_feedback_gain_batch(None, 1, C.byref(inp), 1, K, None, None) == capi.ERR_INVALID_ARG
    assert b"null" in lib.cpmpc_last_error()
    assert lib.cpmpc_feedback_gain_batch(None, 1, None, 1, K, None, None) == capi.ERR_INVALID_ARG
    assert lib.cpmpc_feedback_gain_batch(None, 1, C.byref(inp), 1, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.cpmpc_feedback_gain_batch(None, 1, C.byref(inp), 0, K, None, None) == capi.ERR_INVALID_ARG
    assert lib.cpmpc_feedback_gain_batch_host(None, 1, C.byref(inp), 1, buf, None) == capi.ERR_INVALID_ARG
    assert lib.cpmpc_feedback_gain_batch_host(None, 1, C.byref(inp), 1, None, None) == capi.ERR_INVALID_ARG
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(lib.cpmpc_feedback_gain_batch(None, 1, C.byref(inp), 1, K, None, None))
    assert e.value.code == capi.ERR_INVALID_ARG


def test_apply_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    call = lib.cpmpc_feedback_apply_batch
    assert call(capi.F64, capi.MODEL_SINGLE, 4, None, p, p, p, 300.0, p, None) == capi.ERR_INVALID_ARG
    assert call(capi.F64, capi.MODEL_SINGLE, 4, p, None, p, p, 300.0, p, None) == capi.ERR_INVALID_ARG
    assert call(capi.F64, capi.MODEL_SINGLE, 4, p, p, None, p, 300.0, p, None) == capi.ERR_INVALID_ARG
    assert call(capi.F64, capi.MODEL_SINGLE, 4, p, p, p, None, 300.0, p, None) == capi.ERR_INVALID_ARG
    assert call(capi.F64, capi.MODEL_SINGLE, 4, p, p, p, p, 300.0, None, None) == capi.ERR_INVALID_ARG
    assert call(capi.F64, capi.MODEL_SINGLE, 4, p, p, p, p, 0.0, p, None) == capi.ERR_INVALID_ARG
    assert call(capi.F64, capi.MODEL_SINGLE, 4, p, p, p, p, float("nan"), p, None) == capi.ERR_INVALID_ARG
    assert b"u_limit" in lib.cpmpc_last_error()
    assert call(7, capi.MODEL_SINGLE, 4, p, p, p, p, 300.0, p, None) == capi.ERR_INVALID_ARG
    assert call(capi.F64, 9, 4, p, p, p, p, 300.0, p, None) == capi.ERR_INVALID_ARG
    assert call(capi.F64, capi.MODEL_SINGLE, 0, p, p, p, p, 300.0, p, None) == capi.ERR_INVALID_ARG


def test_pypendulum_keeps_its_names_and_gains_one(lib, pkg):
    """The binding of Optimization gained feedback_gain and lost nothing."""
    pp = pkg.pypendulum()
    for name in ("step", "step_batch", "step_batch_lists", "reset", "set_previous_solution", "set_previous_solution_batch",
                 "get_solution_batch", "set_host_chunk", "feedback_gain", "horizon_beyond_parity"):
        assert hasattr(pp.Optimization, name), name
