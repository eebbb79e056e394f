"""The plant-step Jacobian entry points of the C-ABI without a GPU: exported, prototyped in capi.py, the argument checks answer
CPMPC_ERR_INVALID_ARG before any device is needed, the ctypes mirror of cpmpc_sim_jac has the C compiler's layout, and the
facade and the package carry the new names beside the old ones."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import DYN_TEST, ROOT

NAMES = ("cpmpc_sim_step_jac_batch", "cpmpc_sim_step_jac_batch_host")


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
    assert len(lib.cpmpc_sim_step_jac_batch.argtypes) == 7
    assert len(lib.cpmpc_sim_step_jac_batch_host.argtypes) == 9


def _args(capi, buf, **kw):
    """A well-formed cpmpc_sim_jac over distinct slices of `buf` (never dereferenced: the checks come first)."""
    base = C.addressof(buf)
    a = capi.SimJac(struct_size=C.sizeof(capi.SimJac), state=base, u=base + 1024, x_new=base + 2048, A=base + 4096,
                    Bu=base + 3072)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    dyn = capi.dbl_array(DYN_TEST, 9)
    call = lib.cpmpc_sim_step_jac_batch
    bad = capi.ERR_INVALID_ARG

    def rc(a, dt=0.01, d=dyn, model=0, dtype=capi.F64, B=8):
        return call(model, dtype, B, d, dt, None if a is None else C.byref(a), None)

    assert rc(None) == bad and b"null" in lib.cpmpc_last_error()              # null struct
    assert rc(_args(capi, buf, state=None)) == bad and b"null" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf, u=None)) == bad
    assert rc(_args(capi, buf), d=None) == bad
    assert rc(_args(capi, buf, struct_size=C.sizeof(capi.SimJac) - 8)) == bad and b"struct_size" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf, struct_size=0)) == bad
    for dt in (-0.01, float("nan"), float("inf")):
        assert rc(_args(capi, buf), dt=dt) == bad and b"dt" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf, x_new=None, A=None, Bu=None)) == bad and b"no output" in lib.cpmpc_last_error()
    gb, gx, gu = base + 16384, base + 20480, base + 24576
    assert rc(_args(capi, buf, gx=gx)) == bad and b"gbar" in lib.cpmpc_last_error()      # gx without gbar
    assert rc(_args(capi, buf, gu=gu)) == bad and b"gbar" in lib.cpmpc_last_error()      # gu without gbar
    assert rc(_args(capi, buf, gbar=gb)) == bad and b"gbar" in lib.cpmpc_last_error()    # gbar with neither
    assert rc(_args(capi, buf, x_new=None, A=None, Bu=None, gbar=gb)) == bad
    for field in ("x_new", "gx", "A"):                                                   # aliasing what is only read
        for target, addr in (("state", base), ("gbar", gb)):
            kw = dict(gbar=gb, gx=gx)
            kw[field] = addr
            assert rc(_args(capi, buf, **kw)) == bad, (field, target)
            assert target.encode() in lib.cpmpc_last_error(), (field, target)
    assert rc(_args(capi, buf), model=7) == bad
    assert rc(_args(capi, buf), dtype=5) == bad
    assert rc(_args(capi, buf), B=0) == bad
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(rc(None))
    assert e.value.code == bad
    # the host-pointer form
    host = lib.cpmpc_sim_step_jac_batch_host
    st, u1 = (C.c_double * 4)(), (C.c_double * 1)(1.0)
    A, Bu = (C.c_double * 16)(), (C.c_double * 4)()
    assert host(0, 1, None, 0.01, st, u1, None, A, Bu) == bad
    assert host(0, 1, dyn, 0.01, None, u1, None, A, Bu) == bad
    assert host(0, 1, dyn, 0.01, st, None, None, A, Bu) == bad
    assert host(0, 1, dyn, 0.01, st, u1, None, None, None) == bad
    assert host(0, 1, dyn, -1.0, st, u1, None, A, Bu) == bad
    assert host(0, 0, dyn, 0.01, st, u1, None, A, Bu) == bad
    assert host(3, 1, dyn, 0.01, st, u1, None, A, Bu) == bad
    assert host(0, 1, dyn, 0.01, st, (C.c_double * 1)(float("nan")), None, A, Bu) == bad


def test_well_formed_calls_get_as_far_as_the_device(lib, pkg):
    """Without a gfx950 device a well-formed call is CPMPC_ERR_NO_DEVICE, as every compute entry point."""
    if lib.cpmpc_device_count() > 0:
        pytest.skip("a GPU is present")
    capi = pkg.capi
    buf = (C.c_double * 4096)()
    dyn = capi.dbl_array(DYN_TEST, 9)
    a = _args(capi, buf)
    assert lib.cpmpc_sim_step_jac_batch(0, capi.F64, 8, dyn, 0.01, C.byref(a), None) == capi.ERR_NO_DEVICE
    assert lib.cpmpc_sim_step_jac_batch(0, capi.F64, 8, dyn, 0.0, C.byref(a), None) == capi.ERR_NO_DEVICE
    st, u1 = (C.c_double * 4)(), (C.c_double * 1)(1.0)
    A, Bu = (C.c_double * 16)(), (C.c_double * 4)()
    assert lib.cpmpc_sim_step_jac_batch_host(0, 1, dyn, 0.01, st, u1, None, A, Bu) == capi.ERR_NO_DEVICE
    # the plant step itself answers as before
    one = C.c_void_p(8)
    assert lib.cpmpc_sim_step_batch(capi.F64, 1, dyn, 0.01, one, None, None, one, None) == capi.ERR_NO_DEVICE
    assert lib.cpmpc_sim_step_batch(capi.F64, 1, dyn, -0.01, one, None, None, one, None) == capi.ERR_INVALID_ARG


def test_struct_layout_matches_the_c_compiler(lib, pkg, tmp_path):
    """The gcc probe of test_capi_no_gpu.py for cpmpc_sim_jac."""
    cls = pkg.capi.SimJac
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cpmpc.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(cpmpc_sim_jac));']
    for f, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(cpmpc_sim_jac, %s));' % (f, f))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    assert [f for f, _ in cls._fields_] == ["struct_size", "state", "u", "fext_host", "fext", "x_new", "A", "Bu", "gbar",
                                            "gx", "gu"]
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_pypendulum_simulator_gains_step_jacobian(lib, pkg):
    """The binding of Simulator gained step_jacobian and lost nothing."""
    pp = pkg.pypendulum()
    for name in ("step", "get_state", "set_state", "step_jacobian"):
        assert hasattr(pp.Simulator, name), name
    sim = pp.Simulator()
    with pytest.raises(ValueError):   # dt < 0, before any device is needed (simulator.cc:13)
        sim.step_jacobian(pp.SingleCartPoleParams(*DYN_TEST), -0.01, 0.0, pp.Vector2(0.0, 0.0), pp.Vector2(0.0, 0.0))


def test_package_has_the_differentiable_plant_step(pkg):
    for name in ("sim_step_jacobian", "sim_step_vjp", "sim_step"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.BatchSimulator.step_differentiable)
    assert callable(pkg.BatchSimulator.step)
