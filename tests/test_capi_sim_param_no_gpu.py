"""The per-problem plant step and the plant step's parameter Jacobian in the C-ABI without a GPU: exported, prototyped in
capi.py, the argument checks answer CPMPC_ERR_INVALID_ARG before any device is needed, the ctypes mirror of
cpmpc_sim_param_jac has the C compiler's layout, and the facade and the package carry the new names beside the old ones."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import DYN_TEST, ROOT

NAMES = ("cpmpc_sim_step_dyn_batch", "cpmpc_sim_step_param_jac_batch", "cpmpc_sim_step_param_jac_batch_host")
FIELDS = ["struct_size", "state", "u", "fext_host", "fext", "dyn", "x_new", "P", "gbar", "gp", "gx", "gu"]


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
    assert len(lib.cpmpc_sim_step_dyn_batch.argtypes) == 11
    assert len(lib.cpmpc_sim_step_param_jac_batch.argtypes) == 7
    assert len(lib.cpmpc_sim_step_param_jac_batch_host.argtypes) == 9


# distinct slices of one buffer (never dereferenced: the checks come first); B = 8 doubles per row
OFF = dict(state=0, u=1024, x_new=2048, P=4096, gbar=16384, gp=20480, gx=24576, gu=28672, dyn=32768)


def _args(capi, buf, **kw):
    base = C.addressof(buf)
    a = capi.SimParamJac(struct_size=C.sizeof(capi.SimParamJac), state=base + OFF["state"], u=base + OFF["u"],
                         x_new=base + OFF["x_new"], P=base + OFF["P"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf = (C.c_double * 8192)()
    base = C.addressof(buf)
    dyn = capi.dbl_array(DYN_TEST, 9)
    call = lib.cpmpc_sim_step_param_jac_batch
    bad = capi.ERR_INVALID_ARG
    gb, gp, gx, gu, dv = (base + OFF[k] for k in ("gbar", "gp", "gx", "gu", "dyn"))

    def rc(a, dt=0.01, d=dyn, model=0, dtype=capi.F64, B=8):
        return call(model, dtype, B, d, dt, None if a is None else C.byref(a), None)

    assert rc(None) == bad and b"null" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf, state=None)) == bad and b"null" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf, u=None)) == bad and b"null" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf), d=None) == bad and b"dyn" in lib.cpmpc_last_error()     # neither parameter set
    assert rc(_args(capi, buf, struct_size=C.sizeof(capi.SimParamJac) - 8)) == bad and b"struct_size" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf, struct_size=0)) == bad and b"struct_size" in lib.cpmpc_last_error()
    for dt in (-0.01, float("nan"), float("inf")):
        assert rc(_args(capi, buf), dt=dt) == bad and b"dt" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf, x_new=None, P=None)) == bad and b"no output" in lib.cpmpc_last_error()
    for name, addr in (("gp", gp), ("gx", gx), ("gu", gu)):                              # a gradient without gbar
        assert rc(_args(capi, buf, **{name: addr})) == bad and b"gbar" in lib.cpmpc_last_error(), name
    assert rc(_args(capi, buf, gbar=gb)) == bad and b"gbar" in lib.cpmpc_last_error()    # gbar with none of them
    assert rc(_args(capi, buf, x_new=None, P=None, gbar=gb)) == bad
    for field in ("x_new", "P", "gp", "gx", "gu"):                                       # overlapping what is only read
        for target, addr in (("state", base + OFF["state"]), ("gbar", gb), ("dyn", dv)):
            kw = dict(gbar=gb, gp=gp, gx=gx, gu=gu, dyn=dv)
            kw[field] = addr
            assert rc(_args(capi, buf, **kw)) == bad, (field, target)
            assert target.encode() in lib.cpmpc_last_error() and field.encode() in lib.cpmpc_last_error(), (field, target)
    assert rc(_args(capi, buf), model=7) == bad and b"model" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf), dtype=5) == bad and b"dtype" in lib.cpmpc_last_error()
    assert rc(_args(capi, buf), B=0) == bad and b"B" in lib.cpmpc_last_error()
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(rc(None))
    assert e.value.code == bad
    # the host-pointer form
    host = lib.cpmpc_sim_step_param_jac_batch_host
    st, u1 = (C.c_double * 4)(), (C.c_double * 1)(1.0)
    P, xn = (C.c_double * 36)(), (C.c_double * 4)()
    assert host(0, 1, None, 0.01, st, u1, None, P, xn) == bad
    assert host(0, 1, dyn, 0.01, None, u1, None, P, xn) == bad
    assert host(0, 1, dyn, 0.01, st, None, None, P, xn) == bad
    assert host(0, 1, dyn, 0.01, st, u1, None, None, xn) == bad
    assert host(0, 1, dyn, -1.0, st, u1, None, P, xn) == bad and b"dt" in lib.cpmpc_last_error()
    assert host(0, 0, dyn, 0.01, st, u1, None, P, xn) == bad
    assert host(3, 1, dyn, 0.01, st, u1, None, P, xn) == bad
    assert host(0, 1, dyn, 0.01, st, (C.c_double * 1)(float("nan")), None, P, xn) == bad


def test_per_problem_plant_step_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf = (C.c_double * 8192)()
    base = C.addressof(buf)
    dyn = capi.dbl_array(DYN_TEST, 9)
    call = lib.cpmpc_sim_step_dyn_batch
    bad = capi.ERR_INVALID_ARG
    st, u, dv = C.c_void_p(base), C.c_void_p(base + 1024), C.c_void_p(base + 32768)

    def rc(d=dyn, dev=dv, dt=0.01, uu=u, state=st, model=0, dtype=capi.F64, B=8):
        return call(model, dtype, B, d, dev, dt, uu, None, None, state, None)

    assert rc(d=None, dev=None) == bad and b"null" in lib.cpmpc_last_error()   # neither parameter set
    for kw in (dict(uu=None), dict(state=None)):
        assert rc(**kw) == bad and b"null" in lib.cpmpc_last_error()
        assert rc(dev=None, **kw) == bad
    for dt in (-0.01, float("nan"), float("inf")):
        assert rc(dt=dt) == bad and b"dt" in lib.cpmpc_last_error()
        assert rc(dt=dt, dev=None) == bad
    assert rc(model=7) == bad and b"model" in lib.cpmpc_last_error()
    assert rc(dtype=5) == bad and b"dtype" in lib.cpmpc_last_error()
    assert rc(B=0) == bad and b"B" in lib.cpmpc_last_error()
    assert rc(dev=st) == bad and b"overlaps" in lib.cpmpc_last_error()         # the state is written, dyn only read


def test_well_formed_calls_get_as_far_as_the_device(lib, pkg):
    """Without a gfx950 device a well-formed call is CPMPC_ERR_NO_DEVICE, as every compute entry point."""
    if lib.cpmpc_device_count() > 0:
        pytest.skip("a GPU is present")
    capi = pkg.capi
    buf = (C.c_double * 8192)()
    base = C.addressof(buf)
    dyn = capi.dbl_array(DYN_TEST, 9)
    call = lib.cpmpc_sim_step_param_jac_batch
    gb, gp, gx, gu, dv = (base + OFF[k] for k in ("gbar", "gp", "gx", "gu", "dyn"))
    for a, d in ((_args(capi, buf), dyn), (_args(capi, buf, dyn=dv), None), (_args(capi, buf, dyn=dv), dyn),
                 (_args(capi, buf, x_new=None, P=None, gbar=gb, gp=gp), dyn),
                 (_args(capi, buf, gbar=gb, gp=gp, gx=gx, gu=gu, dyn=dv), None)):
        for dt in (0.01, 0.0):
            assert call(0, capi.F64, 8, d, dt, C.byref(a), None) == capi.ERR_NO_DEVICE
    assert call(1, capi.F32, 8, capi.dbl_array([1.0, 0.1, 0.1, 0.25, 0.2, 9.81], 6), 0.01, C.byref(_args(capi, buf)), None) \
        == capi.ERR_NO_DEVICE
    st, u1 = (C.c_double * 4)(), (C.c_double * 1)(1.0)
    P, xn = (C.c_double * 36)(), (C.c_double * 4)()
    assert lib.cpmpc_sim_step_param_jac_batch_host(0, 1, dyn, 0.01, st, u1, None, P, xn) == capi.ERR_NO_DEVICE
    assert lib.cpmpc_sim_step_param_jac_batch_host(0, 1, dyn, 0.01, st, u1, None, P, None) == capi.ERR_NO_DEVICE
    s_, u_, d_ = C.c_void_p(base), C.c_void_p(base + 1024), C.c_void_p(base + 32768)
    assert lib.cpmpc_sim_step_dyn_batch(0, capi.F64, 8, None, d_, 0.01, u_, None, None, s_, None) == capi.ERR_NO_DEVICE
    assert lib.cpmpc_sim_step_dyn_batch(0, capi.F64, 8, dyn, None, 0.01, u_, None, None, s_, None) == capi.ERR_NO_DEVICE
    assert lib.cpmpc_sim_step_dyn_batch(0, capi.F64, 8, dyn, d_, 0.01, u_, None, None, s_, None) == capi.ERR_NO_DEVICE


def test_struct_layout_matches_the_c_compiler(lib, pkg, tmp_path):
    """The gcc probe of test_capi_no_gpu.py for cpmpc_sim_param_jac."""
    cls = pkg.capi.SimParamJac
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cpmpc.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(cpmpc_sim_param_jac));']
    for f, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(cpmpc_sim_param_jac, %s));' % (f, f))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    assert [f for f, _ in cls._fields_] == FIELDS
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_pypendulum_simulator_gains_step_param_jacobian(lib, pkg):
    pp = pkg.pypendulum()
    for name in ("step", "get_state", "set_state", "step_jacobian", "step_param_jacobian"):
        assert hasattr(pp.Simulator, name), name
    sim = pp.Simulator()
    with pytest.raises(ValueError):   # dt < 0, before any device is needed (simulator.cc:13)
        sim.step_param_jacobian(pp.SingleCartPoleParams(*DYN_TEST), -0.01, 0.0, pp.Vector2(0.0, 0.0), pp.Vector2(0.0, 0.0))


def test_package_has_the_parameter_calls(pkg):
    import inspect
    for name in ("sim_step_param_jacobian", "sim_step_param_vjp", "sim_step_jacobian", "sim_step_vjp", "sim_step"):
        assert callable(getattr(pkg, name)), name
    assert "plant_dyn" in inspect.signature(pkg.ClosedLoop.tick).parameters
    assert "expand" in pkg.sim_step.__doc__   # how a shared parameter set receives a gradient
