"""The plant rollout and its adjoint in the C-ABI without a GPU (cpmpc_sim_rollout_batch, cpmpc_sim_rollout_vjp_batch):
exported, prototyped in capi.py, the argument checks answer CPMPC_ERR_INVALID_ARG before any device is needed and name the
field, well-formed calls get as far as the device, the ctypes mirrors of cpmpc_sim_rollout and cpmpc_sim_rollout_vjp have
the C compiler's layout, and the package carries the new names."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import DYN_TEST, ROOT

NAMES = ("cpmpc_sim_rollout_batch", "cpmpc_sim_rollout_vjp_batch")
FIELDS = {"SimRollout": ["struct_size", "x0", "u", "fext_host", "fext", "dyn", "xs", "x_final"],
          "SimRolloutVjp": ["struct_size", "x0", "u", "fext_host", "fext", "dyn", "xs", "gbar", "gbar_final", "g_x0", "g_u",
                            "g_p"]}
DYN_DOUBLE = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]
B, T = 8, 3


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.capi.load()


def test_symbols_exported_and_prototyped(lib, pkg):
    raw = C.CDLL(pkg.capi.LIB_PATH)
    for name in NAMES:
        assert name in pkg.capi.SYMBOLS and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == 8, name


# distinct slices of one buffer (never dereferenced: the checks come first).  B = 8 doubles per row, T = 3, the 6-state
# model's extents at the most: x0 6 rows, u 3, fext 4, dyn 9, xs / gbar 18 -- every slot is 2048 bytes = 32 rows
SLOTS = ("x0", "u", "fext", "dyn", "xs", "x_final", "gbar", "gbar_final", "g_x0", "g_u", "g_p", "xs_in")
OFF = {name: 2048 * i for i, name in enumerate(SLOTS)}


def _fwd(capi, base, **kw):
    a = capi.SimRollout(struct_size=C.sizeof(capi.SimRollout), x0=base + OFF["x0"], u=base + OFF["u"], xs=base + OFF["xs"],
                        x_final=base + OFF["x_final"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _vjp(capi, base, **kw):
    a = capi.SimRolloutVjp(struct_size=C.sizeof(capi.SimRolloutVjp), x0=base + OFF["x0"], u=base + OFF["u"],
                           xs=base + OFF["xs_in"], gbar=base + OFF["gbar"], g_x0=base + OFF["g_x0"], g_u=base + OFF["g_u"],
                           g_p=base + OFF["g_p"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _common_checks(lib, capi, call, make, base, struct_name):
    dyn = capi.dbl_array(DYN_TEST, 9)
    bad = capi.ERR_INVALID_ARG
    err = lib.cpmpc_last_error

    def rc(a, dt=0.01, d=dyn, model=0, dtype=capi.F64, nb=B, nt=T):
        return call(model, dtype, nb, d, dt, nt, None if a is None else C.byref(a), None)

    assert rc(None) == bad and b"null" in err() and struct_name in err()
    assert rc(make(capi, base, x0=None)) == bad and b"null" in err() and b"x0" in err()
    assert rc(make(capi, base, u=None)) == bad and b"null" in err() and b"u" in err()
    size = C.sizeof(getattr(capi, "SimRollout" if struct_name == b"cpmpc_sim_rollout" else "SimRolloutVjp"))
    for s in (size - 8, size + 8, 0):
        assert rc(make(capi, base, struct_size=s)) == bad and b"struct_size" in err() and struct_name in err()
    for dt in (-0.01, float("nan"), float("inf")):
        assert rc(make(capi, base), dt=dt) == bad and b"dt" in err()
    for nt in (0, -1):
        assert rc(make(capi, base), nt=nt) == bad and b"T must be >= 1" in err()
    assert rc(make(capi, base), model=7) == bad and b"model" in err()
    assert rc(make(capi, base), dtype=5) == bad and b"dtype" in err()
    assert rc(make(capi, base), nb=0) == bad and b"B" in err()
    assert rc(make(capi, base), d=None) == bad and b"dyn" in err()            # neither parameter set
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(rc(None))
    assert e.value.code == bad
    return rc


def test_rollout_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    rc = _common_checks(lib, capi, lib.cpmpc_sim_rollout_batch, _fwd, base, b"cpmpc_sim_rollout")
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    assert rc(_fwd(capi, base, xs=None, x_final=None)) == bad and b"no output" in err()
    ins = dict(x0=base + OFF["x0"], u=base + OFF["u"], fext=base + OFF["fext"], dyn=base + OFF["dyn"])
    for field in ("xs", "x_final"):                                          # overlapping what is only read
        for target, addr in ins.items():
            kw = dict(fext=ins["fext"], dyn=ins["dyn"])
            kw[field] = addr
            assert rc(_fwd(capi, base, **kw)) == bad, (field, target)
            assert b"overlaps" in err() and target.encode() in err() and field.encode() in err(), (field, target)
    # the T-sized extents count: xs that starts before u and reaches into it only through its rows of ticks 1 and 2
    row = B * 8
    assert rc(_fwd(capi, base, xs=ins["u"] - 5 * row)) == bad and b"xs overlaps u" in err()
    assert rc(_fwd(capi, base, x_final=ins["u"] + 2 * row)) == bad and b"x_final overlaps u" in err()   # u's row of tick 2


def test_rollout_vjp_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    rc = _common_checks(lib, capi, lib.cpmpc_sim_rollout_vjp_batch, _vjp, base, b"cpmpc_sim_rollout_vjp")
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    assert rc(_vjp(capi, base, g_x0=None, g_u=None, g_p=None)) == bad and b"no output" in err()
    assert rc(_vjp(capi, base, gbar=None)) == bad and b"gbar" in err() and b"gbar_final" in err()   # neither cotangent
    assert rc(_vjp(capi, base, xs=None)) == bad and b"xs" in err() and b"T > 1" in err()
    ins = dict(x0=base + OFF["x0"], u=base + OFF["u"], fext=base + OFF["fext"], dyn=base + OFF["dyn"], xs=base + OFF["xs_in"],
               gbar=base + OFF["gbar"], gbar_final=base + OFF["gbar_final"])
    for field in ("g_x0", "g_u", "g_p"):                                     # overlapping what is only read
        for target, addr in ins.items():
            kw = dict(fext=ins["fext"], dyn=ins["dyn"], gbar_final=ins["gbar_final"])
            kw[field] = addr
            assert rc(_vjp(capi, base, **kw)) == bad, (field, target)
            assert b"overlaps" in err() and target.encode() in err() and field.encode() in err(), (field, target)
    # the T-sized extents count: the last row of gbar (tick 2, state 3) and of xs; g_u's own row of tick 2 on dyn
    row = B * 8
    assert rc(_vjp(capi, base, g_p=ins["gbar"] + (T * 4 - 1) * row)) == bad and b"g_p overlaps gbar" in err()
    assert rc(_vjp(capi, base, g_x0=ins["xs"] + (T * 4 - 1) * row)) == bad and b"g_x0 overlaps xs" in err()
    assert rc(_vjp(capi, base, dyn=ins["dyn"], g_u=ins["dyn"] - 2 * row)) == bad and b"g_u overlaps dyn" in err()


def test_well_formed_calls_get_as_far_as_the_device(lib, pkg):
    """Without a gfx950 device a well-formed call is CPMPC_ERR_NO_DEVICE, as every compute entry point."""
    if lib.cpmpc_device_count() > 0:
        pytest.skip("a GPU is present")
    capi = pkg.capi
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    dv, gf = base + OFF["dyn"], base + OFF["gbar_final"]
    for model, host in ((0, capi.dbl_array(DYN_TEST, 9)), (1, capi.dbl_array(DYN_DOUBLE, 6))):
        for dtype in (capi.F32, capi.F64):
            for dt in (0.0, 0.01):
                for d, kw in ((host, {}), (None, dict(dyn=dv)), (host, dict(dyn=dv))):
                    for a in (_fwd(capi, base, **kw), _fwd(capi, base, xs=None, **kw), _fwd(capi, base, x_final=None, **kw)):
                        assert lib.cpmpc_sim_rollout_batch(model, dtype, B, d, dt, T, C.byref(a), None) == capi.ERR_NO_DEVICE
                    for a in (_vjp(capi, base, **kw), _vjp(capi, base, gbar=None, gbar_final=gf, g_u=None, **kw),
                              _vjp(capi, base, gbar_final=gf, g_x0=None, g_p=None, **kw)):
                        assert lib.cpmpc_sim_rollout_vjp_batch(model, dtype, B, d, dt, T, C.byref(a), None) \
                            == capi.ERR_NO_DEVICE
                a = _vjp(capi, base, xs=None)                                  # T = 1 needs no checkpoints
                assert lib.cpmpc_sim_rollout_vjp_batch(model, dtype, B, host, dt, 1, C.byref(a), None) == capi.ERR_NO_DEVICE


@pytest.mark.parametrize("cls_name,c_name", [("SimRollout", "cpmpc_sim_rollout"), ("SimRolloutVjp", "cpmpc_sim_rollout_vjp")])
def test_struct_layout_matches_the_c_compiler(lib, pkg, tmp_path, cls_name, c_name):
    """The gcc probe of test_capi_no_gpu.py for the two rollout structs."""
    cls = getattr(pkg.capi, cls_name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cpmpc.h"', "int main(void) {",
             '  printf("size %%zu\\n", sizeof(%s));' % c_name]
    for f, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (f, c_name, f))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    assert [f for f, _ in cls._fields_] == FIELDS[cls_name]
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_package_has_the_rollout_calls(pkg):
    for name in ("sim_rollout_states", "sim_rollout_vjp", "sim_rollout"):
        assert callable(getattr(pkg, name)), name
    for name in ("rollout", "rollout_differentiable"):
        assert callable(getattr(pkg.BatchSimulator, name)), name
    assert "expand" in pkg.sim_rollout.__doc__   # how a shared parameter set receives a gradient
