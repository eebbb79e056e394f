"""The rollout's forward mode in the initial state with the normal equations of the fit of x0 in the C-ABI without a GPU
(cpmpc_sim_rollout_gn_x0_batch), point for point as tests/test_capi_sim_rollout_gn_no_gpu.py: exported, prototyped in capi.py,
the argument checks answer CPMPC_ERR_INVALID_ARG before any device is needed and name the field, a well-formed call gets as far
as the device, the ctypes mirror of cpmpc_sim_rollout_gn_x0 has the C compiler's layout, and the package carries the new
names."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import DYN_TEST, ROOT

NAME = "cpmpc_sim_rollout_gn_x0_batch"
FIELDS = ["struct_size", "x0", "u", "fext_host", "fext", "dyn", "x_obs", "w_host", "tick_w", "cost", "g", "H", "Phi_final",
          "x_final"]
DYN_DOUBLE = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]
B, T = 8, 3
OUTPUTS = ("cost", "g", "H", "Phi_final", "x_final")


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.capi.load()


def test_symbol_exported_and_prototyped(lib, pkg):
    raw = C.CDLL(pkg.capi.LIB_PATH)
    assert NAME in pkg.capi.SYMBOLS and hasattr(raw, NAME)
    assert len(getattr(lib, NAME).argtypes) == 8
    with open(os.path.join(ROOT, "include", "cpmpc.h")) as fh:
        header = fh.read()
    assert "int %s(" % NAME in header
    assert "g = dcost/dx0" in header and header.count("-H^-1 g") >= 2     # the sign convention is stated, here too


# distinct slices of one buffer (never dereferenced: the checks come first).  B = 8 doubles per row, T = 3, the 4-state
# model's extents at the most: x_obs 12 rows, H 16, Phi_final 16 -- every slot is 8192 bytes = 128 rows
SLOTS = ("x0", "u", "fext", "dyn", "x_obs", "tick_w", "cost", "g", "H", "Phi_final", "x_final")
OFF = {name: 8192 * i for i, name in enumerate(SLOTS)}


def _gn(capi, base, **kw):
    a = capi.SimRolloutGnX0(struct_size=C.sizeof(capi.SimRolloutGnX0), x0=base + OFF["x0"], u=base + OFF["u"],
                            x_obs=base + OFF["x_obs"], **{name: base + OFF[name] for name in OUTPUTS})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _buffer():
    buf = (C.c_double * (1024 * len(SLOTS)))()
    return buf, C.addressof(buf)


def test_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf, base = _buffer()
    dyn = capi.dbl_array(DYN_TEST, 9)
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    call = lib.cpmpc_sim_rollout_gn_x0_batch

    def rc(a, dt=0.01, d=dyn, model=0, dtype=capi.F64, nb=B, nt=T):
        return call(model, dtype, nb, d, dt, nt, None if a is None else C.byref(a), None)

    # what every rollout call checks
    assert rc(None) == bad and b"null" in err() and b"cpmpc_sim_rollout_gn_x0" in err()
    assert rc(_gn(capi, base, x0=None)) == bad and b"null" in err() and b"x0" in err()
    assert rc(_gn(capi, base, u=None)) == bad and b"null" in err() and b"u" in err()
    size = C.sizeof(capi.SimRolloutGnX0)
    for s in (size - 8, size + 8, 0):
        assert rc(_gn(capi, base, struct_size=s)) == bad and b"struct_size" in err() and b"cpmpc_sim_rollout_gn_x0" in err()
    for dt in (-0.01, float("nan"), float("inf")):
        assert rc(_gn(capi, base), dt=dt) == bad and b"dt" in err()
    for nt in (0, -1):
        assert rc(_gn(capi, base), nt=nt) == bad and b"T must be >= 1" in err()
    assert rc(_gn(capi, base), model=7) == bad and b"model" in err()
    assert rc(_gn(capi, base), dtype=5) == bad and b"dtype" in err()
    assert rc(_gn(capi, base), nb=0) == bad and b"B" in err()
    assert rc(_gn(capi, base), d=None) == bad and b"dyn" in err()            # neither parameter set
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(rc(None))
    assert e.value.code == bad

    # the call's own rules
    assert rc(_gn(capi, base, **{name: None for name in OUTPUTS})) == bad and b"no output" in err()
    for name in ("cost", "g", "H"):                                           # each needs the recording
        others = {o: None for o in OUTPUTS if o != name}
        assert rc(_gn(capi, base, x_obs=None, **others)) == bad and b"x_obs" in err(), name
    for q, v in ((0, -1.0), (1, float("nan")), (3, float("inf")), (2, -1e-300)):
        w = [1.0, 1.0, 1.0, 1.0]
        w[q] = v
        arr = capi.dbl_array(w, 4)
        assert rc(_gn(capi, base, w_host=C.cast(arr, C.POINTER(C.c_double)))) == bad, (q, v)
        assert b"w_host[%d]" % q in err(), (q, v)
    ins = dict(x0=base + OFF["x0"], u=base + OFF["u"], fext=base + OFF["fext"], dyn=base + OFF["dyn"],
               x_obs=base + OFF["x_obs"], tick_w=base + OFF["tick_w"])
    for field in OUTPUTS:                                                      # overlapping what is only read
        for target, addr in ins.items():
            kw = dict(fext=ins["fext"], dyn=ins["dyn"], tick_w=ins["tick_w"])
            kw[field] = addr
            assert rc(_gn(capi, base, **kw)) == bad, (field, target)
            assert b"overlaps" in err() and target.encode() in err() and field.encode() in err(), (field, target)
    # the extents count: the last row of x_obs (tick 2, state 3), of tick_w (tick 2), and the 16th rows of H and Phi_final
    row = B * 8
    assert rc(_gn(capi, base, cost=ins["x_obs"] + (T * 4 - 1) * row)) == bad and b"cost overlaps x_obs" in err()
    assert rc(_gn(capi, base, tick_w=ins["tick_w"], g=ins["tick_w"] + (T - 1) * row)) == bad and b"g overlaps tick_w" in err()
    assert rc(_gn(capi, base, H=ins["x0"] - 15 * row)) == bad and b"H overlaps x0" in err()
    assert rc(_gn(capi, base, Phi_final=ins["u"] - 15 * row)) == bad and b"Phi_final overlaps u" in err()
    # the 6-state model's 36 rows
    d6 = capi.dbl_array(DYN_DOUBLE, 6)
    assert rc(_gn(capi, base, H=ins["x0"] - 35 * row), model=1, d=d6) == bad and b"H overlaps x0" in err()
    assert rc(_gn(capi, base, Phi_final=ins["u"] - 35 * row), model=1, d=d6) == bad and b"Phi_final overlaps u" in err()


def test_a_well_formed_call_gets_as_far_as_the_device(lib, pkg):
    """Without a gfx950 device a well-formed call is CPMPC_ERR_NO_DEVICE, as every compute entry point."""
    if lib.cpmpc_device_count() > 0:
        pytest.skip("a GPU is present")
    capi = pkg.capi
    buf, base = _buffer()
    dv, tw = base + OFF["dyn"], base + OFF["tick_w"]
    none = {name: None for name in OUTPUTS}
    for model, host, nx in ((0, capi.dbl_array(DYN_TEST, 9), 4), (1, capi.dbl_array(DYN_DOUBLE, 6), 6)):
        w = capi.dbl_array([1.0] * (nx // 2) + [0.0] * (nx // 2), nx)
        wp = C.cast(w, C.POINTER(C.c_double))
        for dtype in (capi.F32, capi.F64):
            for dt in (0.0, 0.01):
                for d, kw in ((host, {}), (None, dict(dyn=dv)), (host, dict(dyn=dv, tick_w=tw, w_host=wp))):
                    forms = [_gn(capi, base, **kw)] + \
                            [_gn(capi, base, **dict(none, **{name: base + OFF[name]}), **kw) for name in OUTPUTS]
                    # the derivative and the last state alone need no recording
                    forms.append(_gn(capi, base, x_obs=None, cost=None, g=None, H=None, **kw))
                    for a in forms:
                        assert lib.cpmpc_sim_rollout_gn_x0_batch(model, dtype, B, d, dt, T, C.byref(a), None) == capi.ERR_NO_DEVICE


def test_struct_layout_matches_the_c_compiler(lib, pkg, tmp_path):
    """The gcc probe of test_capi_no_gpu.py for cpmpc_sim_rollout_gn_x0."""
    cls, c_name = pkg.capi.SimRolloutGnX0, "cpmpc_sim_rollout_gn_x0"
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
    assert [f for f, _ in cls._fields_] == FIELDS
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_package_has_the_estimation_calls(pkg):
    for name in ("sim_rollout_gauss_newton_x0", "sim_estimate_state", "WindowEstimator"):
        assert callable(getattr(pkg, name)), name
    assert "-H^-1 g" in pkg.sim_rollout_gauss_newton_x0.__doc__             # the sign convention
    assert "arrival cost" in pkg.sim_estimate_state.__doc__
    assert "ClosedLoop.set_state" in pkg.WindowEstimator.__doc__
