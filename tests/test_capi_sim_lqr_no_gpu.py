"""The LQR gains along a plant trajectory and the plant under an affine feedback law in the C-ABI without a GPU
(cpmpc_sim_lqr_batch, cpmpc_sim_rollout_fb_batch), point for point as tests/test_capi_sim_ekf_no_gpu.py: exported, prototyped in
capi.py, the argument checks answer CPMPC_ERR_INVALID_ARG before any device is needed and name the field, a well-formed call gets
as far as the device, the ctypes mirrors have the C compiler's layout, and the package carries the new names."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import DYN_TEST, ROOT

DYN_DOUBLE = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]
B, T = 8, 3
LQR_FIELDS = ["struct_size", "x0", "u", "fext_host", "fext", "dyn", "xs", "q_host", "r", "PT", "qf_host", "K", "P0"]
FB_FIELDS = ["struct_size", "x0", "u_nom", "fext_host", "fext", "dyn", "K", "x0_nom", "xs_nom", "u_limit", "xs", "x_final", "us"]
LQR_OUT = ("K", "P0")
FB_OUT = ("xs", "x_final", "us")


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.capi.load()


def test_symbols_exported_and_prototyped(lib, pkg):
    raw = C.CDLL(pkg.capi.LIB_PATH)
    with open(os.path.join(ROOT, "include", "cpmpc.h")) as fh:
        header = fh.read()
    for name in ("cpmpc_sim_lqr_batch", "cpmpc_sim_rollout_fb_batch"):
        assert name in pkg.capi.SYMBOLS and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == 8
        assert "int %s(" % name in header
    doc = header[header.index("TIME-VARYING LQR GAINS"):header.index("} cpmpc_sim_lqr;")]
    assert "k_t = -(Phi_t^T v) / s" in doc and "P   = diag(q_host) + r k_t k_t^T + Acl^T P Acl" in doc      # the recursion
    assert "SIGN CONVENTION" in doc and "u_t = u_nom[t] + k_t . (x_t - x_nom_t)" in doc
    assert "ONLY THE LOWER TRIANGLE" in doc and "PLANT's map at dt" in doc
    doc = header[header.index("AFFINE FEEDBACK LAW"):header.index("} cpmpc_sim_rollout_fb;")]
    assert "u_t = clamp(u_nom[t] + K[t] . d, +-u_limit)" in doc and "SIGN CONVENTION" in doc
    assert "NO feedback inside a tick" in doc and "does not know of the clamp" in doc


# distinct slices of one buffer (never dereferenced: the checks come first).  B = 8 doubles per row, T = 3, the 6-state model's
# extents at the most: PT / P0 36 rows, xs / K 18 -- every slot is 8192 bytes = 128 rows
SLOTS = ("x0", "u", "fext", "dyn", "xs_in", "PT", "K", "P0", "x0_nom", "xs_nom", "xs", "x_final", "us")
OFF = {name: 8192 * i for i, name in enumerate(SLOTS)}


def _buffer():
    buf = (C.c_double * (1024 * len(SLOTS)))()
    return buf, C.addressof(buf)


def _host(capi, values):
    arr = capi.dbl_array(values, len(values))
    return arr, C.cast(arr, C.POINTER(C.c_double))


def _lqr(capi, base, **kw):
    a = capi.SimLqr(struct_size=C.sizeof(capi.SimLqr), x0=base + OFF["x0"], u=base + OFF["u"], xs=base + OFF["xs_in"], r=0.01,
                    K=base + OFF["K"], P0=base + OFF["P0"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _fb(capi, base, **kw):
    a = capi.SimRolloutFb(struct_size=C.sizeof(capi.SimRolloutFb), x0=base + OFF["x0"], u_nom=base + OFF["u"],
                          K=base + OFF["K"], x0_nom=base + OFF["x0_nom"], xs_nom=base + OFF["xs_nom"], u_limit=300.0,
                          xs=base + OFF["xs"], x_final=base + OFF["x_final"], us=base + OFF["us"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _common_checks(capi, lib, call, make, base, c_name, u_field):
    """what every rollout call checks"""
    dyn = capi.dbl_array(DYN_TEST, 9)
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error

    def rc(a, dt=0.01, d=dyn, model=0, dtype=capi.F64, nb=B, nt=T):
        return call(model, dtype, nb, d, dt, nt, None if a is None else C.byref(a), None)

    assert rc(None) == bad and b"null" in err() and c_name in err()
    assert rc(make(capi, base, x0=None)) == bad and b"null" in err() and b"x0" in err()
    assert rc(make(capi, base, **{u_field: None})) == bad and b"null" in err() and u_field.encode() in err()
    size = make(capi, base).struct_size
    for s in (size - 8, size + 8, 0):
        assert rc(make(capi, base, struct_size=s)) == bad and b"struct_size" in err() and c_name in err()
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


def test_lqr_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf, base = _buffer()
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    rc = _common_checks(capi, lib, lib.cpmpc_sim_lqr_batch, _lqr, base, b"cpmpc_sim_lqr", "u")

    # the call's own rules
    assert rc(_lqr(capi, base, K=None, P0=None)) == bad and b"no output" in err()
    assert rc(_lqr(capi, base, xs=None)) == bad and b"xs" in err() and b"T > 1" in err()
    for r in (0.0, -1.0, float("nan"), float("inf"), -0.0):
        assert rc(_lqr(capi, base, r=r)) == bad and b"r must be finite and > 0" in err(), r
    for field in ("q_host", "qf_host"):
        for q, v in ((0, -1.0), (1, float("nan")), (3, float("inf")), (2, -1e-300)):
            w = [1.0, 1.0, 1.0, 1.0]
            w[q] = v
            _arr, ptr = _host(capi, w)
            assert rc(_lqr(capi, base, **{field: ptr})) == bad, (field, q, v)
            assert b"%s[%d]" % (field.encode(), q) in err(), (field, q, v)
    ins = dict(x0=base + OFF["x0"], u=base + OFF["u"], fext=base + OFF["fext"], dyn=base + OFF["dyn"], xs=base + OFF["xs_in"],
               PT=base + OFF["PT"])
    for field in LQR_OUT:                                                      # overlapping what is only read
        for target, addr in ins.items():
            kw = dict(fext=ins["fext"], dyn=ins["dyn"], PT=ins["PT"])
            kw[field] = addr
            assert rc(_lqr(capi, base, **kw)) == bad, (field, target)
            assert b"overlaps" in err() and target.encode() in err() and field.encode() in err(), (field, target)
    # the extents are the true ones: the last row of xs (tick 2, state 3) and of PT (row 15), K's 12 rows and P0's 16
    row = B * 8
    assert rc(_lqr(capi, base, P0=ins["xs"] + (T * 4 - 1) * row)) == bad and b"P0 overlaps xs" in err()
    assert rc(_lqr(capi, base, PT=ins["PT"], K=ins["PT"] + 15 * row)) == bad and b"K overlaps PT" in err()
    assert rc(_lqr(capi, base, K=ins["x0"] - (T * 4 - 1) * row)) == bad and b"K overlaps x0" in err()
    assert rc(_lqr(capi, base, P0=ins["u"] - 15 * row)) == bad and b"P0 overlaps u" in err()
    d6 = capi.dbl_array(DYN_DOUBLE, 6)                                        # the 6-state model's 36 and 18 rows
    assert rc(_lqr(capi, base, P0=ins["u"] - 35 * row), model=1, d=d6) == bad and b"P0 overlaps u" in err()
    assert rc(_lqr(capi, base, K=ins["x0"] - (T * 6 - 1) * row), model=1, d=d6) == bad and b"K overlaps x0" in err()


def test_feedback_rollout_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf, base = _buffer()
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    rc = _common_checks(capi, lib, lib.cpmpc_sim_rollout_fb_batch, _fb, base, b"cpmpc_sim_rollout_fb", "u_nom")

    assert rc(_fb(capi, base, xs=None, x_final=None, us=None)) == bad and b"no output" in err()
    for lim in (0.0, -1.0, float("nan")):
        assert rc(_fb(capi, base, u_limit=lim)) == bad and b"u_limit" in err(), lim
    assert rc(_fb(capi, base, x0_nom=None)) == bad and b"x0_nom" in err()
    assert rc(_fb(capi, base, xs_nom=None)) == bad and b"xs_nom" in err()
    ins = dict(x0=base + OFF["x0"], u_nom=base + OFF["u"], fext=base + OFF["fext"], dyn=base + OFF["dyn"], K=base + OFF["K"],
               x0_nom=base + OFF["x0_nom"], xs_nom=base + OFF["xs_nom"])
    for field in FB_OUT:                                                       # overlapping what is only read
        for target, addr in ins.items():
            kw = dict(fext=ins["fext"], dyn=ins["dyn"])
            kw[field] = addr
            assert rc(_fb(capi, base, **kw)) == bad, (field, target)
            assert b"overlaps" in err() and target.encode() in err() and field.encode() in err(), (field, target)
    row = B * 8
    assert rc(_fb(capi, base, us=ins["K"] + (T * 4 - 1) * row)) == bad and b"us overlaps K" in err()
    assert rc(_fb(capi, base, x_final=ins["xs_nom"] + (T * 4 - 1) * row)) == bad and b"x_final overlaps xs_nom" in err()
    assert rc(_fb(capi, base, xs=ins["u_nom"] - (T * 4 - 1) * row)) == bad and b"xs overlaps u_nom" in err()
    assert rc(_fb(capi, base, us=ins["x0"] - (T - 1) * row)) == bad and b"us overlaps x0" in err()
    d6 = capi.dbl_array(DYN_DOUBLE, 6)
    assert rc(_fb(capi, base, xs=ins["u_nom"] - (T * 6 - 1) * row), model=1, d=d6) == bad and b"xs overlaps u_nom" in err()


def test_well_formed_calls_get_as_far_as_the_device(lib, pkg):
    """Without a gfx950 device a well-formed call is CPMPC_ERR_NO_DEVICE, as every compute entry point."""
    if lib.cpmpc_device_count() > 0:
        pytest.skip("a GPU is present")
    capi = pkg.capi
    buf, base = _buffer()
    dv, pt = base + OFF["dyn"], base + OFF["PT"]
    inf = float("inf")
    for model, host, nx in ((0, capi.dbl_array(DYN_TEST, 9), 4), (1, capi.dbl_array(DYN_DOUBLE, 6), 6)):
        _q, qp = _host(capi, [1.0] * (nx // 2) + [0.0] * (nx // 2))
        for dtype in (capi.F32, capi.F64):
            for dt in (0.0, 0.01):
                for d, kw in ((host, {}), (None, dict(dyn=dv)), (host, dict(dyn=dv, fext=base + OFF["fext"]))):
                    forms = [_lqr(capi, base, **kw), _lqr(capi, base, K=None, **kw), _lqr(capi, base, P0=None, **kw),
                             _lqr(capi, base, PT=pt, q_host=qp, **kw), _lqr(capi, base, qf_host=qp, **kw)]
                    for a in forms:
                        assert lib.cpmpc_sim_lqr_batch(model, dtype, B, d, dt, T, C.byref(a), None) == capi.ERR_NO_DEVICE
                    a = _lqr(capi, base, xs=None, **kw)                         # T = 1 needs no checkpoints
                    assert lib.cpmpc_sim_lqr_batch(model, dtype, B, d, dt, 1, C.byref(a), None) == capi.ERR_NO_DEVICE
                    none = {name: None for name in FB_OUT}
                    forms = [_fb(capi, base, **kw), _fb(capi, base, u_limit=inf, **kw),
                             _fb(capi, base, K=None, x0_nom=None, xs_nom=None, **kw)] + \
                            [_fb(capi, base, **dict(none, **{name: base + OFF[name]}), **kw) for name in FB_OUT]
                    for a in forms:
                        assert lib.cpmpc_sim_rollout_fb_batch(model, dtype, B, d, dt, T, C.byref(a), None) == capi.ERR_NO_DEVICE
                    a = _fb(capi, base, xs_nom=None, **kw)
                    assert lib.cpmpc_sim_rollout_fb_batch(model, dtype, B, d, dt, 1, C.byref(a), None) == capi.ERR_NO_DEVICE


@pytest.mark.parametrize("which", ["lqr", "fb"])
def test_struct_layouts_match_the_c_compiler(lib, pkg, tmp_path, which):
    """The gcc probe of test_capi_no_gpu.py for cpmpc_sim_lqr and cpmpc_sim_rollout_fb."""
    cls, c_name, fields = {"lqr": (pkg.capi.SimLqr, "cpmpc_sim_lqr", LQR_FIELDS),
                           "fb": (pkg.capi.SimRolloutFb, "cpmpc_sim_rollout_fb", FB_FIELDS)}[which]
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
    assert [f for f, _ in cls._fields_] == fields
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_package_has_the_tracking_calls(pkg):
    for name in ("sim_lqr", "sim_rollout_feedback"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.BatchSimulator.rollout_feedback) and callable(pkg.ClosedLoop.tick_hold)
    assert "lower triangle" in pkg.sim_lqr.__doc__ and "no matrix is inverted" in pkg.sim_lqr.__doc__
    assert "no feedback inside a tick" in pkg.sim_rollout_feedback.__doc__
    assert "control_dt" in pkg.ClosedLoop.tick_hold.__doc__ and "u_{m-1}" in pkg.ClosedLoop.tick_hold.__doc__
