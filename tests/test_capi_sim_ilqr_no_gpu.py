"""The two iLQR passes in the C-ABI without a GPU (cpmpc_sim_ilqr_backward_batch, cpmpc_sim_ilqr_forward_batch), point for point
as tests/test_capi_sim_lqr_no_gpu.py: exported, prototyped in capi.py, every refusal answers CPMPC_ERR_INVALID_ARG before any
device is needed and names the field, a well-formed call gets as far as the device, the ctypes mirrors have the C compiler's
layout, and the package carries the new names."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import DYN_TEST, ROOT

DYN_DOUBLE = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]
B, T = 8, 3
BW_FIELDS = ["struct_size", "x0", "u", "fext_host", "fext", "dyn", "xs", "x0_ref", "xs_ref", "u_ref", "q_host", "r", "PT", "qf_host",
             "mu", "u_limit", "K", "kff", "dV", "P0", "g0", "hmax"]
FW_FIELDS = ["struct_size", "x0", "u_nom", "fext_host", "fext", "dyn", "kff", "K", "x0_nom", "xs_nom", "alpha", "u_limit", "x0_ref",
             "xs_ref", "u_ref", "q_host", "r", "PT", "qf_host", "xs", "x_final", "us", "cost"]
BW_OUT = ("K", "kff", "dV", "P0", "g0", "hmax")
FW_OUT = ("xs", "x_final", "us", "cost")


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.capi.load()


def test_symbols_exported_and_prototyped(lib, pkg):
    raw = C.CDLL(pkg.capi.LIB_PATH)
    with open(os.path.join(ROOT, "include", "cpmpc.h")) as fh:
        header = fh.read()
    for name in ("cpmpc_sim_ilqr_backward_batch", "cpmpc_sim_ilqr_forward_batch"):
        assert name in pkg.capi.SYMBOLS and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == 8
        assert "int %s(" % name in header
    doc = header[header.index("THE COST of both calls"):header.index("} cpmpc_sim_ilqr_backward;")]
    assert "NO factor 1/2" in doc and "Row T-1 of xs_ref IS read" in doc and "ONLY THE LOWER TRIANGLE" in doc
    assert "k_t = clamp(u_t - h / s, +-u_limit) - u_t" in doc and "K_t = (the clamp changed u_t - h / s) ? 0" in doc  # the recursion
    assert "g   = q o e_t + r (u_t - uref_t + k_t) K_t + Acl^T (g + v k_t)" in doc and "HALF the gradient" in doc
    assert "SIGN CONVENTION" in doc and "alpha dV[0] + alpha^2 dV[1]" in doc
    assert "dt = 0" in doc and "k_t = clamp(u_t - (u_t - uref_t) r / (r + mu)) - u_t" in doc
    assert "NOT modelled" in doc and "Gauss-Newton" in doc
    doc = header[header.index("The FORWARD PASS"):header.index("} cpmpc_sim_ilqr_forward;")]
    assert "u_t = clamp(u_nom[t] + alpha kff[t] + K[t] . d, +-u_limit)" in doc and "NO feedback inside a tick" in doc
    assert "a DEVICE array, NULL: 1" in doc and "bit for bit" in doc


# distinct slices of one buffer (never dereferenced: the checks come first).  B = 8 doubles per row, T = 3, the 6-state model's
# extents at the most: PT / P0 36 rows, xs / K 18 -- every slot is 8192 bytes = 128 rows
SLOTS = ("x0", "u", "fext", "dyn", "xs_in", "x0_ref", "xs_ref", "u_ref", "PT", "mu", "K", "kff", "dV", "P0", "g0", "hmax", "x0_nom",
         "xs_nom", "alpha", "xs", "x_final", "us", "cost")
OFF = {name: 8192 * i for i, name in enumerate(SLOTS)}


def _buffer():
    buf = (C.c_double * (1024 * len(SLOTS)))()
    return buf, C.addressof(buf)


def _host(capi, values):
    arr = capi.dbl_array(values, len(values))
    return arr, C.cast(arr, C.POINTER(C.c_double))


def _bw(capi, base, **kw):
    a = capi.SimIlqrBackward(struct_size=C.sizeof(capi.SimIlqrBackward), x0=base + OFF["x0"], u=base + OFF["u"],
                             xs=base + OFF["xs_in"], x0_ref=base + OFF["x0_ref"], xs_ref=base + OFF["xs_ref"], r=0.01,
                             u_limit=float("inf"), **{n: base + OFF[n] for n in BW_OUT})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _fw(capi, base, **kw):
    a = capi.SimIlqrForward(struct_size=C.sizeof(capi.SimIlqrForward), x0=base + OFF["x0"], u_nom=base + OFF["u"],
                            kff=base + OFF["kff"], K=base + OFF["K"], x0_nom=base + OFF["x0_nom"], xs_nom=base + OFF["xs_nom"],
                            x0_ref=base + OFF["x0_ref"], xs_ref=base + OFF["xs_ref"], r=0.01, u_limit=300.0,
                            **{n: base + OFF[n] for n in FW_OUT})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _common_checks(capi, lib, call, make, base, c_name, u_field):
    """what every rollout call checks, and what the two passes share: the weights, the limit, the reference"""
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
    for r in (0.0, -1.0, float("nan"), float("inf"), -0.0):
        assert rc(make(capi, base, r=r)) == bad and b"r must be finite and > 0" in err(), r
    for field in ("q_host", "qf_host"):
        for q, v in ((0, -1.0), (1, float("nan")), (3, float("inf")), (2, -1e-300)):
            w = [1.0, 1.0, 1.0, 1.0]
            w[q] = v
            _arr, ptr = _host(capi, w)
            assert rc(make(capi, base, **{field: ptr})) == bad, (field, q, v)
            assert b"%s[%d]" % (field.encode(), q) in err(), (field, q, v)
    for lim in (0.0, -1.0, float("nan")):
        assert rc(make(capi, base, u_limit=lim)) == bad and b"u_limit" in err(), lim
    for field in ("x0_ref", "xs_ref"):                                        # a missing reference
        assert rc(make(capi, base, **{field: None})) == bad and b"reference" in err() and field.encode() in err()
        assert rc(make(capi, base, **{field: None}), nt=1) == bad              # row T-1 is the terminal target: T = 1 needs it too
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(rc(None))
    assert e.value.code == bad
    return rc


def _accepted(lib, capi):
    """-> a check that a call passes the argument checks: made only where there is no device (the pointers are not device
    memory), where it answers CPMPC_ERR_NO_DEVICE"""
    def accepted(call):
        return lib.cpmpc_device_count() > 0 or call() == capi.ERR_NO_DEVICE
    return accepted


def test_backward_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf, base = _buffer()
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    rc = _common_checks(capi, lib, lib.cpmpc_sim_ilqr_backward_batch, _bw, base, b"cpmpc_sim_ilqr_backward", "u")
    accepted = _accepted(lib, capi)

    assert rc(_bw(capi, base, **{n: None for n in BW_OUT})) == bad and b"no output" in err()
    assert rc(_bw(capi, base, xs=None)) == bad and b"xs" in err() and b"T > 1" in err()
    ins = {n: base + OFF[s] for n, s in (("x0", "x0"), ("u", "u"), ("fext", "fext"), ("dyn", "dyn"), ("xs", "xs_in"),
                                         ("x0_ref", "x0_ref"), ("xs_ref", "xs_ref"), ("u_ref", "u_ref"), ("PT", "PT"), ("mu", "mu"))}
    optional = {n: ins[n] for n in ("fext", "dyn", "u_ref", "PT", "mu")}
    for field in BW_OUT:                                                       # overlapping what is only read
        for target, addr in ins.items():
            kw = dict(optional)
            kw[field] = addr
            assert rc(_bw(capi, base, **kw)) == bad, (field, target)
            assert b"overlaps" in err() and target.encode() in err() and field.encode() in err(), (field, target)
    # the extents are the true ones
    row = B * 8
    assert rc(_bw(capi, base, g0=ins["xs_ref"] + (T * 4 - 1) * row)) == bad and b"g0 overlaps xs_ref" in err()
    assert accepted(lambda: rc(_bw(capi, base, g0=ins["xs_ref"] + T * 4 * row)))
    assert rc(_bw(capi, base, mu=ins["mu"], hmax=ins["mu"])) == bad and b"hmax overlaps mu" in err()
    assert accepted(lambda: rc(_bw(capi, base, mu=ins["mu"], hmax=ins["mu"] + row)))
    assert rc(_bw(capi, base, dV=ins["x0"] - row)) == bad and b"dV overlaps x0" in err()
    assert accepted(lambda: rc(_bw(capi, base, dV=ins["x0"] - 2 * row)))
    assert rc(_bw(capi, base, kff=ins["u"] - (T - 1) * row)) == bad and b"kff overlaps u" in err()
    assert rc(_bw(capi, base, K=ins["x0"] - (T * 4 - 1) * row)) == bad and b"K overlaps x0" in err()
    d6 = capi.dbl_array(DYN_DOUBLE, 6)                                        # the 6-state model's 36, 18 and 6 rows
    assert rc(_bw(capi, base, P0=ins["u"] - 35 * row), model=1, d=d6) == bad and b"P0 overlaps u" in err()
    assert rc(_bw(capi, base, g0=ins["x0"] - 5 * row), model=1, d=d6) == bad and b"g0 overlaps x0" in err()


def test_forward_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf, base = _buffer()
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    rc = _common_checks(capi, lib, lib.cpmpc_sim_ilqr_forward_batch, _fw, base, b"cpmpc_sim_ilqr_forward", "u_nom")
    accepted = _accepted(lib, capi)

    assert rc(_fw(capi, base, **{n: None for n in FW_OUT})) == bad and b"no output" in err()
    assert rc(_fw(capi, base, x0_nom=None)) == bad and b"x0_nom" in err()      # K without the nominal
    assert rc(_fw(capi, base, xs_nom=None)) == bad and b"xs_nom" in err()
    ins = {n: base + OFF[s] for n, s in (("x0", "x0"), ("u_nom", "u"), ("fext", "fext"), ("dyn", "dyn"), ("kff", "kff"), ("K", "K"),
                                         ("x0_nom", "x0_nom"), ("xs_nom", "xs_nom"), ("alpha", "alpha"), ("x0_ref", "x0_ref"),
                                         ("xs_ref", "xs_ref"), ("u_ref", "u_ref"), ("PT", "PT"))}
    optional = {n: ins[n] for n in ("fext", "dyn", "alpha", "u_ref", "PT")}
    for field in FW_OUT:
        for target, addr in ins.items():
            kw = dict(optional)
            kw[field] = addr
            assert rc(_fw(capi, base, **kw)) == bad, (field, target)
            assert b"overlaps" in err() and target.encode() in err() and field.encode() in err(), (field, target)
    row = B * 8
    assert rc(_fw(capi, base, cost=ins["kff"] + (T - 1) * row)) == bad and b"cost overlaps kff" in err()
    assert accepted(lambda: rc(_fw(capi, base, cost=ins["kff"] + T * row)))
    assert rc(_fw(capi, base, alpha=ins["alpha"], us=ins["alpha"] - (T - 1) * row)) == bad and b"us overlaps alpha" in err()
    assert rc(_fw(capi, base, x_final=ins["xs_ref"] + (T * 4 - 1) * row)) == bad and b"x_final overlaps xs_ref" in err()
    assert rc(_fw(capi, base, xs=ins["u_nom"] - (T * 4 - 1) * row)) == bad and b"xs overlaps u_nom" in err()
    # the nominal trajectory is read only where K is given: without K an output may lie there
    assert accepted(lambda: rc(_fw(capi, base, K=None, xs=ins["xs_nom"])))
    d6 = capi.dbl_array(DYN_DOUBLE, 6)
    assert rc(_fw(capi, base, xs=ins["u_nom"] - (T * 6 - 1) * row), model=1, d=d6) == bad and b"xs overlaps u_nom" in err()


def test_well_formed_calls_get_as_far_as_the_device(lib, pkg):
    """Without a gfx950 device a well-formed call is CPMPC_ERR_NO_DEVICE, as every compute entry point.  (With one there is
    nothing to check here: the pointers are not device memory.)"""
    if lib.cpmpc_device_count() > 0:
        return
    capi = pkg.capi
    buf, base = _buffer()
    dv, pt = base + OFF["dyn"], base + OFF["PT"]
    inf = float("inf")
    for model, host, nx in ((0, capi.dbl_array(DYN_TEST, 9), 4), (1, capi.dbl_array(DYN_DOUBLE, 6), 6)):
        _q, qp = _host(capi, [1.0] * (nx // 2) + [0.0] * (nx // 2))
        for dtype in (capi.F32, capi.F64):
            for dt in (0.0, 0.01):
                for d, kw in ((host, {}), (None, dict(dyn=dv)), (host, dict(dyn=dv, fext=base + OFF["fext"]))):
                    none = {name: None for name in BW_OUT}
                    forms = [_bw(capi, base, **kw), _bw(capi, base, PT=pt, q_host=qp, **kw), _bw(capi, base, qf_host=qp, **kw),
                             _bw(capi, base, mu=base + OFF["mu"], u_ref=base + OFF["u_ref"], u_limit=4.0, **kw)] + \
                            [_bw(capi, base, **dict(none, **{name: base + OFF[name]}), **kw) for name in BW_OUT]
                    for a in forms:
                        assert lib.cpmpc_sim_ilqr_backward_batch(model, dtype, B, d, dt, T, C.byref(a), None) == capi.ERR_NO_DEVICE
                    a = _bw(capi, base, xs=None, **kw)                          # T = 1 needs no checkpoints
                    assert lib.cpmpc_sim_ilqr_backward_batch(model, dtype, B, d, dt, 1, C.byref(a), None) == capi.ERR_NO_DEVICE
                    none = {name: None for name in FW_OUT}
                    forms = [_fw(capi, base, **kw), _fw(capi, base, u_limit=inf, alpha=base + OFF["alpha"], **kw),
                             _fw(capi, base, kff=None, K=None, x0_nom=None, xs_nom=None, **kw), _fw(capi, base, kff=None, **kw),
                             _fw(capi, base, K=None, PT=pt, u_ref=base + OFF["u_ref"], **kw)] + \
                            [_fw(capi, base, **dict(none, **{name: base + OFF[name]}), **kw) for name in FW_OUT]
                    for a in forms:
                        assert lib.cpmpc_sim_ilqr_forward_batch(model, dtype, B, d, dt, T, C.byref(a), None) == capi.ERR_NO_DEVICE
                    a = _fw(capi, base, xs_nom=None, **kw)
                    assert lib.cpmpc_sim_ilqr_forward_batch(model, dtype, B, d, dt, 1, C.byref(a), None) == capi.ERR_NO_DEVICE


@pytest.mark.parametrize("which", ["backward", "forward"])
def test_struct_layouts_match_the_c_compiler(lib, pkg, tmp_path, which):
    """The gcc probe of test_capi_no_gpu.py for cpmpc_sim_ilqr_backward and cpmpc_sim_ilqr_forward."""
    cls, c_name, fields = {"backward": (pkg.capi.SimIlqrBackward, "cpmpc_sim_ilqr_backward", BW_FIELDS),
                           "forward": (pkg.capi.SimIlqrForward, "cpmpc_sim_ilqr_forward", FW_FIELDS)}[which]
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


def test_package_has_the_ilqr_calls(pkg):
    for name in ("sim_ilqr_backward", "sim_ilqr_forward", "sim_ilqr"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.BatchSimulator.ilqr)
    assert "HALF the gradient" in pkg.sim_ilqr_backward.__doc__ and "scalar clamp" in pkg.sim_ilqr_backward.__doc__
    assert "bit for bit" in pkg.sim_ilqr_forward.__doc__
    assert "NO host synchronisation" in pkg.sim_ilqr.__doc__ and "never increases" in pkg.sim_ilqr.__doc__
