"""The fused line search of the iLQR iteration in the C-ABI without a GPU (cpmpc_sim_ilqr_search_batch), point for point as
tests/test_capi_sim_ilqr_no_gpu.py: exported, prototyped in capi.py, every refusal answers CPMPC_ERR_INVALID_ARG before any
device is needed and names the field, a well-formed call gets as far as the device, the ctypes mirror has the C compiler's
layout, and the package carries the new name and the loop's new keyword."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

from conftest import DYN_TEST, ROOT

DYN_DOUBLE = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]
B, T = 8, 3
# the documented order; `reserved` is the explicit padding behind the 32-bit trials
FIELDS = ["struct_size", "x0", "u_nom", "fext_host", "fext", "dyn", "xs_nom", "cost_nom", "kff", "K", "dV", "trials", "reserved",
          "armijo", "u_limit", "x0_ref", "xs_ref", "u_ref", "q_host", "r", "PT", "qf_host", "xs", "x_final", "us", "cost", "alpha"]
OUT = ("xs", "x_final", "us", "cost", "alpha")
IN = ("x0", "u_nom", "fext", "dyn", "xs_nom", "cost_nom", "kff", "K", "dV", "x0_ref", "xs_ref", "u_ref", "PT")


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.capi.load()


def test_symbol_exported_and_prototyped(lib, pkg):
    raw = C.CDLL(pkg.capi.LIB_PATH)
    with open(os.path.join(ROOT, "include", "cpmpc.h")) as fh:
        header = fh.read()
    name = "cpmpc_sim_ilqr_search_batch"
    assert name in pkg.capi.SYMBOLS and hasattr(raw, name)
    assert len(getattr(lib, name).argtypes) == 8
    assert "int %s(" % name in header
    doc = header[header.index("The LINE SEARCH"):header.index("} cpmpc_sim_ilqr_search;")]
    assert "for j in 0 .. trials-1 while not accepted:" in doc and "pred = dV[0] alpha + dV[1] alpha^2" in doc   # the recursion
    assert "accepted = pred < 0 and J_try - cost_nom <= armijo pred" in doc and "if not accepted: alpha = alpha / 2" in doc
    assert "xs = xs_nom, us = u_nom, x_final = xs_nom[T-1], cost = cost_nom, alpha = 0" in doc and "a COPY" in doc
    assert "SIGN CONVENTION of dV" in doc and "predicted CHANGE of J (negative: a decrease)" in doc
    assert "A FAILED PROBLEM KEEPS ITS NOMINAL BY COPY" in doc and "NOT FINITE while its nominal is finite" in doc
    assert "0 . NaN" in doc and "No other problem is affected" in doc
    assert "THE DECISIONS ARE THOSE OF THE TRIAL LADDER" in doc and "bit for bit" in doc
    assert "xs_nom is ALWAYS" in doc and "there is no x0_nom" in doc and "NO OUTPUT MAY OVERLAP AN" in doc


# distinct slices of one buffer (never dereferenced: the checks come first).  B = 8 doubles per row, T = 3, the 6-state model's
# extents at the most: PT 36 rows, xs / K 18 -- every slot is 8192 bytes = 128 rows
SLOTS = IN + OUT
OFF = {name: 8192 * i for i, name in enumerate(SLOTS)}


def _buffer():
    buf = (C.c_double * (1024 * len(SLOTS)))()
    return buf, C.addressof(buf)


def _host(capi, values):
    arr = capi.dbl_array(values, len(values))
    return arr, C.cast(arr, C.POINTER(C.c_double))


def _se(capi, base, **kw):
    a = capi.SimIlqrSearch(struct_size=C.sizeof(capi.SimIlqrSearch), r=0.01, u_limit=300.0, trials=6, armijo=1e-4,
                           **{n: base + OFF[n] for n in ("x0", "u_nom", "xs_nom", "cost_nom", "kff", "K", "dV", "x0_ref", "xs_ref")},
                           **{n: base + OFF[n] for n in OUT})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _accepted(lib, capi):
    def accepted(call):
        return lib.cpmpc_device_count() > 0 or call() == capi.ERR_NO_DEVICE
    return accepted


def test_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf, base = _buffer()
    dyn = capi.dbl_array(DYN_TEST, 9)
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    c_name = b"cpmpc_sim_ilqr_search"

    def rc(a, dt=0.01, d=dyn, model=0, dtype=capi.F64, nb=B, nt=T):
        return lib.cpmpc_sim_ilqr_search_batch(model, dtype, nb, d, dt, nt, None if a is None else C.byref(a), None)

    # ---- everything the forward call refuses
    assert rc(None) == bad and b"null" in err() and c_name in err()
    assert rc(_se(capi, base, x0=None)) == bad and b"null" in err() and b"x0" in err()
    assert rc(_se(capi, base, u_nom=None)) == bad and b"null" in err() and b"u_nom" in err()
    size = _se(capi, base).struct_size
    for s in (size - 8, size + 8, 0):
        assert rc(_se(capi, base, struct_size=s)) == bad and b"struct_size" in err() and c_name in err()
    for dt in (-0.01, float("nan"), float("inf")):
        assert rc(_se(capi, base), dt=dt) == bad and b"dt" in err()
    for nt in (0, -1):
        assert rc(_se(capi, base), nt=nt) == bad and b"T must be >= 1" in err()
    assert rc(_se(capi, base), model=7) == bad and b"model" in err()
    assert rc(_se(capi, base), dtype=5) == bad and b"dtype" in err()
    assert rc(_se(capi, base), nb=0) == bad and b"B" in err()
    assert rc(_se(capi, base), d=None) == bad and b"dyn" in err()             # neither parameter set
    for r in (0.0, -1.0, float("nan"), float("inf"), -0.0):
        assert rc(_se(capi, base, r=r)) == bad and b"r must be finite and > 0" in err(), r
    for field in ("q_host", "qf_host"):
        for q, v in ((0, -1.0), (1, float("nan")), (3, float("inf")), (2, -1e-300)):
            w = [1.0, 1.0, 1.0, 1.0]
            w[q] = v
            _arr, ptr = _host(capi, w)
            assert rc(_se(capi, base, **{field: ptr})) == bad, (field, q, v)
            assert b"%s[%d]" % (field.encode(), q) in err(), (field, q, v)
    for lim in (0.0, -1.0, float("nan")):
        assert rc(_se(capi, base, u_limit=lim)) == bad and b"u_limit" in err(), lim
    for field in ("x0_ref", "xs_ref"):                                         # a missing reference
        assert rc(_se(capi, base, **{field: None})) == bad and b"reference" in err() and field.encode() in err()
        assert rc(_se(capi, base, **{field: None}), nt=1) == bad
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(rc(None))
    assert e.value.code == bad
    accepted = _accepted(lib, capi)

    # ---- the search's own
    for field in ("xs_nom", "cost_nom", "kff", "dV"):
        assert rc(_se(capi, base, **{field: None})) == bad and b"null" in err() and field.encode() in err(), field
    assert rc(_se(capi, base, xs_nom=None), nt=1) == bad and b"xs_nom" in err()  # row T-1 is read for the copy: T = 1 too
    assert rc(_se(capi, base, xs_nom=None, K=None)) == bad and b"xs_nom" in err()
    for n in (0, -1, 33, 1 << 20):
        assert rc(_se(capi, base, trials=n)) == bad and b"trials" in err() and b"1..32" in err(), n
    for n in (1, 32):
        assert accepted(lambda: rc(_se(capi, base, trials=n)))
    for n in (1, -1, 1 << 30):                                                 # the padding behind trials is held to 0
        assert rc(_se(capi, base, reserved=n)) == bad and b"reserved" in err() and b"must be 0" in err(), n
    for v in (0.0, 1.0, -1e-4, 1.5, float("nan"), float("inf"), -float("inf")):
        assert rc(_se(capi, base, armijo=v)) == bad and b"armijo" in err(), v
    for v in (1e-300, 0.5, 1.0 - 2.0 ** -53):
        assert accepted(lambda: rc(_se(capi, base, armijo=v)))
    assert rc(_se(capi, base, **{n: None for n in OUT})) == bad and b"no output" in err()

    # ---- each output against each input
    ins = {n: base + OFF[n] for n in IN}
    optional = {n: ins[n] for n in ("fext", "dyn", "u_ref", "PT")}
    for field in OUT:
        for target, addr in ins.items():
            kw = dict(optional)
            kw[field] = addr
            assert rc(_se(capi, base, **kw)) == bad, (field, target)
            assert b"%s overlaps %s," % (field.encode(), target.encode()) in err(), (field, target)
    # the extents are the true ones
    row = B * 8
    assert rc(_se(capi, base, cost=ins["kff"] + (T - 1) * row)) == bad and b"cost overlaps kff" in err()
    assert accepted(lambda: rc(_se(capi, base, cost=ins["kff"] + T * row)))
    assert rc(_se(capi, base, alpha=ins["dV"] + row)) == bad and b"alpha overlaps dV" in err()
    assert accepted(lambda: rc(_se(capi, base, alpha=ins["dV"] + 2 * row)))
    assert rc(_se(capi, base, alpha=ins["cost_nom"])) == bad and b"alpha overlaps cost_nom" in err()
    assert accepted(lambda: rc(_se(capi, base, alpha=ins["cost_nom"] + row)))
    assert rc(_se(capi, base, us=ins["cost_nom"] - (T - 1) * row)) == bad and b"us overlaps cost_nom" in err()
    assert accepted(lambda: rc(_se(capi, base, us=ins["cost_nom"] - T * row)))
    assert rc(_se(capi, base, x_final=ins["xs_nom"] + (T * 4 - 1) * row)) == bad and b"x_final overlaps xs_nom" in err()
    assert accepted(lambda: rc(_se(capi, base, x_final=ins["xs_nom"] + T * 4 * row)))
    assert rc(_se(capi, base, xs=ins["u_nom"] - (T * 4 - 1) * row)) == bad and b"xs overlaps u_nom" in err()
    assert accepted(lambda: rc(_se(capi, base, xs=ins["u_nom"] - T * 4 * row)))
    assert rc(_se(capi, base, x_final=ins["K"] - 3 * row)) == bad and b"x_final overlaps K" in err()
    assert accepted(lambda: rc(_se(capi, base, x_final=ins["K"] - 4 * row)))
    # xs_nom is read whether or not K is given
    assert rc(_se(capi, base, K=None, xs=ins["xs_nom"])) == bad and b"xs overlaps xs_nom" in err()
    assert accepted(lambda: rc(_se(capi, base, K=None, xs=ins["K"])))           # and K, not given, overlaps nothing
    d6 = capi.dbl_array(DYN_DOUBLE, 6)                                         # the 6-state model's 18, 6 and 36 rows
    assert rc(_se(capi, base, xs=ins["u_nom"] - (T * 6 - 1) * row), model=1, d=d6) == bad and b"xs overlaps u_nom" in err()
    assert accepted(lambda: rc(_se(capi, base, xs=ins["u_nom"] - T * 6 * row), model=1, d=d6))
    assert rc(_se(capi, base, x_final=ins["x0"] - 5 * row), model=1, d=d6) == bad and b"x_final overlaps x0" in err()
    assert accepted(lambda: rc(_se(capi, base, x_final=ins["x0"] - 6 * row), model=1, d=d6))
    assert rc(_se(capi, base, PT=ins["PT"], cost=ins["PT"] + 35 * row), model=1, d=d6) == bad and b"cost overlaps PT" in err()
    assert accepted(lambda: rc(_se(capi, base, PT=ins["PT"], cost=ins["PT"] + 36 * row), model=1, d=d6))
    assert rc(_se(capi, base, alpha=ins["xs_nom"] + (T * 6 - 1) * row), model=1, d=d6) == bad and b"alpha overlaps xs_nom" in err()
    assert accepted(lambda: rc(_se(capi, base, alpha=ins["xs_nom"] + T * 6 * row), model=1, d=d6))
    # a float call's rows are half as long
    assert rc(_se(capi, base, cost=ins["kff"] + (T - 1) * row // 2), dtype=capi.F32) == bad and b"cost overlaps kff" in err()
    assert accepted(lambda: rc(_se(capi, base, cost=ins["kff"] + T * row // 2), dtype=capi.F32))


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
                    none = {name: None for name in OUT}
                    forms = [_se(capi, base, **kw), _se(capi, base, u_limit=inf, trials=1, **kw), _se(capi, base, K=None, **kw),
                             _se(capi, base, K=None, PT=pt, q_host=qp, u_ref=base + OFF["u_ref"], trials=32, armijo=0.5, **kw),
                             _se(capi, base, qf_host=qp, **kw)] + \
                            [_se(capi, base, **dict(none, **{name: base + OFF[name]}), **kw) for name in OUT]
                    for a in forms:
                        assert lib.cpmpc_sim_ilqr_search_batch(model, dtype, B, d, dt, T, C.byref(a), None) == capi.ERR_NO_DEVICE
                        assert lib.cpmpc_sim_ilqr_search_batch(model, dtype, B, d, dt, 1, C.byref(a), None) == capi.ERR_NO_DEVICE


def test_struct_layout_matches_the_c_compiler(lib, pkg, tmp_path):
    """The gcc probe of test_capi_no_gpu.py for cpmpc_sim_ilqr_search."""
    cls, c_name = pkg.capi.SimIlqrSearch, "cpmpc_sim_ilqr_search"
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
    # no hidden padding: the fields tile the struct
    assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    assert cls.trials.size == 4 and cls.reserved.offset == cls.trials.offset + 4


def test_package_has_the_search_and_the_loops_keyword(pkg):
    assert callable(pkg.sim_ilqr_search)
    doc = pkg.sim_ilqr_search.__doc__
    assert "bit for bit" in doc and "BY COPY" in doc and "0 . NaN" in doc and "larger mu" in doc
    sig = inspect.signature(pkg.sim_ilqr_search)
    assert list(sig.parameters)[:13] == ["params", "dt", "state", "u_nom", "xs_nom", "cost_nom", "kff", "K", "dV", "x_ref", "u_ref",
                                         "q", "r"]
    assert sig.parameters["trials"].default == 6 and sig.parameters["want"].default == ("xs", "us", "cost", "alpha")
    for fn in (pkg.sim_ilqr, pkg.BatchSimulator.ilqr):
        p = inspect.signature(fn).parameters["search"]
        assert p.default == "trials"                                           # the present loop, untouched
    assert "search=\"fused\"" in pkg.sim_ilqr.__doc__
    with pytest.raises(ValueError, match="search"):
        pkg.sim_ilqr(DYN_TEST, 0.01, None, None, [0.0] * 4, [1.0] * 4, 0.01, search="ladder")
    with pytest.raises(ValueError, match="32"):
        pkg.sim_ilqr(DYN_TEST, 0.01, None, None, [0.0] * 4, [1.0] * 4, 0.01, search="fused", trials=33)
    with pytest.raises(ValueError):
        pkg.sim_ilqr_search(DYN_TEST, 0.01, None, None, None, None, None, None, None, [0.0] * 4, None, [1.0] * 4, 0.01, want="J")
