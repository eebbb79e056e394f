"""The Rauch-Tung-Striebel smoother over a window in the C-ABI without a GPU (cpmpc_sim_rts_batch, cpmpc_sim_rts_work_rows),
point for point as tests/test_capi_sim_ekf_no_gpu.py: exported, prototyped in capi.py, the argument checks answer
CPMPC_ERR_INVALID_ARG before any device is needed and name the field -- the filter's rules, and work and work_rows -- a
well-formed call gets as far as the device, the ctypes mirror of cpmpc_sim_rts has the C compiler's layout, and the package
carries the new names."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import DYN_TEST, ROOT

NAME = "cpmpc_sim_rts_batch"
FIELDS = ["struct_size", "x0", "P0", "u", "fext_host", "fext", "dyn", "y", "tick_w", "w_host", "q_host", "work", "work_rows",
          "x_final", "P_final", "xs", "nis", "xs_smooth", "Ps_smooth", "x0_smooth", "P0_smooth", "ok"]
DYN_DOUBLE = [1.0, 0.1, 0.1, 0.25, 0.2, 9.81]
B, T = 8, 3
OUTPUTS = ("x_final", "P_final", "xs", "nis", "xs_smooth", "Ps_smooth", "x0_smooth", "P0_smooth", "ok")
ROWS = {0: 44, 1: 90}     # a tick's record: 2 NX + 2 NH + NX^2


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.capi.load()


def test_symbol_exported_and_prototyped(lib, pkg):
    raw = C.CDLL(pkg.capi.LIB_PATH)
    assert NAME in pkg.capi.SYMBOLS and hasattr(raw, NAME)
    assert "cpmpc_sim_rts_work_rows" in pkg.capi.SYMBOLS and hasattr(raw, "cpmpc_sim_rts_work_rows")
    assert len(getattr(lib, NAME).argtypes) == 8 and len(lib.cpmpc_sim_rts_work_rows.argtypes) == 2
    for model, rows in ROWS.items():
        for nt in (1, 3, 100):
            assert lib.cpmpc_sim_rts_work_rows(model, nt) == rows * nt
    assert lib.cpmpc_sim_rts_work_rows(7, 3) == 0 and lib.cpmpc_sim_rts_work_rows(0, 0) == 0
    assert lib.cpmpc_sim_rts_work_rows(1, 100) * 262144 * 8 == 18874368000          # the 18.9 GB of the docstring
    with open(os.path.join(ROOT, "include", "cpmpc.h")) as fh:
        header = fh.read()
    assert "int %s(" % NAME in header and "int64_t cpmpc_sim_rts_work_rows(int model, int T);" in header
    doc = header[header.index("RAUCH-TUNG-STRIEBEL SMOOTHER"):header.index("} cpmpc_sim_rts;")]
    assert "G_t   = P_t A_t^T (P-_{t+1})^-1" in doc and "P^s_t = P_t + G_t (P^s_{t+1} - P-_{t+1}) G_t^T" in doc   # the recursion
    assert "NOT\n * POSITIVE DEFINITE" in doc and "8 NX eps" in doc and "P0 = 0" in doc          # the fallback
    assert "44 T rows" in doc and "90 T" in doc and "TWO launches" in doc                       # what it costs


# distinct slices of one buffer (never dereferenced: the checks come first).  B = 8 doubles per row, T = 3, the 6-state model's
# extents at the most: Ps_smooth 144 rows, work 270 -- every slot is 32768 bytes = 512 rows
SLOTS = ("x0", "P0", "u", "fext", "dyn", "y", "tick_w", "x_final", "P_final", "xs", "nis", "xs_smooth", "Ps_smooth", "x0_smooth",
         "P0_smooth", "ok", "work")
SLOT = 32768
OFF = {name: SLOT * i for i, name in enumerate(SLOTS)}


def _rts(capi, base, **kw):
    a = capi.SimRts(struct_size=C.sizeof(capi.SimRts), x0=base + OFF["x0"], P0=base + OFF["P0"], u=base + OFF["u"],
                    y=base + OFF["y"], work=base + OFF["work"], work_rows=512, **{name: base + OFF[name] for name in OUTPUTS})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _buffer():
    buf = (C.c_double * (SLOT // 8 * len(SLOTS)))()
    return buf, C.addressof(buf)


def _host(capi, values):
    arr = capi.dbl_array(values, len(values))
    return arr, C.cast(arr, C.POINTER(C.c_double))


def test_argument_checks_need_no_device(lib, pkg):
    capi = pkg.capi
    buf, base = _buffer()
    dyn = capi.dbl_array(DYN_TEST, 9)
    bad, err = capi.ERR_INVALID_ARG, lib.cpmpc_last_error
    call = lib.cpmpc_sim_rts_batch

    def rc(a, dt=0.01, d=dyn, model=0, dtype=capi.F64, nb=B, nt=T):
        return call(model, dtype, nb, d, dt, nt, None if a is None else C.byref(a), None)

    # what every rollout call checks
    assert rc(None) == bad and b"null" in err() and b"cpmpc_sim_rts" in err()
    assert rc(_rts(capi, base, x0=None)) == bad and b"null" in err() and b"x0" in err()
    assert rc(_rts(capi, base, u=None)) == bad and b"null" in err() and b"u" in err()
    size = C.sizeof(capi.SimRts)
    for s in (size - 8, size + 8, 0):
        assert rc(_rts(capi, base, struct_size=s)) == bad and b"struct_size" in err() and b"cpmpc_sim_rts" in err()
    for dt in (-0.01, float("nan"), float("inf")):
        assert rc(_rts(capi, base), dt=dt) == bad and b"dt" in err()
    for nt in (0, -1):
        assert rc(_rts(capi, base), nt=nt) == bad and b"T must be >= 1" in err()
    assert rc(_rts(capi, base), model=7) == bad and b"model" in err()
    assert rc(_rts(capi, base), dtype=5) == bad and b"dtype" in err()
    assert rc(_rts(capi, base), nb=0) == bad and b"B" in err()
    assert rc(_rts(capi, base), d=None) == bad and b"dyn" in err()            # neither parameter set
    with pytest.raises(capi.CpmpcError) as e:
        capi.check(rc(None))
    assert e.value.code == bad

    # the call's own rules
    assert rc(_rts(capi, base, P0=None)) == bad and b"null" in err() and b"P0" in err()
    assert rc(_rts(capi, base, **{name: None for name in OUTPUTS})) == bad and b"no output" in err()
    _w1, one_measured = _host(capi, [0.0, 1e4, 0.0, 0.0])
    assert rc(_rts(capi, base, y=None)) == bad and b"without y" in err()                   # w_host NULL: ones
    assert rc(_rts(capi, base, y=None, w_host=one_measured)) == bad and b"without y" in err()
    for field in ("w_host", "q_host"):
        for q, v in ((0, -1.0), (1, float("nan")), (3, float("inf")), (2, -1e-300)):
            w = [1.0, 1.0, 1.0, 1.0]
            w[q] = v
            _arr, ptr = _host(capi, w)
            assert rc(_rts(capi, base, **{field: ptr})) == bad, (field, q, v)
            assert b"%s[%d]" % (field.encode(), q) in err(), (field, q, v)
    ins = dict(x0=base + OFF["x0"], P0=base + OFF["P0"], u=base + OFF["u"], fext=base + OFF["fext"], dyn=base + OFF["dyn"],
               y=base + OFF["y"], tick_w=base + OFF["tick_w"])
    for field in OUTPUTS:                                                      # overlapping what is only read
        for target, addr in ins.items():
            kw = dict(fext=ins["fext"], dyn=ins["dyn"], tick_w=ins["tick_w"])
            kw[field] = addr
            assert rc(_rts(capi, base, **kw)) == bad, (field, target)
            assert b"overlaps" in err() and target.encode() in err() and field.encode() in err(), (field, target)
    # the workspace: required, large enough, and over nothing
    assert rc(_rts(capi, base, work=None)) == bad and b"null" in err() and b"work" in err()
    for model, d in ((0, dyn), (1, capi.dbl_array(DYN_DOUBLE, 6))):
        need = ROWS[model] * T
        for rows in (need - 1, 0, -5):
            assert rc(_rts(capi, base, work_rows=rows), model=model, d=d) == bad, (model, rows)
            assert b"work_rows" in err() and str(need).encode() in err(), (model, rows)
    row = B * 8
    for target, addr in ins.items():                                           # work over what is read
        kw = dict(fext=ins["fext"], dyn=ins["dyn"], tick_w=ins["tick_w"], work=addr)
        assert rc(_rts(capi, base, **kw)) == bad, target
        assert b"work overlaps" in err() and target.encode() in err(), target
    for field in OUTPUTS:                                                      # work over what is written
        assert rc(_rts(capi, base, work=base + OFF[field])) == bad, field
        assert b"work overlaps" in err() and field.encode() in err(), field
    # its extent is what the helper returns, not work_rows: the last of the 132 rows (the rows next to them are accepted: the
    # well-formed calls below, which need a machine without a device -- every call HERE is refused before a device is looked at)
    assert rc(_rts(capi, base, nis=base + OFF["work"] + (44 * T - 1) * row)) == bad and b"work overlaps nis" in err()
    assert rc(_rts(capi, base, x0_smooth=base + OFF["work"] - 3 * row)) == bad and b"work overlaps x0_smooth" in err()
    # the extents are the true ones: the last row of y (tick 2, state 3) and of tick_w (tick 2), the 16th rows of P0 and
    # P_final, the 12th of xs
    assert rc(_rts(capi, base, nis=ins["y"] + (T * 4 - 1) * row)) == bad and b"nis overlaps y" in err()
    assert rc(_rts(capi, base, tick_w=ins["tick_w"], x_final=ins["tick_w"] + (T - 1) * row)) == bad
    assert b"x_final overlaps tick_w" in err()
    assert rc(_rts(capi, base, nis=ins["P0"] + 15 * row)) == bad and b"nis overlaps P0" in err()
    assert rc(_rts(capi, base, P_final=ins["x0"] - 15 * row)) == bad and b"P_final overlaps x0" in err()
    assert rc(_rts(capi, base, xs=ins["u"] - (T * 4 - 1) * row)) == bad and b"xs overlaps u" in err()
    # the smoothed outputs hold T + 1 indices
    assert rc(_rts(capi, base, xs_smooth=ins["u"] - ((T + 1) * 4 - 1) * row)) == bad and b"xs_smooth overlaps u" in err()
    assert rc(_rts(capi, base, Ps_smooth=ins["u"] - ((T + 1) * 16 - 1) * row)) == bad and b"Ps_smooth overlaps u" in err()
    assert rc(_rts(capi, base, P0_smooth=ins["x0"] - 15 * row)) == bad and b"P0_smooth overlaps x0" in err()
    # the 6-state model's 36 and 18 rows
    d6 = capi.dbl_array(DYN_DOUBLE, 6)
    assert rc(_rts(capi, base, nis=ins["P0"] + 35 * row), model=1, d=d6) == bad and b"nis overlaps P0" in err()
    assert rc(_rts(capi, base, P_final=ins["x0"] - 35 * row), model=1, d=d6) == bad and b"P_final overlaps x0" in err()
    assert rc(_rts(capi, base, xs=ins["u"] - (T * 6 - 1) * row), model=1, d=d6) == bad and b"xs overlaps u" in err()
    assert rc(_rts(capi, base, Ps_smooth=ins["u"] - ((T + 1) * 36 - 1) * row), model=1, d=d6) == bad
    assert b"Ps_smooth overlaps u" in err()


def test_a_well_formed_call_gets_as_far_as_the_device(lib, pkg):
    """Without a gfx950 device a well-formed call is CPMPC_ERR_NO_DEVICE, as every compute entry point."""
    if lib.cpmpc_device_count() > 0:
        pytest.skip("a GPU is present")
    capi = pkg.capi
    buf, base = _buffer()
    dv, tw = base + OFF["dyn"], base + OFF["tick_w"]
    none = {name: None for name in OUTPUTS}
    for model, host, nx in ((0, capi.dbl_array(DYN_TEST, 9), 4), (1, capi.dbl_array(DYN_DOUBLE, 6), 6)):
        _w, wp = _host(capi, [1e4] * (nx // 2) + [0.0] * (nx // 2))
        _q, qp = _host(capi, [0.0] * (nx // 2) + [1e-6] * (nx // 2))
        _z, zp = _host(capi, [0.0] * nx)
        for dtype in (capi.F32, capi.F64):
            for dt in (0.0, 0.01):
                for d, kw in ((host, {}), (None, dict(dyn=dv)), (host, dict(dyn=dv, tick_w=tw, w_host=wp, q_host=qp))):
                    forms = [_rts(capi, base, **kw)] + \
                            [_rts(capi, base, **dict(none, **{name: base + OFF[name]}), **kw) for name in OUTPUTS]
                    forms.append(_rts(capi, base, y=None, w_host=zp, **{k: v for k, v in kw.items() if k != "w_host"}))
                    # the extents end where they should: exactly the rows the helper returns, an output in the row behind the
                    # workspace's last, one ending in the row before its first, xs_smooth ending in the row before u
                    row = B * (4 if dtype == capi.F32 else 8)
                    need = ROWS[model] * T
                    forms.append(_rts(capi, base, work_rows=need, **kw))
                    forms.append(_rts(capi, base, nis=base + OFF["work"] + need * row, **kw))
                    forms.append(_rts(capi, base, x0_smooth=base + OFF["work"] - nx * row, **kw))
                    forms.append(_rts(capi, base, xs_smooth=base + OFF["u"] - (T + 1) * nx * row, **kw))
                    for a in forms:
                        assert lib.cpmpc_sim_rts_batch(model, dtype, B, d, dt, T, C.byref(a), None) == capi.ERR_NO_DEVICE


def test_struct_layout_matches_the_c_compiler(lib, pkg, tmp_path):
    """The gcc probe of test_capi_no_gpu.py for cpmpc_sim_rts."""
    cls, c_name = pkg.capi.SimRts, "cpmpc_sim_rts"
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


def test_package_has_the_smoother(pkg):
    assert callable(pkg.sim_rts) and callable(pkg.WindowEstimator.smooth)
    doc = pkg.sim_rts.__doc__
    assert "18.9 GB" in doc and "44 T" in doc and "90 T" in doc and "work=None allocates" in doc      # what the workspace costs
    assert "8 nx eps" in doc and "TWO launches" in doc
    assert "prior_cov" in pkg.WindowEstimator.smooth.__doc__
