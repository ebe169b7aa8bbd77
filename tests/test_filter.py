"""Row filters pushed down to the GPU, the parts that need no GPU: the filter classes and their compilation
into the predicate table (conjunctive normal form, literal conversion, what is returned unhandled), the ABI
structs' layout, and the per-record evaluator of cobrix_amd/csrc/cbx_filter.h run on the host
(tests/native/filter_host.cpp) against a Python evaluator of the contract over the oracle's rows: random
filters over SYN200, and a family of filters per field (`field_filters`) over every decoder kind of the decode
fuzz copybooks, a ladder of field widths on cut records, record offsets and segment redefines.

The contract (include/cobrix_hip.h): SQL three-valued logic, a row is kept only when the whole filter is
true; a field is null exactly where the decode makes it null; numerics compare as the column's value,
strings as UTF-8 bytes in unsigned byte order.  `py_keep` below states it over decoded rows; the GPU tests
(test_gpu_filter.py) use the same evaluator.
"""
from __future__ import annotations

import ctypes
import os
import random
import shutil
import subprocess
from decimal import Decimal

import numpy as np
import pytest

from cobrix_amd import copybook as cbk
from cobrix_amd import filter as F
from cobrix_amd import native as N
from cobrix_amd.plan import build_plan
from cobrix_amd.reader import ReaderParameters, parse_copybook_for
from cobrix_amd.synth import SYN200_COPYBOOK, syn200

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")

WIDE_COPYBOOK = """
       01  REC.
           05  ID            PIC 9(4) COMP.
           05  BIG           PIC S9(25)V9(5) COMP-3.
           05  CNT           PIC 9(2).
           05  ITEMS         OCCURS 3 TIMES.
              10  ITEM-NO    PIC 9(3).
           05  VALS  PIC 9(2) OCCURS 0 TO 4 TIMES DEPENDING ON CNT.
           05  RATE          COMP-1.
           05  NAME          PIC X(8).
"""


# ---------------------------------------------------------------------------------------------
# The contract over decoded rows (three-valued: True / False / None = unknown)
# ---------------------------------------------------------------------------------------------
_PATHS: dict = {}


def row_value(cb: cbk.Copybook, row: dict, name: str):
    """The row's value of field `name` (rows with schema_policy collapse_root); None when the field or a
    group around it is null."""
    hit = _PATHS.get((id(cb), name))
    if hit is None or hit[0] is not cb:   # (the lookup walks the whole copybook: once per field, not per row)
        st = cb.get_field_by_name(name)
        path = []
        while st.parent is not None and st.parent.parent is not None:   # up to, not including, the 01 group
            path.append(st.name)
            st = st.parent
        hit = _PATHS[(id(cb), name)] = (cb, tuple(reversed(path)))
    v = row
    for k in hit[1]:
        if v is None:
            return None
        v = v[k]
    return v


def _key(v):
    return v.encode("utf-8") if isinstance(v, str) else v


def py_eval(cb: cbk.Copybook, row: dict, f):
    if isinstance(f, F.And):
        a, b = py_eval(cb, row, f.left), py_eval(cb, row, f.right)
        return False if a is False or b is False else (None if a is None or b is None else True)
    if isinstance(f, F.Or):
        a, b = py_eval(cb, row, f.left), py_eval(cb, row, f.right)
        return True if a is True or b is True else (None if a is None or b is None else False)
    if isinstance(f, F.Not):
        a = py_eval(cb, row, f.child)
        return None if a is None else not a
    v = row_value(cb, row, f.attribute)
    if isinstance(f, F.IsNull):
        return v is None
    if isinstance(f, F.IsNotNull):
        return v is not None
    if v is None:
        return None
    v = _key(v)
    if isinstance(f, F.In):
        return any(v == _key(x) for x in f.values)
    x = _key(f.value)
    if isinstance(f, F.StringStartsWith):
        return v.startswith(x)
    return {F.EqualTo: v == x, F.GreaterThan: v > x, F.GreaterThanOrEqual: v >= x, F.LessThan: v < x,
            F.LessThanOrEqual: v <= x}[type(f)]


def py_keep(cb: cbk.Copybook, row: dict, filters) -> bool:
    return all(py_eval(cb, row, f) is True for f in filters)


# ---------------------------------------------------------------------------------------------
# compile_filters
# ---------------------------------------------------------------------------------------------
def _plan(text: str, **kw):
    cb = parse_copybook_for(text, ReaderParameters())
    return build_plan(cb, **kw)


def _table(t: N.CbxFilter):
    """[(group, field, op, literals)] of a compiled table."""
    out = []
    for i in range(t.n_terms):
        tm = t.terms[i]
        lits = []
        for j in range(tm.lit_begin, tm.lit_begin + tm.lit_count):
            lt = t.literals[j]
            lits.append((lt.lo, lt.hi, bytes(t.pool[lt.str_off:lt.str_off + lt.str_len])))
        out.append((tm.group, tm.field, tm.op, lits))
    return out


@pytest.fixture(scope="module")
def syn_plan():
    return _plan(SYN200_COPYBOOK)


def _fi(plan, name):
    return plan.field_of_node[id(plan.copybook.get_field_by_name(name))]


def test_cnf_or_of_ands(syn_plan):
    """(a AND b) OR (c AND d) -> (a|c)(a|d)(b|c)(b|d); two filters are AND-ed as further groups."""
    a, b = F.EqualTo("BR-ID", 1), F.GreaterThan("REC-ID", 2)
    c, d = F.LessThan("CUST-KEY", 3), F.IsNull("AMT-01")
    t, un = F.compile_filters(syn_plan, [F.Or(F.And(a, b), F.And(c, d)), F.EqualTo("NAME", "AB")])
    assert not un and t is not None
    tab = _table(t)
    fa, fb, fc, fd = (_fi(syn_plan, n) for n in ("BR-ID", "REC-ID", "CUST-KEY", "AMT-01"))
    groups = {}
    for g, fld, op, _ in tab:
        groups.setdefault(g, []).append((fld, op))
    assert [groups[g] for g in sorted(groups)] == [
        [(fa, N.OP_EQ), (fc, N.OP_LT)], [(fa, N.OP_EQ), (fd, N.OP_IS_NULL)],
        [(fb, N.OP_GT), (fc, N.OP_LT)], [(fb, N.OP_GT), (fd, N.OP_IS_NULL)],
        [(_fi(syn_plan, "NAME"), N.OP_EQ)]]
    assert [g for g, *_ in tab] == sorted(g for g, *_ in tab)          # groups never decrease
    assert tab[-1][3] == [(0, 0, b"AB")]


def test_not_pushed_to_leaves(syn_plan):
    """De Morgan: NOT(a AND (b OR c)) -> (NOT a) OR (NOT b AND NOT c) -> (a'|b')(a'|c'), ops flipped."""
    f = F.Not(F.And(F.EqualTo("BR-ID", 1), F.Or(F.LessThan("REC-ID", 5), F.StringStartsWith("NAME", "X"))))
    t, un = F.compile_filters(syn_plan, [f])
    assert not un
    ops = {}
    for g, fld, op, _ in _table(t):
        ops.setdefault(g, []).append(op)
    assert list(ops.values()) == [[N.OP_NE, N.OP_GE], [N.OP_NE, N.OP_NOT_STARTS_WITH]]
    t2, _ = F.compile_filters(syn_plan, [F.Not(F.Not(F.In("BR-ID", [1, 2])))])
    assert [(op, len(l)) for _, _, op, l in _table(t2)] == [(N.OP_IN, 2)]
    t3, _ = F.compile_filters(syn_plan, [F.Not(F.IsNull("AMT-02"))])
    assert _table(t3)[0][2] == N.OP_IS_NOT_NULL


def test_over_limit_filters_unhandled(syn_plan):
    """A filter whose normal form exceeds the table is returned whole; the others still compile."""
    big = F.Or(*[F.And(F.EqualTo("BR-ID", i), F.EqualTo("REC-ID", i)) for i in (1, 2)])
    for i in range(3, 9):   # 2^8 clauses
        big = F.Or(big, F.And(F.EqualTo("BR-ID", i), F.EqualTo("REC-ID", i)))
    small = F.EqualTo("BR-ID", 7)
    t, un = F.compile_filters(syn_plan, [big, small])
    assert un == [big] and "limit" in un.reasons[0]
    assert [(g, op) for g, _, op, _ in _table(t)] == [(0, N.OP_EQ)]
    many = F.In("BR-ID", list(range(N.CBX_FILTER_MAX_LITERALS + 1)))
    t, un = F.compile_filters(syn_plan, [many])
    assert t is None and un == [many]
    long_lit = F.EqualTo("NAME", "x" * (N.CBX_FILTER_POOL_BYTES + 1))
    assert F.compile_filters(syn_plan, [long_lit])[1] == [long_lit]
    # the table holds at least 16 terms, 64 literals and 1 KiB of literal bytes
    assert N.CBX_FILTER_MAX_TERMS >= 16 and N.CBX_FILTER_MAX_LITERALS >= 64 and N.CBX_FILTER_POOL_BYTES >= 1024
    sixteen = [F.EqualTo("BR-ID", i) for i in range(16)]
    t, un = F.compile_filters(syn_plan, sixteen)
    assert not un and t.n_terms == 16


def test_literal_conversion(syn_plan):
    one = lambda f: F.compile_filters(syn_plan, [f])   # noqa: E731
    t, un = one(F.GreaterThan("AMT-01", Decimal("1.05")))
    assert not un and _table(t)[0][3] == [(105, 0, b"")]
    t, un = one(F.EqualTo("AMT-01", 3))                 # an int at scale 2
    assert _table(t)[0][3] == [(300, 0, b"")]
    t, un = one(F.EqualTo("AMT-01", Decimal("1.005")))  # not representable at scale 2
    assert t is None and len(un) == 1 and "scale" in un.reasons[0]
    t, un = one(F.EqualTo("ACCT-NO", 2 ** 63))          # outside int64
    assert t is None and "range" in un.reasons[0]
    t, un = one(F.EqualTo("ACCT-NO", 2 ** 63 - 1))
    assert not un and _table(t)[0][3] == [(2 ** 63 - 1, 0, b"")]
    t, un = one(F.EqualTo("BR-ID", 2 ** 31))            # BR-ID is an int32 column
    assert t is None and "range" in un.reasons[0]
    t, un = one(F.LessThan("ACCT-NO", -2))              # negative: sign-extended to 128 bits
    assert _table(t)[0][3] == [(2 ** 64 - 2, 2 ** 64 - 1, b"")]
    assert one(F.EqualTo("AMT-01", 1.5))[0] is None     # a float is not an exact literal
    assert one(F.EqualTo("AMT-01", "1.5"))[0] is None
    assert one(F.EqualTo("NAME", 5))[0] is None
    assert one(F.EqualTo("AMT-01", None))[0] is None
    assert one(F.EqualTo("AMT-01", Decimal(10) ** 13))[0] is None      # decimal(15, 2) holds < 10^13
    t, un = one(F.EqualTo("NAME", "éA"))
    assert _table(t)[0][3] == [(0, 0, "éA".encode("utf-8"))]


def test_dec128_literal_sign_extended():
    plan = _plan(WIDE_COPYBOOK)
    v = Decimal("-1234567890123456789012345.00001")
    t, un = F.compile_filters(plan, [F.LessThan("BIG", v)])
    assert not un
    lo, hi, _ = _table(t)[0][3][0]
    u = -123456789012345678901234500001
    assert (hi << 64 | lo) == u % (1 << 128) and hi >> 63 == 1
    t, un = F.compile_filters(plan, [F.EqualTo("BIG", Decimal(10) ** 25)])   # decimal(30, 5) holds < 10^25
    assert t is None and "range" in un.reasons[0]


def test_unsupported_cases_unhandled_with_reason():
    plan = _plan(WIDE_COPYBOOK)
    for f, word in ((F.EqualTo("ITEM-NO", 1), "OCCURS"), (F.EqualTo("VALS", 1), "OCCURS"),
                    (F.GreaterThan("RATE", 1), "COMP-1"), (F.EqualTo("NO-SUCH", 1), "not found"),
                    (F.EqualTo("ITEMS", 1), "primitive"), (F.StringStartsWith("ID", "1"), "numeric")):
        t, un = F.compile_filters(plan, [f, F.EqualTo("ID", 4)])
        assert un == [f] and word in un.reasons[0], (f, un.reasons)
        assert t.n_terms == 1                         # the supported filter still compiles
    t, un = F.compile_filters(plan, [F.IsNull("RATE"), F.IsNotNull("RATE")])   # null tests on floats are fine
    assert not un and t.n_terms == 2
    # a record-walk plan: every field may lie at a data-dependent offset
    cb = parse_copybook_for(WIDE_COPYBOOK, ReaderParameters(variable_size_occurs=True))
    walk = build_plan(cb, walk=True, variable_size_occurs=True, string_views=1)
    t, un = F.compile_filters(walk, [F.EqualTo("NAME", "A")])
    assert t is None and "data-dependent" in un.reasons[0]

    class Custom(F.Filter):
        pass
    c = Custom()
    assert F.compile_filters(plan, [c])[1] == [c]
    assert F.compile_filters(plan, None) == (None, [])


# ---------------------------------------------------------------------------------------------
# ABI structs
# ---------------------------------------------------------------------------------------------
FILTER_STRUCTS = {"cbx_filter_literal": N.CbxFilterLiteral, "cbx_filter_term": N.CbxFilterTerm,
                  "cbx_filter": N.CbxFilter}


def test_filter_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of the filter structs as a C compiler sees include/cobrix_hip.h, and the constants."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cobrix_hip.h"', "int main(void) {"]
    for cname, py in FILTER_STRUCTS.items():
        src.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            src.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    consts = {"CBX_FILTER_MAX_TERMS": N.CBX_FILTER_MAX_TERMS, "CBX_FILTER_MAX_LITERALS": N.CBX_FILTER_MAX_LITERALS,
              "CBX_FILTER_POOL_BYTES": N.CBX_FILTER_POOL_BYTES, "CBX_OP_EQ": N.OP_EQ, "CBX_OP_NE": N.OP_NE,
              "CBX_OP_LT": N.OP_LT, "CBX_OP_LE": N.OP_LE, "CBX_OP_GT": N.OP_GT, "CBX_OP_GE": N.OP_GE,
              "CBX_OP_IN": N.OP_IN, "CBX_OP_NOT_IN": N.OP_NOT_IN, "CBX_OP_IS_NULL": N.OP_IS_NULL,
              "CBX_OP_IS_NOT_NULL": N.OP_IS_NOT_NULL, "CBX_OP_STARTS_WITH": N.OP_STARTS_WITH,
              "CBX_OP_NOT_STARTS_WITH": N.OP_NOT_STARTS_WITH}
    for c in consts:
        src.append(f'printf("const {c} %d\\n", (int){c});')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    try:
        r = subprocess.run(["gcc", "-I", os.path.dirname(HDR), "-o", str(exe), str(c)], capture_output=True, text=True)
    except OSError as e:  # pragma: no cover
        pytest.skip(f"no C compiler: {e}")
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for line in filter(None, out):
        cname, what, val = line.split()
        if cname == "const":
            assert consts[what] == int(val), what
            continue
        py = FILTER_STRUCTS[cname]
        got = ctypes.sizeof(py) if what == "sizeof" else getattr(py, what).offset
        assert got == int(val), f"{cname}.{what}: ctypes {got} != C {val}"


def test_scan_block_constant_matches_the_kernels():
    """native.FILTER_SCAN_BLOCK_RECORDS (the size the GPU tests step over) restates the scan passes' tile."""
    import re
    src = open(os.path.join(ROOT, "cobrix_amd", "csrc", "cbx_kernels.hip")).read()
    block = int(re.search(r"constexpr int kScanBlock = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int kScanItems = (\d+);", src).group(1))
    assert re.search(r"constexpr int kScanTile = kScanBlock \* kScanItems;", src)
    assert N.FILTER_SCAN_BLOCK_RECORDS == block * items * N.FILTER_TILE_RECORDS


# ---------------------------------------------------------------------------------------------
# The kernel's per-record evaluator on the host
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    so = tmp_path_factory.mktemp("filter_host") / "libcbx_filter_host.so"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-o", str(so), os.path.join(ROOT, "tests", "native", "filter_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_filter_fixed.argtypes = [P, i32, i32, P, P, P, i64, i32, i32, i32, P, ctypes.c_char_p, i32]
    lib.cbxh_filter_framed.argtypes = [P, i32, i32, P, P, P, i64, P, P, P, i64, i32, P, ctypes.c_char_p, i32]
    return lib


def host_keep(lib, plan, table: N.CbxFilter, data: bytes, stride: int, walk: bool = False, start_off: int = 0):
    """(status, keep flags, reason) of the host evaluator over fixed-length records."""
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    n = len(data) // stride
    keep = np.zeros(max(1, n), dtype=np.uint8)
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    err = ctypes.create_string_buffer(256)
    rc = lib.cbxh_filter_fixed(ctypes.addressof(fields), len(plan.fields), int(walk), ctypes.addressof(table),
                               ctypes.addressof(plan.options.lut), buf.ctypes.data, n, stride, start_off, -1,
                               keep.ctypes.data, err, 256)
    return rc, keep[:n].astype(bool), err.value.decode()


def host_keep_framed(lib, plan, table: N.CbxFilter, data: bytes, rec_off, rec_len, rec_seg=None, start_off: int = 0):
    """(status, keep flags, reason) of the host evaluator over framed records: record i is rec_len[i] bytes at
    rec_off[i] of data, its active segment rec_seg[i] (None: -1 for all)."""
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    off = np.ascontiguousarray(rec_off, dtype=np.int64)
    ln = np.ascontiguousarray(rec_len, dtype=np.int32)
    seg = np.ascontiguousarray(rec_seg, dtype=np.int32) if rec_seg is not None else None
    n = len(off)
    assert len(ln) == n and (seg is None or len(seg) == n)
    keep = np.zeros(max(1, n), dtype=np.uint8)
    buf = np.frombuffer(data, dtype=np.uint8)
    err = ctypes.create_string_buffer(256)
    rc = lib.cbxh_filter_framed(ctypes.addressof(fields), len(plan.fields), 0, ctypes.addressof(table),
                                ctypes.addressof(plan.options.lut), buf.ctypes.data, len(data), off.ctypes.data,
                                ln.ctypes.data, seg.ctypes.data if seg is not None else None, n, start_off,
                                keep.ctypes.data, err, 256)
    return rc, keep[:n].astype(bool), err.value.decode()


HOST_SEED = 6   # chosen on the CPU from the oracle's rows alone: every run below keeps and drops rows
HOST_RUNS = 60


def random_filter(rng: random.Random, cb, rows):
    """A random filter over SYN200 whose literals are decoded values of the data itself."""
    numeric = ["REC-ID", "BR-ID", "ACCT-NO", "CUST-KEY"] + [f"AMT-0{i}" for i in range(1, 9)] + \
              [f"RATE-0{i}" for i in range(1, 5)] + [f"QTY-0{i}" for i in range(1, 5)] + \
              [f"ZN-0{i}" for i in range(1, 5)] + ["ZD-01", "ZD-02"]

    def value_of(name, nonempty=False):
        while True:
            v = row_value(cb, rows[rng.randrange(len(rows))], name)
            if v is not None and not (nonempty and v == ""):
                return v

    def leaf():
        if rng.random() < 0.25:
            k = rng.randrange(5)
            if k == 0:
                return F.EqualTo("NAME", value_of("NAME"))
            if k == 1:
                return F.StringStartsWith("NAME", value_of("NAME", True)[:rng.randint(1, 2)])
            if k == 2:
                return F.In("NAME", [value_of("NAME") for _ in range(3)])
            return rng.choice([F.LessThan, F.GreaterThanOrEqual, F.GreaterThan, F.LessThanOrEqual])("NAME", value_of("NAME"))
        name = rng.choice(numeric)
        k = rng.randrange(8)
        if k == 0:
            return F.IsNull(name)
        if k == 1:
            return F.IsNotNull(name)
        if k == 2:
            return F.EqualTo(name, value_of(name))
        if k == 3:
            return F.In(name, [value_of(name) for _ in range(rng.randint(1, 4))])
        return rng.choice([F.LessThan, F.GreaterThanOrEqual, F.GreaterThan, F.LessThanOrEqual])(name, value_of(name))

    shape = rng.randrange(6)
    if shape == 0:
        return leaf()
    if shape == 1:
        return F.Not(leaf())
    if shape == 2:
        return F.Or(leaf(), leaf())
    if shape == 3:
        return F.Or(F.IsNull("FX-RATE"), F.And(leaf(), F.Not(leaf())))
    if shape == 4:
        return F.Not(F.And(leaf(), F.Or(leaf(), leaf())))
    return F.Or(F.And(leaf(), leaf()), leaf())


@pytest.fixture(scope="module")
def syn_rows():
    from oracle import oracle as O
    cb = parse_copybook_for(SYN200_COPYBOOK, ReaderParameters())
    data = syn200(2000, seed=5, malformed_rate=0.2).numpy().tobytes()
    return cb, data, O.rows(O.decode_fixed(cb, data), collapse_root=True)


def test_host_evaluator_matches_contract(host_shim, syn_plan, syn_rows):
    """2,000 SYN200 records with a fifth of the numeric fields malformed (nulls are plentiful): the keep flag
    of the kernel's evaluator equals the contract evaluated over the oracle's rows, for random filters."""
    cb, data, rows = syn_rows
    rng = random.Random(HOST_SEED)
    for run in range(HOST_RUNS):
        f = random_filter(rng, cb, rows)
        exp = np.array([py_keep(cb, r, [f]) for r in rows])
        # (the seed is chosen so that the oracle alone keeps and drops rows in every run)
        assert exp.any() and not exp.all(), (run, f)
        table, un = F.compile_filters(syn_plan, [f])
        assert not un, (f, un.reasons)
        rc, keep, err = host_keep(host_shim, syn_plan, table, data, 200)
        assert rc == 0, err
        bad = np.nonzero(keep != exp)[0]
        assert bad.size == 0, (run, f, bad[:5], rows[bad[0]])


def test_host_evaluator_rejects_what_the_c_side_does_not_cover(host_shim):
    plan = _plan(WIDE_COPYBOOK)
    rec = bytes(plan.copybook.record_size)

    def status(field_name, op, walk=False):
        t = N.CbxFilter()
        t.n_terms = 1
        t.terms[0].field, t.terms[0].op = _fi(plan, field_name), op
        if op not in (N.OP_IS_NULL, N.OP_IS_NOT_NULL):
            t.n_literals, t.terms[0].lit_count = 1, 1
        return host_keep(host_shim, plan, t, rec, len(rec), walk)

    rc, _, err = status("ITEM-NO", N.OP_EQ)
    assert rc == N.CBX_E_UNSUPPORTED and "OCCURS" in err
    rc, _, err = status("RATE", N.OP_LT)
    assert rc == N.CBX_E_UNSUPPORTED and "COMP-1" in err
    assert status("RATE", N.OP_IS_NULL)[0] == 0
    rc, _, err = status("NAME", N.OP_EQ, walk=True)
    assert rc == N.CBX_E_UNSUPPORTED and "data-dependent" in err
    assert status("ID", N.OP_STARTS_WITH)[0] == N.CBX_E_ARGUMENT
    t = N.CbxFilter()
    t.n_terms = N.CBX_FILTER_MAX_TERMS + 1
    assert host_keep(host_shim, plan, t, rec, len(rec))[0] == N.CBX_E_ARGUMENT
    t = N.CbxFilter()
    t.n_terms, t.n_literals = 2, 2
    for i, g in enumerate((1, 0)):    # groups must not decrease
        t.terms[i].field, t.terms[i].op, t.terms[i].group = _fi(plan, "ID"), N.OP_EQ, g
        t.terms[i].lit_begin, t.terms[i].lit_count = i, 1
    assert host_keep(host_shim, plan, t, rec, len(rec))[0] == N.CBX_E_ARGUMENT


# ---------------------------------------------------------------------------------------------
# Every decoder kind and edge: one family of filters per field of a copybook, against the contract
# over the oracle's rows (shared with test_gpu_filter.py, which runs the same families on the GPU)
# ---------------------------------------------------------------------------------------------
def leaf_names(cb: cbk.Copybook):
    """Names of the copybook's primitive fields, in record order."""
    def walk(g):
        for c in g.children:
            if isinstance(c, cbk.Group):
                yield from walk(c)
            else:
                yield c.name
    return list(walk(cb.ast))


def field_filters(cb: cbk.Copybook, rows, rng: random.Random):
    """(field name, filter) for every leaf of the copybook: IsNull, IsNotNull, and for four literals drawn
    from the oracle's non-null values of the field EqualTo / LessThan / GreaterThanOrEqual / Not(In([v, w]))
    (w: another drawn value); for a non-empty string literal also StringStartsWith of a prefix of 1-3
    characters and its Not.  A field the oracle never decodes to a value yields the two null tests only."""
    for name in leaf_names(cb):
        yield name, F.IsNull(name)
        yield name, F.IsNotNull(name)
        values = [v for v in (row_value(cb, r, name) for r in rows) if v is not None]
        if not values:
            continue
        for _ in range(4):
            v, w = rng.choice(values), rng.choice(values)
            yield name, F.EqualTo(name, v)
            yield name, F.LessThan(name, v)
            yield name, F.GreaterThanOrEqual(name, v)
            yield name, F.Not(F.In(name, [v, w]))
            if isinstance(v, str) and v:
                pre = F.StringStartsWith(name, v[:rng.randint(1, 3)])
                yield name, pre
                yield name, F.Not(pre)


def expected_keep(cb: cbk.Copybook, rows, filters) -> np.ndarray:
    """The contract's keep flag of every oracle row."""
    return np.array([py_keep(cb, r, filters) for r in rows], dtype=bool)


SEPARATION = 0.9   # share of the compiled filters that must keep some and drop some of the oracle's rows


def check_field_filters(cb, plan, rows, family, keep_fn, unhandled_names=(), reason="", null_tests_compile=True,
                        expected=None, separation=SEPARATION):
    """Every filter of `family` [(name, filter)] through compile_filters and keep_fn(table, filter) -> keep flags:
    - the unhandled filters are exactly those on the fields `unhandled_names` (but for their null tests, when
      null_tests_compile), each with `reason` in its reason;
    - at least SEPARATION of the compiled ones keep and drop rows (from the oracle's rows alone);
    - no record's flag differs from the contract.  Returns the number of compiled filters.
    expected: a dict that keeps the contract's flags per filter of the family between runs over the same rows.
    separation: 0 for a single row, which no filter can both keep and drop: then the compiled filters must
    keep it and drop it at least once each."""
    compiled = separated = kept_all = 0
    expected = {} if expected is None else expected
    unhandled, bad = [], []
    for name, f in family:
        table, un = F.compile_filters(plan, [f])
        if un:
            assert table is None and len(un) == 1 and un[0] is f
            unhandled.append((name, f, un.reasons[0]))
            continue
        exp = expected.get(id(f))
        if exp is None:
            exp = expected[id(f)] = expected_keep(cb, rows, [f])
        compiled += 1
        separated += bool(exp.any() and not exp.all())
        kept_all += bool(exp.all())
        keep = keep_fn(table, f)
        assert keep.shape == exp.shape, (name, f, keep.shape, exp.shape)
        for i in np.nonzero(keep != exp)[0][:2]:
            bad.append((name, f, int(i), row_value(cb, rows[i], name), bool(keep[i])))
    print(f"filters: {compiled} compiled, {separated} keep and drop rows, {len(unhandled)} unhandled, "
          f"{len(bad)} mismatches")
    want = [f for name, f in family
            if name in unhandled_names and not (null_tests_compile and isinstance(f, (F.IsNull, F.IsNotNull)))]
    assert len(unhandled) == len(want) and all(u[1] is w for u, w in zip(unhandled, want)), \
        [(u[0], u[1], u[2]) for u in unhandled if not any(u[1] is w for w in want)][:5]
    assert all(reason in u[2] for u in unhandled), [u for u in unhandled if reason not in u[2]][:3]
    assert compiled > 0 and separated >= separation * compiled, (separated, compiled)
    assert separation > 0 or 0 < kept_all < compiled, (kept_all, compiled)
    assert not bad, (len(bad), bad[:5])
    return compiled


def _host_fn(lib, plan, data, stride, start_off=0):
    def fn(table, f):
        rc, keep, err = host_keep(lib, plan, table, data, stride, start_off=start_off)
        assert rc == 0, (f, err)
        return keep
    return fn


def fuzz_records(cb: cbk.Copybook, n: int, seed: int, start: int = 0, end: int = 0) -> bytes:
    """n FUZZ_COPYBOOK records of test_decode_fuzz's generators, `start` / `end` random bytes around each."""
    from test_decode_fuzz import _random_bytes
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    leaves = list(O._iter_leaves(cb.ast))
    out = bytearray()
    for _ in range(n):
        out += bytes(rng.integers(0, 256, start, dtype=np.uint8))
        for p in leaves:
            out += _random_bytes(rng, p, p.data_size)
        out += bytes(rng.integers(0, 256, end, dtype=np.uint8))
    assert len(out) == n * (cb.record_size + start + end)
    return bytes(out)


def ascii_records(cb: cbk.Copybook, n: int, seed: int) -> bytes:
    from test_decode_fuzz import _random_ascii_bytes
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    leaves = list(O._iter_leaves(cb.ast))
    return b"".join(_random_ascii_bytes(rng, p, p.data_size, True) for _ in range(n) for p in leaves)


def reader_plan(text: str, p: ReaderParameters):
    """(copybook, plan) as the readers build them from the parameters (no Seg_Id levels, no record ids)."""
    cb = parse_copybook_for(text, p)
    plan = build_plan(cb, segment_field=p.segment_field, segment_redefine_map=p.segment_id_redefine_map or None)
    return cb, plan


FUZZ_N = 321   # five whole 64-record tiles and one record
FUZZ_OPTIONS = [("cp037", "both"), ("common", "none"), ("cp875", "left")]


@pytest.mark.parametrize("start,end", [(0, 0), (3, 2)])
@pytest.mark.parametrize("code_page,trim", FUZZ_OPTIONS)
def test_host_every_decoder_kind_ebcdic(host_shim, code_page, trim, start, end):
    """FUZZ_COPYBOOK (every zoned / binary / COMP-3 shape of the decode fuzz, three strings, two floats):
    the byte-loop numerics inside the filter, the fast-path width classes, null tests on floats."""
    from oracle import reader_oracle as RO
    from test_decode_fuzz import FUZZ_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim,
                         start_offset=start, end_offset=end)
    cb, plan = reader_plan(FUZZ_COPYBOOK, p)
    data = fuzz_records(cb, FUZZ_N, 31, start, end)
    rows = RO.fixed_len_rows(cb, data, p)
    assert len(rows) == FUZZ_N
    family = list(field_filters(cb, rows, random.Random(17)))
    n = check_field_filters(cb, plan, rows, family, _host_fn(host_shim, plan, data, cb.record_size + start + end, start),
                            unhandled_names=("F01", "F02"), reason="COMP-1 / COMP-2")
    assert n > 1000


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_host_every_decoder_kind_ascii(host_shim, charset):
    """ASCII_COPYBOOK: every CBX_K_ASCII_NUM shape, an ASCII string (ascii_lut, or the charset's table), PIC N
    fields (unhandled: UTF-16)."""
    from oracle import reader_oracle as RO
    from test_decode_fuzz import ASCII_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
    cb, plan = reader_plan(ASCII_COPYBOOK, p)
    data = ascii_records(cb, FUZZ_N, 32)
    rows = RO.fixed_len_rows(cb, data, p)
    assert len(rows) == FUZZ_N
    kinds = {plan.fields[_fi(plan, nm)].kind for nm in leaf_names(cb)}
    assert N.K_ASCII_NUM in kinds and (N.K_STRING if charset else N.K_STRING_ASCII) in kinds
    family = list(field_filters(cb, rows, random.Random(18)))
    n = check_field_filters(cb, plan, rows, family, _host_fn(host_shim, plan, data, cb.record_size),
                            unhandled_names=("N1", "N2", "N3"), reason="UTF-16", null_tests_compile=False)
    assert n > 300


# strings of every size class of flt_load_bytes (whole words, a partial last word, past kFltRegBytes = 32: the
# pointer path), COMP-3 of 1..16 bytes and zoned of 1..16 bytes beside them
LADDER_SIZES = [1, 2, 3, 5, 7, 8, 9, 12, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40, 47]
LADDER_COPYBOOK = "       01  R.\n" + "".join(
    f"           05  X{s:02d}   PIC X({s}).\n"
    f"           05  P{s:02d}   PIC S9({min(2 * (s % 16) + 1, 31)}) COMP-3.\n"
    f"           05  Z{s:02d}   PIC S9({s % 16 + 1}).\n" for s in LADDER_SIZES)
# cp037: blank (weighted), letters and digits, cent / not sign / pound (two UTF-8 bytes each), NUL HT IFS
LADDER_ALPHABET = [0x40] * 12 + [0xC1, 0xC2, 0x81, 0x82, 0xE9, 0xF0, 0xF1, 0xF9] + [0x4A, 0x5F, 0xB1] + [0x00, 0x05, 0x1C]


def ladder_file(n: int = 500, seed: int = 33, every_length: bool = False):
    """(RDW file, payload offsets, payload lengths): n records of the ladder, 30 % whole, the others cut at a
    uniform length in 1..L; every_length: L records instead, record i cut at i + 1 bytes, so every field is
    cut at every length once.  String fields are drawn from LADDER_ALPHABET.  Three quarters of the numeric
    fields are well-formed numbers over the digits 0, 1 and 9 (the alphabet alone almost never forms a wide
    COMP-3 value, and a field that is null in every row gives no filter that separates rows); the others are
    alphabet bytes too, mostly malformed."""
    cb = cbk.parse_copybook(LADDER_COPYBOOK)
    rng = random.Random(seed)
    digit = lambda: rng.choice((0, 1, 9))   # noqa: E731
    recs = []
    for i in range(cb.record_size if every_length else n):
        b = bytearray()
        for nm in leaf_names(cb):
            size = cb.get_field_by_name(nm).data_size
            if nm[0] == "X" or rng.random() < 0.25:
                b += bytes(rng.choice(LADDER_ALPHABET) for _ in range(size))
            elif nm[0] == "P":
                nib = [digit() for _ in range(2 * size - 1)] + [rng.choice((0xC, 0xD, 0xF))]
                b += bytes((nib[2 * j] << 4) | nib[2 * j + 1] for j in range(size))
            else:
                z = [0xF0 | digit() for _ in range(size)]
                z[-1] = (z[-1] & 0x0F) | rng.choice((0xC0, 0xD0, 0xF0))
                b += bytes(z)
        assert len(b) == cb.record_size
        if every_length:
            recs.append(bytes(b[:i + 1]))
        else:
            recs.append(bytes(b) if rng.random() < 0.3 else bytes(b[:rng.randint(1, len(b))]))
    raw = b"".join(bytes([0, 0, len(r) & 0xFF, len(r) >> 8]) + r for r in recs)
    off = np.cumsum([0] + [len(r) + 4 for r in recs[:-1]]) + 4
    return raw, off.astype(np.int64), np.array([len(r) for r in recs], dtype=np.int32)


def ladder_params(trim: str) -> ReaderParameters:
    return ReaderParameters(is_record_sequence=True, schema_policy="collapse_root", ebcdic_code_page="cp037",
                            string_trimming_policy=trim)


@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
def test_host_width_ladder_on_cut_records(host_shim, trim):
    """Strings of 1-47 bytes (registers up to 32 bytes, the pointer beyond), COMP-3 and zoned of every width,
    on RDW records cut at random lengths: a numeric field the record ends inside is null, a string that
    starts inside the record compares as its cut value -- through the framed entry point, head = the
    record's offset in the file as in the kernel."""
    from oracle import oracle as O
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    raw, off, ln = ladder_file()
    eo, el = O.frame_rdw(raw)
    assert np.array_equal(eo, off) and np.array_equal(el, ln)
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == len(off) == 500
    assert plan.fields[_fi(plan, "X33")].size > 32 >= plan.fields[_fi(plan, "X32")].size   # both string paths
    family = list(field_filters(cb, rows, random.Random(19)))

    def fn(table, f):
        rc, keep, err = host_keep_framed(host_shim, plan, table, raw, off, ln)
        assert rc == 0, (f, err)
        return keep
    n = check_field_filters(cb, plan, rows, family, fn)
    assert n > 950


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_width_ladder_cut_at_every_length(host_shim, trim):
    """One ladder record per length 1..L: every string field cut after each of its bytes (the partial last
    word of flt_load_bytes at every size, with and without 8 bytes in front of its end), every numeric field
    cut inside at every byte."""
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    raw, off, ln = ladder_file(seed=34, every_length=True)
    assert ln.tolist() == list(range(1, cb.record_size + 1))
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == cb.record_size
    family = list(field_filters(cb, rows, random.Random(26)))

    def fn(table, f):
        rc, keep, err = host_keep_framed(host_shim, plan, table, raw, off, ln)
        assert rc == 0, (f, err)
        return keep
    assert check_field_filters(cb, plan, rows, family, fn) > 950


NARROW_SEGMENTS = {"C": "STATIC_DETAILS", "P": "CONTACTS"}   # (transformed identifiers, as parse_options gives them)


def narrow_file(n: int, seed: int):
    """An RDW_NARROW file for filters: every second 'C' record gets a valid TAXPAYER-NUM (the generator's
    letters there have the top bit set: null for an unsigned 4-byte value), and every seventh record a
    segment id 'X' that the redefine map does not name (no active segment: both redefines are null)."""
    from cobrix_amd.synth import rdw_narrow
    d, hdr = rdw_narrow(n, seed=seed)
    raw = bytearray(d.numpy().tobytes())
    c_recs = [int(h) for h in hdr.tolist() if raw[int(h) + 4] == 0xC3]
    for k, h in enumerate(c_recs[::2]):
        raw[h + 4 + 56:h + 4 + 60] = (1000 + 37 * k).to_bytes(4, "big")
    for h in hdr.tolist()[3::7]:
        raw[int(h) + 4] = 0xE7   # cp037 'X'
    return bytes(raw)


def narrow_params() -> ReaderParameters:
    return ReaderParameters(is_record_sequence=True, schema_policy="collapse_root", segment_field="SEGMENT-ID",
                            segment_id_redefine_map=dict(NARROW_SEGMENTS))


def test_host_segment_redefines(host_shim):
    """RDW_NARROW with its redefine map: the active segment of every record passed to the evaluator (the
    oracle's, -1 where the id names no redefine); a field of the other redefine is null."""
    from cobrix_amd.synth import RDW_NARROW_COPYBOOK
    from oracle import oracle as O
    from oracle import reader_oracle as RO
    p = narrow_params()
    cb, plan = reader_plan(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(300, 21)
    off, ln = O.frame_rdw(raw)
    recs = RO.var_len_records(cb, raw, p)
    rows = RO.var_len_rows(cb, raw, p)
    assert len(recs) == len(rows) == len(off) == 300
    groups = [g.name.upper() for g in plan.segment_groups]
    seg = np.array([groups.index(r.active_segment.upper()) if r.active_segment is not None else -1 for r in recs],
                   dtype=np.int32)
    assert {-1, 0, 1} == set(seg.tolist())
    assert {plan.fields[_fi(plan, nm)].segment for nm in leaf_names(cb)} == {-1, 0, 1}
    family = list(field_filters(cb, rows, random.Random(20)))

    def fn(table, f):
        rc, keep, err = host_keep_framed(host_shim, plan, table, raw, off, ln, seg)
        assert rc == 0, (f, err)
        return keep
    n = check_field_filters(cb, plan, rows, family, fn)
    assert n > 150
    # the segment matters: with no active segment every comparison on a redefine's field is unknown
    t, _ = F.compile_filters(plan, [F.IsNotNull("COMPANY-NAME")])
    rc, keep, _ = host_keep_framed(host_shim, plan, t, raw, off, ln)
    assert rc == 0 and not keep.any()
