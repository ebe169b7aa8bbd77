"""Row filters pushed down to the GPU, the parts that need no GPU: the filter classes and their compilation
into the predicate table (conjunctive normal form, literal conversion, what is returned unhandled), the ABI
structs' layout, and the per-record evaluator of cobrix_amd/csrc/cbx_filter.h run on the host
(tests/native/filter_host.cpp) against a Python evaluator of the contract over the oracle's rows.

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
def row_value(cb: cbk.Copybook, row: dict, name: str):
    """The row's value of field `name` (rows with schema_policy collapse_root); None when the field or a
    group around it is null."""
    st = cb.get_field_by_name(name)
    path = []
    while st.parent is not None and st.parent.parent is not None:   # up to, not including, the 01 group
        path.append(st.name)
        st = st.parent
    v = row
    for k in reversed(path):
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
    return lib


def host_keep(lib, plan, table: N.CbxFilter, data: bytes, stride: int, walk: bool = False):
    """(status, keep flags, reason) of the host evaluator over fixed-length records."""
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    n = len(data) // stride
    keep = np.zeros(max(1, n), dtype=np.uint8)
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    err = ctypes.create_string_buffer(256)
    rc = lib.cbxh_filter_fixed(ctypes.addressof(fields), len(plan.fields), int(walk), ctypes.addressof(table),
                               ctypes.addressof(plan.options.lut), buf.ctypes.data, n, stride, 0, -1,
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
