"""Aggregate pushdown, the parts that need no GPU: the aggregate function classes and their compilation into the
aggregate table (term sharing, what is Unhandled and why), the ABI structs' layout, Spark's result types, and
the host/device part of cobrix_amd/csrc/cbx_aggregate.h (aggregate_build, the per-record decode, agg_accumulate,
agg_merge) run on the host (tests/native/aggregate_host.cpp) against a Python evaluator over the oracle's rows.

The contract (include/cobrix_hip.h): a field's value is the one the row filter compares -- null where the decode
makes it null, else the column's value; nulls are skipped; sums are exact.  `expected_aggregates` below states
it over decoded rows with Python ints and Decimals; the GPU tests (test_gpu_aggregate.py) use the same evaluator.
"""
from __future__ import annotations

import ctypes
import decimal
import os
import random
import shutil
import subprocess
from decimal import Decimal

import numpy as np
import pytest

from cobrix_amd import aggregate as A
from cobrix_amd import filter as F
from cobrix_amd import native as N
from cobrix_amd.plan import build_plan
from cobrix_amd.reader import ReaderParameters, parse_copybook_for
from cobrix_amd.synth import SYN200_COPYBOOK, syn200
from test_filter import (FUZZ_N, FUZZ_OPTIONS, LADDER_COPYBOOK, LADDER_SIZES, WIDE_COPYBOOK, ascii_records, fuzz_records,
                         ladder_file, ladder_params, leaf_names, narrow_file, narrow_params, py_keep, reader_plan,
                         row_value)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")
ALL_FUNCS = (A.Count, A.Min, A.Max, A.Sum)

# Fields of the test copybooks that do not take all four functions, with a word of the reason: strings and
# COMP-1 / COMP-2 take COUNT only, UTF-16 fields nothing.  (The GPU tests assert the same tables.)
STRING, FLOAT, UTF16 = "string field", "COMP-1 / COMP-2", "UTF-16"
SYN_RESTRICTED = {"NAME": STRING, "FX_RATE": FLOAT, "FILLER": "not a decoded primitive"}
FUZZ_RESTRICTED = {"S1": STRING, "S2": STRING, "A1": STRING, "F01": FLOAT, "F02": FLOAT}
ASCII_RESTRICTED = {"S1": STRING, "N1": UTF16, "N2": UTF16, "N3": UTF16}
LADDER_RESTRICTED = {f"X{s:02d}": STRING for s in LADDER_SIZES}
NARROW_RESTRICTED = {n: STRING for n in ("SEGMENT_ID", "COMPANY_ID", "COMPANY_NAME", "ADDRESS", "TAXPAYER_TYPE",
                                          "TAXPAYER_STR", "PHONE_NUMBER", "CONTACT_PERSON")}


# ---------------------------------------------------------------------------------------------
# The contract over decoded rows
# ---------------------------------------------------------------------------------------------
def _fi(plan, name):
    return plan.field_of_node[id(plan.copybook.get_field_by_name(name))]


def unscaled(v, scale: int) -> int:
    """The column's value as the integer the library aggregates: an int, or a Decimal at the column's scale."""
    if isinstance(v, Decimal):
        with decimal.localcontext() as ctx:
            ctx.prec = 120
            u = v.scaleb(scale)
            assert u == u.to_integral_value(), (v, scale)
            return int(u)
    assert isinstance(v, (int, np.integer)) and not isinstance(v, bool), (type(v), v)
    return int(v)


def expected_aggregates(cb, plan, rows, aggregates, filters=()):
    """(n_rows, values, raw): COUNT(*) of the rows the filters keep, one Spark-typed value per aggregate
    (computed with Python ints and Decimals from the rows' values), and per aggregated column
    {"count", "min", "max", "sum"} as exact unscaled ints (None without a non-null value)."""
    kept = [r for r in rows if py_keep(cb, r, filters)] if filters else rows
    values, raw = [], {}
    for ag in aggregates:
        if isinstance(ag, A.CountStar):
            values.append(len(kept))
            continue
        f = plan.fields[_fi(plan, ag.column)]
        vals = [v for v in (row_value(cb, r, ag.column) for r in kept) if v is not None]
        if isinstance(ag, A.Count):
            raw.setdefault(ag.column, {})["count"] = len(vals)
            values.append(len(vals))
            continue
        is_dec = f.out_type in (N.O_DEC64, N.O_DEC128)
        ints = [unscaled(v, f.out_scale if is_dec else 0) for v in vals]
        col = raw.setdefault(ag.column, {})
        col["count"] = len(vals)
        if isinstance(ag, A.Min):
            col["min"] = min(ints) if ints else None
            values.append(min(vals) if vals else None)
        elif isinstance(ag, A.Max):
            col["max"] = max(ints) if ints else None
            values.append(max(vals) if vals else None)
        else:
            s = sum(ints)
            col["sum"] = s if ints else None
            if not ints:
                values.append(None)
            elif not is_dec:                      # Spark: sum of int / long is a long that wraps (non-ANSI)
                values.append((s + (1 << 63)) % (1 << 64) - (1 << 63))
            elif abs(s) >= 10 ** min(38, f.out_precision + 10):   # decimal(min(38, p + 10), s) overflows to null
                values.append(None)
            else:
                with decimal.localcontext() as ctx:
                    ctx.prec = 120
                    values.append(Decimal(s).scaleb(-f.out_scale))
    return len(kept), values, raw


def field_requests(plan, names):
    """([(name, [function classes])], {name: reason}) from compile_aggregates alone: the functions every leaf
    takes, and why a leaf does not take all four."""
    requests, restricted = [], {}
    for name in names:
        funcs = []
        for fn in ALL_FUNCS:
            try:
                A.compile_aggregates(plan, [fn(name)])
                funcs.append(fn)
            except A.Unhandled as e:
                restricted[name] = str(e)
        assert funcs in ([], [A.Count], list(ALL_FUNCS)), (name, funcs)
        if funcs:
            requests.append((name, funcs))
    return requests, restricted


def check_aggregates(cb, plan, rows, agg_fn, filters=(), restricted=None, require_mixed=True):
    """Every leaf of the copybook through compile_aggregates and agg_fn(aggregates) -> AggregateResult, sixteen
    columns to a call, COUNT(*) in front:
    - the leaves that do not take all four functions are exactly `restricted` {name: word of the reason};
    - n_rows, every Spark value and every raw count / min / max / sum equal the contract over `rows`;
    - (require_mixed) among the fields at least one has 0 < count < n_rows and one has min < 0 < max, judged
      from the rows alone.  Returns the number of functions compared."""
    requests, why = field_requests(plan, leaf_names(cb))
    restricted = restricted or {}
    assert set(why) == set(restricted), (sorted(set(why) ^ set(restricted)))
    assert all(restricted[n] in why[n] for n in why), why
    compared = 0
    partial = signs = False
    for k in range(0, len(requests), N.CBX_AGG_MAX_TERMS):
        chunk = requests[k:k + N.CBX_AGG_MAX_TERMS]
        aggs = [A.CountStar()] + [fn(name) for name, funcs in chunk for fn in funcs]
        n_rows, exp_values, exp_raw = expected_aggregates(cb, plan, rows, aggs, filters)
        got = agg_fn(aggs)
        assert got.n_rows == n_rows, (got.n_rows, n_rows)
        assert len(got.raw["terms"]) == len(chunk)
        for (name, funcs), term in zip(chunk, got.raw["terms"]):
            e = exp_raw[name]
            assert term["field"] == _fi(plan, name)
            want = {"field": term["field"], "count": e["count"], "min": e.get("min"), "max": e.get("max"), "sum": e.get("sum")}
            assert term == want, (name, term, want)
            partial |= 0 < e["count"] < n_rows
            signs |= e.get("min") is not None and e["min"] < 0 < e["max"]
        bad = [(ag, g, e) for ag, g, e in zip(aggs, got.values, exp_values)
               if not ((g is None and e is None) or
                       (g is not None and e is not None and g == e and isinstance(g, Decimal) == isinstance(e, Decimal)))]
        assert not bad, bad[:3]
        compared += len(aggs)
    if require_mixed:
        assert partial and signs, (partial, signs)
    return compared


# ---------------------------------------------------------------------------------------------
# compile_aggregates
# ---------------------------------------------------------------------------------------------
def _plan(text: str, **kw):
    return build_plan(parse_copybook_for(text, ReaderParameters()), **kw)


@pytest.fixture(scope="module")
def syn_plan():
    return _plan(SYN200_COPYBOOK)


def test_functions_of_one_column_share_a_term(syn_plan):
    aggs = [A.CountStar(), A.Min("AMT-01"), A.Count("NAME"), A.Sum("AMT-01"), A.Max("BR-ID"), A.Max("AMT-01"),
            A.Count("AMT-01"), A.CountStar()]
    table, slots = A.compile_aggregates(syn_plan, aggs)
    amt, name, br = (_fi(syn_plan, n) for n in ("AMT-01", "NAME", "BR-ID"))
    assert table.n_terms == 3
    assert [(table.terms[t].field, table.terms[t].funcs) for t in range(3)] == [
        (amt, N.AGG_MIN | N.AGG_SUM | N.AGG_MAX | N.AGG_COUNT), (name, N.AGG_COUNT), (br, N.AGG_MAX)]
    assert [(s.func, s.term) for s in slots] == [(0, -1), (N.AGG_MIN, 0), (N.AGG_COUNT, 1), (N.AGG_SUM, 0), (N.AGG_MAX, 2),
                                                 (N.AGG_MAX, 0), (N.AGG_COUNT, 0), (0, -1)]
    f = syn_plan.fields[amt]
    assert (slots[1].out_type, slots[1].out_precision, slots[1].out_scale) == (f.out_type, f.out_precision, f.out_scale)
    table, slots = A.compile_aggregates(syn_plan, [A.CountStar()])
    assert table.n_terms == 0 and len(slots) == 1
    assert A.compile_aggregates(syn_plan, [])[0].n_terms == 0


def test_sixteen_column_limit(syn_plan):
    numeric = [n for n, funcs in field_requests(syn_plan, leaf_names(syn_plan.copybook))[0] if len(funcs) == 4]
    assert len(numeric) > N.CBX_AGG_MAX_TERMS == 16
    aggs = [fn(n) for n in numeric[:16] for fn in ALL_FUNCS]
    table, slots = A.compile_aggregates(syn_plan, aggs)
    assert table.n_terms == 16 and len(slots) == 64 and all(table.terms[t].funcs == 15 for t in range(16))
    with pytest.raises(A.Unhandled, match="more than 16"):
        A.compile_aggregates(syn_plan, aggs + [A.Count(numeric[16])])
    A.compile_aggregates(syn_plan, aggs + [A.Count(numeric[3]), A.CountStar()])   # no new column: fine


def test_every_unhandled_reason():
    plan = _plan(WIDE_COPYBOOK)
    for ag, word in ((A.Sum("ITEM-NO"), "OCCURS"), (A.Count("VALS"), "OCCURS"), (A.Min("RATE"), "COMP-1 / COMP-2"),
                     (A.Sum("RATE"), "COMP-1 / COMP-2"), (A.Max("NAME"), "string field"), (A.Sum("NAME"), "string field"),
                     (A.Count("NO-SUCH"), "not found"), (A.Count("ITEMS"), "primitive")):
        # all or nothing: one unpushable function returns the whole request
        with pytest.raises(A.Unhandled, match=word):
            A.compile_aggregates(plan, [A.CountStar(), A.Sum("ID"), ag])
    table, _ = A.compile_aggregates(plan, [A.Count("RATE"), A.Count("NAME")])   # COUNT needs the null test only
    assert table.n_terms == 2

    class Distinct(A.AggregateFunc):
        pass
    with pytest.raises(A.Unhandled, match="Distinct"):
        A.compile_aggregates(plan, [Distinct()])
    cb = parse_copybook_for(WIDE_COPYBOOK, ReaderParameters(variable_size_occurs=True))
    walk = build_plan(cb, walk=True, variable_size_occurs=True, string_views=1)
    with pytest.raises(A.Unhandled, match="data-dependent"):
        A.compile_aggregates(walk, [A.Count("NAME")])
    assert A.compile_aggregates(walk, [A.CountStar()])[0].n_terms == 0
    from test_decode_fuzz import ASCII_COPYBOOK
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    with pytest.raises(A.Unhandled, match="UTF-16"):
        A.compile_aggregates(aplan, [A.Count("N2")])


# ---------------------------------------------------------------------------------------------
# ABI structs
# ---------------------------------------------------------------------------------------------
AGG_STRUCTS = {"cbx_aggregate_term": N.CbxAggregateTerm, "cbx_aggregate": N.CbxAggregate,
               "cbx_aggregate_value": N.CbxAggregateValue, "cbx_aggregate_result": N.CbxAggregateResult}


def test_aggregate_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of the aggregate structs as a C compiler sees include/cobrix_hip.h, and the constants."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cobrix_hip.h"', "int main(void) {"]
    for cname, py in AGG_STRUCTS.items():
        src.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            src.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    consts = {"CBX_AGG_MAX_TERMS": N.CBX_AGG_MAX_TERMS, "CBX_AGG_COUNT": N.AGG_COUNT, "CBX_AGG_MIN": N.AGG_MIN,
              "CBX_AGG_MAX": N.AGG_MAX, "CBX_AGG_SUM": N.AGG_SUM, "CBX_ABI_VERSION": N.ABI_VERSION}
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
    seen = 0
    for line in filter(None, out):
        cname, what, val = line.split()
        seen += 1
        if cname == "const":
            assert consts[what] == int(val), what
            continue
        py = AGG_STRUCTS[cname]
        got = ctypes.sizeof(py) if what == "sizeof" else getattr(py, what).offset
        assert got == int(val), f"{cname}.{what}: ctypes {got} != C {val}"
    assert seen == len(consts) + sum(1 + len(py._fields_) for py in AGG_STRUCTS.values())
    assert N.ABI_VERSION == 25 and {"cbx_aggregate_records", "cbx_aggregate_pass_times"} <= set(N.EXPORTED_SYMBOLS)


# ---------------------------------------------------------------------------------------------
# Spark's result types
# ---------------------------------------------------------------------------------------------
def _result(out_type, p, s, count, mn, mx, sm, funcs=(N.AGG_COUNT, N.AGG_MIN, N.AGG_MAX, N.AGG_SUM)):
    slots = [A.Slot(0, -1, -1, N.O_I64, 0, 0)] + [A.Slot(fn, 0, 7, out_type, p, s) for fn in funcs]
    return A.AggregateResult(slots, count + 2, [{"field": 7, "count": count, "min": mn, "max": mx, "sum": sm}])


def test_spark_values_long_sum_wraps():
    v = 10 ** 18 - 1
    r = _result(N.O_I64, 18, 0, 10, v, v, 10 * v)
    assert 10 * v > 2 ** 63
    assert r.values == [12, 10, v, v, 10 * v - 2 ** 64] and r.values[4] < 0
    r = _result(N.O_I32, 9, 0, 3, -5, 7, -(2 ** 63) - 1)        # an int column sums to a long too
    assert r.values == [5, 3, -5, 7, 2 ** 63 - 1]
    assert _result(N.O_I64, 18, 0, 2, 1, 2, 2 ** 63 - 1).values[4] == 2 ** 63 - 1     # the largest long: no wrap
    assert all(type(x) is int for x in r.values)


def test_spark_values_decimal_sum_overflows_to_none():
    top = 10 ** 38 - 1
    r = _result(N.O_DEC128, 38, 0, 600, -top, top, 600 * top)
    assert 600 * top > 2 ** 127                                  # beyond 128 bits: the third limb's range
    assert r.values == [602, 600, Decimal(-top), Decimal(top), None]
    assert _result(N.O_DEC128, 38, 0, 1, top, top, top).values[4] == Decimal(top)
    # decimal(15, 2) sums to decimal(25, 2): |unscaled| < 10^25
    r = _result(N.O_DEC64, 15, 2, 4, -150, 99999, 10 ** 25 - 1)
    assert r.values == [6, 4, Decimal("-1.50"), Decimal("999.99"), Decimal(10 ** 25 - 1).scaleb(-2)]
    assert r.values[2].as_tuple().exponent == -2 and str(r.values[4]) == "9" * 23 + ".99"
    assert _result(N.O_DEC64, 15, 2, 4, -150, 99999, 10 ** 25).values[4] is None
    assert _result(N.O_DEC64, 15, 2, 4, -150, 99999, -(10 ** 25)).values[4] is None
    # decimal(30, 5) sums to decimal(38, 5), not decimal(40, 5)
    assert _result(N.O_DEC128, 30, 5, 2, 0, 0, 10 ** 38).values[4] is None


def test_spark_values_none_without_a_non_null_value():
    for ot, p, s in ((N.O_I32, 9, 0), (N.O_I64, 18, 0), (N.O_DEC64, 15, 2), (N.O_DEC128, 30, 5)):
        assert _result(ot, p, s, 0, None, None, None).values == [2, 0, None, None, None]


def test_merge_is_agg_merge():
    a = _result(N.O_DEC64, 15, 2, 3, -7, 10, 5)
    b = _result(N.O_DEC64, 15, 2, 0, None, None, None)
    c = _result(N.O_DEC64, 15, 2, 2, -9, 4, -8)
    ab, ac = a.merge(b), a.merge(c)
    assert ab.raw["terms"] == a.raw["terms"] == b.merge(a).raw["terms"] and ab.n_rows == 5 + 2
    assert ac.raw == {"n_rows": 9, "terms": [{"field": 7, "count": 5, "min": -9, "max": 10, "sum": -3}]}
    assert a.merge(b).merge(c).raw == a.merge(b.merge(c)).raw == c.merge(a).merge(b).raw
    assert b.merge(b).values == [4, 0, None, None, None]
    with pytest.raises(ValueError):
        a.merge(_result(N.O_DEC64, 15, 2, 1, 1, 1, 1, funcs=(N.AGG_COUNT,)))


# ---------------------------------------------------------------------------------------------
# The host/device part on the host
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    so = tmp_path_factory.mktemp("aggregate_host") / "libcbx_aggregate_host.so"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-o", str(so), os.path.join(ROOT, "tests", "native", "aggregate_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_aggregate_fixed.argtypes = [P, i32, i32, P, P, P, P, i64, i32, i32, i32, i32, P, ctypes.c_char_p, i32]
    lib.cbxh_aggregate_framed.argtypes = [P, i32, i32, P, P, P, P, i64, P, P, P, i64, i32, i32, P, ctypes.c_char_p, i32]
    return lib


def host_table(lib, plan, table: N.CbxAggregate, flt, data: bytes, stride: int, walk: bool = False, start_off: int = 0,
               n_parts: int = 5):
    """(status, cbx_aggregate_result, reason) of the host evaluator over fixed-length records."""
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    n = len(data) // stride
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    res = N.CbxAggregateResult()
    err = ctypes.create_string_buffer(256)
    rc = lib.cbxh_aggregate_fixed(ctypes.addressof(fields), len(plan.fields), int(walk),
                                  ctypes.addressof(flt) if flt is not None else None, ctypes.addressof(table),
                                  ctypes.addressof(plan.options.lut), buf.ctypes.data, n, stride, start_off, -1, n_parts,
                                  ctypes.addressof(res), err, 256)
    return rc, res, err.value.decode()


def _filter_table(plan, filters):
    if not filters:
        return None
    flt, un = F.compile_filters(plan, filters)
    assert not un, un.reasons
    return flt


def host_fixed_fn(lib, plan, data: bytes, stride: int, filters=(), start_off: int = 0, n_parts: int = 5):
    def fn(aggs):
        table, slots = A.compile_aggregates(plan, aggs)
        rc, res, err = host_table(lib, plan, table, _filter_table(plan, filters), data, stride, start_off=start_off,
                                  n_parts=n_parts)
        assert rc == 0, err
        return A.AggregateResult.from_struct(table, slots, res)
    return fn


def host_framed_fn(lib, plan, data: bytes, rec_off, rec_len, rec_seg=None, filters=(), n_parts: int = 5):
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    off = np.ascontiguousarray(rec_off, dtype=np.int64)
    ln = np.ascontiguousarray(rec_len, dtype=np.int32)
    seg = np.ascontiguousarray(rec_seg, dtype=np.int32) if rec_seg is not None else None
    buf = np.frombuffer(data, dtype=np.uint8)

    def fn(aggs):
        table, slots = A.compile_aggregates(plan, aggs)
        flt = _filter_table(plan, filters)
        res = N.CbxAggregateResult()
        err = ctypes.create_string_buffer(256)
        rc = lib.cbxh_aggregate_framed(ctypes.addressof(fields), len(plan.fields), 0,
                                       ctypes.addressof(flt) if flt is not None else None, ctypes.addressof(table),
                                       ctypes.addressof(plan.options.lut), buf.ctypes.data, len(data), off.ctypes.data,
                                       ln.ctypes.data, seg.ctypes.data if seg is not None else None, len(off), 0, n_parts,
                                       ctypes.addressof(res), err, 256)
        assert rc == 0, err.value
        return A.AggregateResult.from_struct(table, slots, res)
    return fn


def test_aggregate_build_refusals(host_shim):
    plan = _plan(WIDE_COPYBOOK)
    rec = bytes(plan.copybook.record_size)

    def status(terms, walk=False, n_terms=None, p=plan):
        t = N.CbxAggregate()
        t.n_terms = len(terms) if n_terms is None else n_terms
        for i, (field, funcs) in enumerate(terms):
            t.terms[i].field = _fi(p, field) if isinstance(field, str) else field
            t.terms[i].funcs = funcs
        rc, _, err = host_table(host_shim, p, t, None, bytes(p.copybook.record_size), p.copybook.record_size, walk)
        return rc, err

    assert status([("ID", 15), ("BIG", 15), ("RATE", N.AGG_COUNT), ("NAME", N.AGG_COUNT)])[0] == 0
    assert status([])[0] == 0                                                       # COUNT(*) alone
    for terms, word in (([("ITEM-NO", N.AGG_SUM)], "OCCURS"), ([("VALS", N.AGG_COUNT)], "OCCURS"),
                        ([("RATE", N.AGG_SUM)], "COMP-1 / COMP-2"), ([("RATE", N.AGG_COUNT | N.AGG_MIN)], "COMP-1 / COMP-2"),
                        ([("NAME", N.AGG_MAX)], "string field")):
        rc, err = status(terms)
        assert rc == N.CBX_E_UNSUPPORTED and word in err and err.startswith("cbx_aggregate: term 0: "), (terms, rc, err)
    rc, err = status([("NAME", N.AGG_COUNT)], walk=True)
    assert rc == N.CBX_E_UNSUPPORTED and "data-dependent" in err
    for terms, kw, word in (([(99, 1)], {}, "out of range"), ([(-1, 1)], {}, "out of range"),
                            ([("ID", 0)], {}, "function mask"), ([("ID", 16)], {}, "function mask"),
                            ([("ID", 1), ("BIG", 2), ("ID", 4)], {}, "repeated"),
                            ([], {"n_terms": N.CBX_AGG_MAX_TERMS + 1}, "sizes"), ([], {"n_terms": -1}, "sizes")):
        rc, err = status(terms, **kw)
        assert rc == N.CBX_E_ARGUMENT and word in err, (terms, rc, err)
    from test_decode_fuzz import ASCII_COPYBOOK
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    rc, err = status([("N1", N.AGG_COUNT)], p=aplan)
    assert rc == N.CBX_E_UNSUPPORTED and "UTF-16" in err
    gen = build_plan(parse_copybook_for(WIDE_COPYBOOK, ReaderParameters()), generate_record_id=True)
    ids = [i for i, f in enumerate(gen.fields) if f.kind in (N.K_RECORD_ID, N.K_FILE_ID)]
    assert ids
    rc, err = status([(ids[0], N.AGG_COUNT)], p=gen)
    assert rc == N.CBX_E_UNSUPPORTED and "generated" in err
    assert rec is not None


@pytest.fixture(scope="module")
def syn_rows():
    from oracle import oracle as O
    cb = parse_copybook_for(SYN200_COPYBOOK, ReaderParameters())
    data = syn200(2000, seed=5, malformed_rate=0.2).numpy().tobytes()
    return cb, data, O.rows(O.decode_fixed(cb, data), collapse_root=True)


def syn_filters(cb, rows):
    """One-term, OR-group and conjunction filters over SYN200 (literals are the data's), and none."""
    brs = sorted(v for v in (row_value(cb, r, "BR-ID") for r in rows) if v is not None)
    br = brs[len(brs) // 2]
    return {"none": [], "br_lt": [F.LessThan("BR-ID", br)], "amt_gt": [F.GreaterThan("AMT-01", Decimal("1234567.89"))],
            "or_group": [F.Or(F.EqualTo("BR-ID", br), F.IsNull("QTY-01"))],
            "three_terms": [F.GreaterThan("AMT-01", 0), F.LessThan("ZD-01", 0), F.IsNotNull("RATE-01")],
            "name_lt": [F.LessThan("NAME", "M")], "keep_none": [F.IsNull("REC-ID")]}


def test_host_syn200_every_field_with_and_without_a_filter(host_shim, syn_plan, syn_rows):
    """2,000 SYN200 records, a fifth of the numeric fields malformed: every function of every accepted field."""
    cb, data, rows = syn_rows
    for key, filters in syn_filters(cb, rows).items():
        kept = sum(py_keep(cb, r, filters) for r in rows)
        assert {"none": kept == 2000, "keep_none": kept == 0}.get(key, 0 < kept < 2000), (key, kept)
        n = check_aggregates(cb, syn_plan, rows, host_fixed_fn(host_shim, syn_plan, data, 200, filters), filters,
                             SYN_RESTRICTED, require_mixed=kept > 0)
        assert n > 100


def test_host_merge_of_a_three_way_split_equals_the_whole(host_shim, syn_plan, syn_rows):
    cb, data, rows = syn_rows
    aggs = [A.CountStar()] + [fn(n) for n in ("AMT-01", "ACCT-NO", "ZD-01", "BR-ID") for fn in ALL_FUNCS] + [A.Count("NAME")]
    filters = syn_filters(cb, rows)["or_group"]
    whole = host_fixed_fn(host_shim, syn_plan, data, 200, filters, n_parts=1)(aggs)
    cuts = [0, 200 * 701, 200 * 702, len(data)]
    a, b, c = (host_fixed_fn(host_shim, syn_plan, data[x:y], 200, filters)(aggs) for x, y in zip(cuts, cuts[1:]))
    assert a.n_rows and c.n_rows and a.n_rows + b.n_rows + c.n_rows == whole.n_rows
    for m in (a.merge(b).merge(c), a.merge(b.merge(c)), c.merge(a).merge(b)):
        assert m.raw == whole.raw and m.values == whole.values
    n_rows, values, _ = expected_aggregates(cb, syn_plan, rows, aggs, filters)
    assert whole.n_rows == n_rows and whole.values == values


@pytest.mark.parametrize("start,end", [(0, 0), (3, 2)])
@pytest.mark.parametrize("code_page,trim", FUZZ_OPTIONS)
def test_host_every_decoder_kind_ebcdic(host_shim, code_page, trim, start, end):
    """FUZZ_COPYBOOK: every zoned / binary / COMP-3 shape of the decode fuzz, COUNT of three strings and two floats."""
    from oracle import reader_oracle as RO
    from test_decode_fuzz import FUZZ_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim,
                         start_offset=start, end_offset=end)
    cb, plan = reader_plan(FUZZ_COPYBOOK, p)
    data = fuzz_records(cb, FUZZ_N, 31, start, end)
    rows = RO.fixed_len_rows(cb, data, p)
    assert len(rows) == FUZZ_N
    stride = cb.record_size + start + end
    for filters in ([], [F.IsNotNull("P05")], [F.GreaterThan("B05", 0)]):
        n = check_aggregates(cb, plan, rows, host_fixed_fn(host_shim, plan, data, stride, filters, start), filters,
                             FUZZ_RESTRICTED)
        assert n > 4 * 60


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_host_every_decoder_kind_ascii(host_shim, charset):
    from oracle import reader_oracle as RO
    from test_decode_fuzz import ASCII_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
    cb, plan = reader_plan(ASCII_COPYBOOK, p)
    data = ascii_records(cb, FUZZ_N, 32)
    rows = RO.fixed_len_rows(cb, data, p)
    assert len(rows) == FUZZ_N
    for filters in ([], [F.IsNotNull("A04")], [F.GreaterThan("A02", 0)]):
        n = check_aggregates(cb, plan, rows, host_fixed_fn(host_shim, plan, data, cb.record_size, filters), filters,
                             ASCII_RESTRICTED)
        assert n > 40


@pytest.mark.parametrize("every_length", [False, True])
@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_width_ladder_on_cut_records(host_shim, trim, every_length):
    """COMP-3 and zoned of every width beside strings of 1-47 bytes on RDW records cut at random lengths, and one
    record per length 1..L: a numeric field the record ends inside is null, a string that starts inside counts."""
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    raw, off, ln = ladder_file(seed=34, every_length=True) if every_length else ladder_file()
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == len(off)
    for filters in ([], [F.IsNotNull("P08")]):
        n = check_aggregates(cb, plan, rows, host_framed_fn(host_shim, plan, raw, off, ln, filters=filters), filters,
                             LADDER_RESTRICTED)
        assert n > 4 * 38


def test_host_segment_redefines(host_shim):
    """RDW_NARROW with its redefine map: a field of the inactive redefine is null (not counted)."""
    from cobrix_amd.synth import RDW_NARROW_COPYBOOK
    from oracle import oracle as O
    from oracle import reader_oracle as RO
    p = narrow_params()
    cb, plan = reader_plan(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(300, 21)
    off, ln = O.frame_rdw(raw)
    recs = RO.var_len_records(cb, raw, p)
    rows = RO.var_len_rows(cb, raw, p)
    groups = [g.name.upper() for g in plan.segment_groups]
    seg = np.array([groups.index(r.active_segment.upper()) if r.active_segment is not None else -1 for r in recs],
                   dtype=np.int32)
    fn = host_framed_fn(host_shim, plan, raw, off, ln, seg)
    assert check_aggregates(cb, plan, rows, fn, (), NARROW_RESTRICTED, require_mixed=False) > 6
    got = fn([A.CountStar(), A.Count("COMPANY-NAME"), A.Count("PHONE-NUMBER"), A.Count("TAXPAYER-NUM")])
    c, ph = (sum(r[g] is not None for r in rows) for g in ("STATIC_DETAILS", "CONTACTS"))
    assert got.values[:3] == [300, c, ph] and 0 < got.values[3] < c and c + ph < 300
    # the segment matters: with no active segment every field of a redefine is null
    assert host_framed_fn(host_shim, plan, raw, off, ln)([A.Count("COMPANY-NAME"), A.Count("SEGMENT-ID")]).values == [0, 300]
