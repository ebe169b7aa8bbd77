"""Grouped aggregate pushdown (GROUP BY), the parts that need no GPU: compile_group_by and what it refuses, the new
ABI structs' layout, GroupedAggregateResult (Spark-typed keys, merge, rows()), and the host/device part of
cobrix_amd/csrc/cbx_group.h (group_build, the key hash, the comparison with a slot's representative record,
find-or-claim, the limb-carry add) run on the host (tests/native/group_host.cpp) against a Python evaluator.

The evaluator (`expected_groups`) takes the oracle's rows, groups them by the tuple of `row_value` of the key columns
and calls `expected_aggregates` of test_aggregate.py per group; it never uses the code under test.  The GPU tests
(test_gpu_group.py) use the same evaluator.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import struct
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
from test_aggregate import ALL_FUNCS, _filter_table, _fi, expected_aggregates
from test_filter import (FUZZ_N, FUZZ_OPTIONS, LADDER_COPYBOOK, WIDE_COPYBOOK, ascii_records, fuzz_records, ladder_file,
                         ladder_params, narrow_file, narrow_params, py_keep, reader_plan, row_value)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")


# ---------------------------------------------------------------------------------------------
# The contract over decoded rows
# ---------------------------------------------------------------------------------------------
def expected_groups(cb, plan, rows, group_by, aggregates, filters=()):
    """{key tuple: (n_rows, values, raw)}: the rows the filters keep, grouped by the key columns' values."""
    kept = [r for r in rows if py_keep(cb, r, filters)] if filters else rows
    buckets = {}
    for r in kept:
        buckets.setdefault(tuple(row_value(cb, r, k) for k in group_by), []).append(r)
    return {key: expected_aggregates(cb, plan, rs, aggregates) for key, rs in buckets.items()}


def check_groups(got: A.GroupedAggregateResult, exp: dict, aggregates):
    """The same keys (values and Python types), and per key n_rows, every Spark value (Decimal where Decimal) and
    every raw count / min / max / sum."""
    assert len(got.groups) == len(exp), (len(got.groups), len(exp))
    ekeys = {k: k for k in exp}
    assert set(got.groups) == set(exp), (sorted(set(got.groups) ^ set(exp), key=repr)[:6])
    columns = []
    for ag in aggregates:
        if not isinstance(ag, A.CountStar) and ag.column not in columns:
            columns.append(ag.column)
    for key, g in got.groups.items():
        assert all(type(a) is type(b) for a, b in zip(key, ekeys[key])), (key, ekeys[key])
        n_rows, values, raw = exp[key]
        assert g.n_rows == n_rows, (key, g.n_rows, n_rows)
        assert len(g.values) == len(values)
        for ag, a, b in zip(aggregates, g.values, values):
            assert (a is None and b is None) or (a is not None and b is not None and a == b and
                                                 isinstance(a, Decimal) == isinstance(b, Decimal)), (key, ag, a, b)
        assert len(g.raw["terms"]) == len(columns)
        for c, term in zip(columns, g.raw["terms"]):
            e = raw[c]
            want = {"field": term["field"], "count": e["count"], "min": e.get("min"), "max": e.get("max"), "sum": e.get("sum")}
            assert term == want, (key, c, term, want)
    assert got.rows() == [tuple(k) + tuple(got.groups[k].values) for k in sorted(got.groups, key=A._key_order)]
    return len(exp)


def _plan(text: str, **kw):
    return build_plan(parse_copybook_for(text, ReaderParameters()), **kw)


@pytest.fixture(scope="module")
def syn_plan():
    return _plan(SYN200_COPYBOOK)


# ---------------------------------------------------------------------------------------------
# compile_group_by
# ---------------------------------------------------------------------------------------------
def test_compile_group_by(syn_plan):
    table, keys = A.compile_group_by(syn_plan, ["BR-ID", "NAME", "AMT-01"])
    want = [_fi(syn_plan, n) for n in ("BR-ID", "NAME", "AMT-01")]
    assert table.n_keys == 3 and list(table.fields)[:3] == want and [k.field for k in keys] == want
    assert [k.is_str for k in keys] == [False, True, False]
    f = syn_plan.fields[want[2]]
    assert (keys[2].out_type, keys[2].out_precision, keys[2].out_scale) == (f.out_type, f.out_precision, f.out_scale)
    # a key may also be aggregated
    A.compile_aggregates(syn_plan, [A.Sum("BR-ID"), A.Count("NAME")])


def test_compile_group_by_every_refusal(syn_plan):
    plan = _plan(WIDE_COPYBOOK)
    for cols, word in ((["ITEM-NO"], "OCCURS"), (["RATE"], "COMP-1 / COMP-2 key"), (["NO-SUCH"], "not found"),
                       (["ITEMS"], "primitive"), (["ID", "ID"], "repeated"), ([], "1 to 4"),
                       (["ID", "BIG", "NAME", "RATE", "ID"], "1 to 4"), ([A.Sum("ID")], "plain column")):
        with pytest.raises(A.Unhandled, match=word):
            A.compile_group_by(plan, cols)
    with pytest.raises(A.Unhandled, match="1 to 4"):
        A.compile_group_by(syn_plan, ["BR-ID", "NAME", "AMT-01", "ACCT-NO", "ZD-01"])
    long_plan = _plan("       01  R.\n           05  S32  PIC X(32).\n           05  S33  PIC X(33).\n")
    assert A.compile_group_by(long_plan, ["S32"])[0].n_keys == 1
    with pytest.raises(A.Unhandled, match="longer than 32"):
        A.compile_group_by(long_plan, ["S33"])
    cb = parse_copybook_for(WIDE_COPYBOOK, ReaderParameters(variable_size_occurs=True))
    walk = build_plan(cb, walk=True, variable_size_occurs=True, string_views=1)
    with pytest.raises(A.Unhandled, match="data-dependent"):
        A.compile_group_by(walk, ["NAME"])
    from test_decode_fuzz import ASCII_COPYBOOK
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    with pytest.raises(A.Unhandled, match="UTF-16"):
        A.compile_group_by(aplan, ["N2"])
    # MIN / MAX of a DEC128 column: refused for a grouped call only
    _, slots = A.compile_aggregates(plan, [A.Count("BIG"), A.Sum("BIG")])
    A.check_grouped_functions(slots)
    for fn in (A.Min, A.Max):
        _, slots = A.compile_aggregates(plan, [A.Sum("ID"), fn("BIG")])
        with pytest.raises(A.Unhandled, match="DEC128"):
            A.check_grouped_functions(slots)


# ---------------------------------------------------------------------------------------------
# ABI structs
# ---------------------------------------------------------------------------------------------
GROUP_STRUCTS = {"cbx_group_by": N.CbxGroupBy, "cbx_group_key": N.CbxGroupKey, "cbx_group_strides": N.CbxGroupStrides,
                 "cbx_group_output": N.CbxGroupOutput, "cbx_group_header": N.CbxGroupHeader}


def test_group_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of the grouped-aggregate structs as a C compiler sees include/cobrix_hip.h, and the constants."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cobrix_hip.h"', "int main(void) {"]
    for cname, py in GROUP_STRUCTS.items():
        src.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            src.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    consts = {"CBX_GROUP_MAX_KEYS": N.CBX_GROUP_MAX_KEYS, "CBX_ABI_VERSION": N.ABI_VERSION}
    for c in consts:
        src.append(f'printf("const {c} %d\\n", (int){c});')
    src.append('printf("const64 CBX_GROUP_MAX_WORKSPACE_BYTES %lld\\n", (long long)CBX_GROUP_MAX_WORKSPACE_BYTES);')
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
        elif cname == "const64":
            assert N.CBX_GROUP_MAX_WORKSPACE_BYTES == int(val)
        else:
            py = GROUP_STRUCTS[cname]
            got = ctypes.sizeof(py) if what == "sizeof" else getattr(py, what).offset
            assert got == int(val), f"{cname}.{what}: ctypes {got} != C {val}"
    assert seen == len(consts) + 1 + sum(1 + len(py._fields_) for py in GROUP_STRUCTS.values())
    assert N.ABI_VERSION == 25 and set(N.GROUP_SYMBOLS) <= set(N.EXPORTED_SYMBOLS)
    assert set(N.GROUP_SYMBOLS) == {"cbx_group_layout", "cbx_aggregate_grouped", "cbx_group_pass_times"}


# ---------------------------------------------------------------------------------------------
# GroupedAggregateResult
# ---------------------------------------------------------------------------------------------
def _agg(n_rows, count, mn, mx, sm):
    slots = [A.Slot(0, -1, -1, N.O_I64, 0, 0)] + [A.Slot(fn, 0, 7, N.O_DEC64, 15, 2) for fn in (1, 2, 4, 8)]
    return A.AggregateResult(slots, n_rows, [{"field": 7, "count": count, "min": mn, "max": mx, "sum": sm}])


def test_key_value_mapping():
    def cell(v=0, null=0, n=0):
        return N.CbxGroupKey(v & (2 ** 64 - 1), (v >> 64) & (2 ** 64 - 1), null, n)
    i32, i64 = A.KeySlot(1, False, N.O_I32, 9, 0), A.KeySlot(1, False, N.O_I64, 18, 0)
    d64, d128 = A.KeySlot(1, False, N.O_DEC64, 15, 2), A.KeySlot(1, False, N.O_DEC128, 30, 5)
    s = A.KeySlot(1, True, N.O_STRING, 0, 0)
    assert A._key_value(i32, cell(-5), b"") == -5 and type(A._key_value(i32, cell(-5), b"")) is int
    assert A._key_value(i64, cell(-2 ** 63), b"") == -2 ** 63
    v = A._key_value(d64, cell(-150), b"")
    assert v == Decimal("-1.50") and v.as_tuple().exponent == -2
    v = A._key_value(d128, cell(-(10 ** 29)), b"")
    assert v == Decimal(-(10 ** 29)).scaleb(-5) and v.as_tuple().exponent == -5
    assert A._key_value(d64, cell(0, null=1), b"") is None and A._key_value(s, cell(0, null=1), b"xx") is None
    assert A._key_value(s, cell(n=0), b"junk") == "" and A._key_value(s, cell(n=3), "é1junk".encode()) == "é1"


def test_grouped_result_merge_and_rows_order():
    keys = [A.KeySlot(3, False, N.O_I32, 9, 0), A.KeySlot(4, True, N.O_STRING, 0, 0)]
    slots = _agg(0, 0, None, None, None).slots
    a = A.GroupedAggregateResult(keys, slots, {(1, "B"): _agg(3, 2, -7, 10, 3), (None, ""): _agg(1, 0, None, None, None),
                                               (1, None): _agg(2, 2, 1, 2, 3)})
    b = A.GroupedAggregateResult(keys, slots, {(1, "B"): _agg(2, 2, -9, 4, -5), (-4, "A"): _agg(1, 1, 5, 5, 5),
                                               (None, None): _agg(4, 0, None, None, None)})
    m = a.merge(b)
    assert set(m.groups) == {(1, "B"), (None, ""), (1, None), (-4, "A"), (None, None)} and m.n_rows == 13
    assert m.groups[(1, "B")].raw == {"n_rows": 5, "terms": [{"field": 7, "count": 4, "min": -9, "max": 10, "sum": -2}]}
    assert m.groups[(1, None)].raw == a.groups[(1, None)].raw and m.groups[(-4, "A")].raw == b.groups[(-4, "A")].raw
    assert b.merge(a).rows() == m.rows()
    # nulls first, per key column; "" is not null
    assert [r[:2] for r in m.rows()] == [(None, None), (None, ""), (-4, "A"), (1, None), (1, "B")]
    assert m.rows()[4] == (1, "B", 5, 4, Decimal("-0.09"), Decimal("0.10"), Decimal("-0.02"))
    assert set(a.groups) == {(1, "B"), (None, ""), (1, None)}            # merge leaves its sides alone
    with pytest.raises(ValueError):
        a.merge(A.GroupedAggregateResult(keys[:1], slots, {}))


# ---------------------------------------------------------------------------------------------
# The host/device part on the host
# ---------------------------------------------------------------------------------------------
def _hipcc():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    return hipcc


@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("group_host") / "libcbx_group_host.so"
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-o", str(so), os.path.join(ROOT, "tests", "native", "group_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_group_strides.argtypes = [P, i32, i32, P, P, i64, P, ctypes.c_char_p, i32]
    lib.cbxh_group_fixed.argtypes = [P, i32, i32, P, P, P, P, P, i64, i32, i32, i32, i32, i64, P, P, ctypes.c_char_p, i32]
    lib.cbxh_group_framed.argtypes = [P, i32, i32, P, P, P, P, P, i64, P, P, P, i64, i32, i32, i64, P, P, ctypes.c_char_p, i32]
    return lib


class HostError(Exception):
    def __init__(self, rc, reason):
        super().__init__(f"{rc}: {reason}")
        self.rc, self.reason = rc, reason


def host_group(lib, plan, data: bytes, group_by, aggs, filters=(), max_groups=4096, stride=0, framing=None, start_off=0,
               n_parts=3, walk=False, tables=None):
    """GroupedAggregateResult of the host evaluator over fixed-length records (stride) or framed ones (framing =
    (rec_off, rec_len, rec_seg or None)); GroupOverflow / HostError as the readers raise them."""
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    if tables is None:
        gtable, keys = A.compile_group_by(plan, group_by)
        table, slots = A.compile_aggregates(plan, aggs)
    else:
        gtable, table = tables
        keys, slots = [], []
    flt = _filter_table(plan, filters)
    err = ctypes.create_string_buffer(256)
    strides = N.CbxGroupStrides()
    rc = lib.cbxh_group_strides(ctypes.addressof(fields), len(plan.fields), int(walk), ctypes.addressof(table),
                                ctypes.addressof(gtable), max_groups, ctypes.addressof(strides), err, 256)
    if rc != 0:
        raise HostError(rc, err.value.decode())
    nt, nk = table.n_terms, gtable.n_keys
    n_rows = (ctypes.c_int64 * max_groups)()
    values = (N.CbxAggregateValue * (max_groups * nt))() if nt else None
    cells = (N.CbxGroupKey * (max_groups * nk))()
    key_bytes = (ctypes.c_uint8 * (max_groups * strides.str_stride))() if strides.str_stride else None
    out = N.CbxGroupOutput(ctypes.addressof(n_rows), ctypes.addressof(values) if nt else None, ctypes.addressof(cells),
                           ctypes.addressof(key_bytes) if key_bytes is not None else None)
    hdr = N.CbxGroupHeader()
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    head = (ctypes.addressof(fields), len(plan.fields), int(walk), ctypes.addressof(flt) if flt is not None else None,
            ctypes.addressof(table), ctypes.addressof(gtable), ctypes.addressof(plan.options.lut), buf.ctypes.data)
    tail = (n_parts, max_groups, ctypes.addressof(out), ctypes.addressof(hdr), err, 256)
    if framing is None:
        rc = lib.cbxh_group_fixed(*head, len(data) // stride, stride, start_off, -1, *tail)
    else:
        off = np.ascontiguousarray(framing[0], dtype=np.int64)
        ln = np.ascontiguousarray(framing[1], dtype=np.int32)
        seg = np.ascontiguousarray(framing[2], dtype=np.int32) if framing[2] is not None else None
        rc = lib.cbxh_group_framed(*head, len(data), off.ctypes.data, ln.ctypes.data,
                                   seg.ctypes.data if seg is not None else None, len(off), start_off, *tail)
    if rc != 0:
        raise HostError(rc, err.value.decode())
    if hdr.overflow:
        raise A.GroupOverflow(max_groups)
    res = A.GroupedAggregateResult.from_arrays(table, slots, keys, strides, hdr.n_groups, n_rows, values, cells, key_bytes)
    assert res.n_rows == hdr.n_rows
    return res


@pytest.fixture(scope="module")
def syn_rows():
    from oracle import oracle as O
    cb = parse_copybook_for(SYN200_COPYBOOK, ReaderParameters())
    data = syn200(2000, seed=5, malformed_rate=0.2).numpy().tobytes()
    return cb, data, O.rows(O.decode_fixed(cb, data), collapse_root=True)


SYN_AGGS = [A.CountStar()] + [fn(n) for n in ("AMT-01", "ACCT-NO", "BR-ID") for fn in ALL_FUNCS] + [A.Count("NAME")]


def syn_group_filters(cb, rows):
    brs = sorted(v for v in (row_value(cb, r, "BR-ID") for r in rows) if v is not None)
    return {"none": [], "br_lt": [F.LessThan("BR-ID", brs[len(brs) // 2])],
            "or_group": [F.Or(F.GreaterThan("AMT-01", Decimal("1234567.89")), F.IsNull("QTY-01"))],
            "keep_none": [F.IsNull("REC-ID")]}


@pytest.mark.parametrize("group_by", [["BR-ID"], ["BR-ID", "NAME"], ["ZD-01"]])
def test_host_syn200(host_shim, syn_plan, syn_rows, group_by):
    """2,000 SYN200 records, a fifth of the numeric fields malformed (so NULL is a key), with and without filters."""
    cb, data, rows = syn_rows
    for name, filters in syn_group_filters(cb, rows).items():
        exp = expected_groups(cb, syn_plan, rows, group_by, SYN_AGGS, filters)
        got = host_group(host_shim, syn_plan, data, group_by, SYN_AGGS, filters, stride=200)
        assert check_groups(got, exp, SYN_AGGS) == len(exp)
        if name == "none":
            assert len(exp) > 20
            # (a binary field is never malformed; a fifth of the zoned ones are)
            assert any(k[0] is None for k in exp) == (group_by == ["ZD-01"])
        if name == "keep_none":
            assert not exp


def test_host_three_way_split_merged_equals_the_whole(host_shim, syn_plan, syn_rows):
    cb, data, rows = syn_rows
    filters = syn_group_filters(cb, rows)["or_group"]
    whole = host_group(host_shim, syn_plan, data, ["BR-ID", "NAME"], SYN_AGGS, filters, stride=200, n_parts=1)
    cuts = [0, 200 * 701, 200 * 702, len(data)]
    a, b, c = (host_group(host_shim, syn_plan, data[x:y], ["BR-ID", "NAME"], SYN_AGGS, filters, stride=200)
               for x, y in zip(cuts, cuts[1:]))
    for m in (a.merge(b).merge(c), c.merge(a.merge(b))):
        assert m.rows() == whole.rows() and {k: g.raw for k, g in m.groups.items()} == {k: g.raw for k, g in whole.groups.items()}
    check_groups(whole, expected_groups(cb, syn_plan, rows, ["BR-ID", "NAME"], SYN_AGGS, filters), SYN_AGGS)


def test_host_max_groups_exact_and_one_less(host_shim, syn_plan, syn_rows):
    cb, data, rows = syn_rows
    exp = expected_groups(cb, syn_plan, rows, ["BR-ID"], [A.CountStar()])
    d = len(exp)
    for parts in (1, 3):
        got = host_group(host_shim, syn_plan, data, ["BR-ID"], [A.CountStar()], max_groups=d, stride=200, n_parts=parts)
        assert check_groups(got, exp, [A.CountStar()]) == d
    with pytest.raises(A.GroupOverflow, match="max_groups"):
        host_group(host_shim, syn_plan, data, ["BR-ID"], [A.CountStar()], max_groups=d - 1, stride=200, n_parts=1)
    with pytest.raises(A.GroupOverflow):
        host_group(host_shim, syn_plan, data, ["BR-ID"], [A.CountStar()], max_groups=1, stride=200)


def _key_candidates(plan, cb):
    """The leaves compile_group_by accepts, by decoder kind."""
    from test_filter import leaf_names
    by_kind = {}
    for name in leaf_names(cb):
        try:
            t, _ = A.compile_group_by(plan, [name])
        except A.Unhandled:
            continue
        by_kind.setdefault((plan.fields[t.fields[0]].kind, plan.fields[t.fields[0]].out_type), []).append(name)
    return by_kind


@pytest.mark.parametrize("start,end", [(0, 0), (3, 2)])
@pytest.mark.parametrize("code_page,trim", FUZZ_OPTIONS)
def test_host_every_decoder_kind_ebcdic(host_shim, code_page, trim, start, end):
    """FUZZ_COPYBOOK: one key of every accepted decoder kind and output type (and every accepted field in pairs)."""
    from oracle import reader_oracle as RO
    from test_decode_fuzz import FUZZ_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim,
                         start_offset=start, end_offset=end)
    cb, plan = reader_plan(FUZZ_COPYBOOK, p)
    data = fuzz_records(cb, FUZZ_N, 31, start, end)
    rows = RO.fixed_len_rows(cb, data, p)
    stride = cb.record_size + start + end
    by_kind = _key_candidates(plan, cb)
    assert {k for k, _ in by_kind} >= {N.K_STRING, N.K_BCD, N.K_BINARY, N.K_ZONED}
    aggs = [A.CountStar(), A.Sum("P05"), A.Count("B05"), A.Min("B05")]
    for filters in ([], [F.IsNotNull("P05")]):
        for names in by_kind.values():
            for group_by in ([names[0]], names[-2:]):
                exp = expected_groups(cb, plan, rows, group_by, aggs, filters)
                got = host_group(host_shim, plan, data, group_by, aggs, filters, stride=stride, start_off=start)
                check_groups(got, exp, aggs)


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_host_every_decoder_kind_ascii(host_shim, charset):
    from oracle import reader_oracle as RO
    from test_decode_fuzz import ASCII_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
    cb, plan = reader_plan(ASCII_COPYBOOK, p)
    data = ascii_records(cb, FUZZ_N, 32)
    rows = RO.fixed_len_rows(cb, data, p)
    by_kind = _key_candidates(plan, cb)
    # (with a charset the strings go through the code-page table as K_STRING)
    assert {k for k, _ in by_kind} >= {N.K_STRING if charset else N.K_STRING_ASCII, N.K_ASCII_NUM}
    aggs = [A.CountStar(), A.Sum("A02"), A.Count("A04")]
    for filters in ([], [F.IsNotNull("A04")]):
        for names in by_kind.values():
            exp = expected_groups(cb, plan, rows, names[:1], aggs, filters)
            check_groups(host_group(host_shim, plan, data, names[:1], aggs, filters, stride=cb.record_size), exp, aggs)


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_width_ladder_cut_at_every_length(host_shim, trim):
    """One record per length: a string key that starts past the record's end is NULL, one that starts at its end is
    "" -- two groups; a numeric key the record ends inside is NULL."""
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    raw, off, ln = ladder_file(seed=34, every_length=True)
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == len(off)
    aggs = [A.CountStar(), A.Count("P08"), A.Sum("P08")]
    for group_by in (["X05"], ["X32"], ["P05"], ["Z07"], ["X03", "P03"]):
        for filters in ([], [F.IsNotNull("X02")]):
            exp = expected_groups(cb, plan, rows, group_by, aggs, filters)
            got = host_group(host_shim, plan, raw, group_by, aggs, filters, framing=(off, ln, None))
            check_groups(got, exp, aggs)
            if not filters and len(group_by) == 1:
                assert (None,) in exp
    exp = expected_groups(cb, plan, rows, ["X05"], aggs)
    assert (None,) in exp and ("",) in exp


def test_host_segment_redefines(host_shim):
    """RDW_NARROW with its redefine map: a key in the inactive redefine is NULL."""
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
    aggs = [A.CountStar(), A.Count("TAXPAYER-NUM"), A.Sum("TAXPAYER-NUM"), A.Count("PHONE-NUMBER")]
    for group_by in (["SEGMENT-ID"], ["TAXPAYER-TYPE"], ["SEGMENT-ID", "TAXPAYER-TYPE"], ["TAXPAYER-NUM"]):
        for filters in ([], [F.IsNotNull("COMPANY-NAME")]):
            exp = expected_groups(cb, plan, rows, group_by, aggs, filters)
            check_groups(host_group(host_shim, plan, raw, group_by, aggs, filters, framing=(off, ln, seg)), exp, aggs)
    exp = expected_groups(cb, plan, rows, ["TAXPAYER-TYPE"], aggs)
    assert (None,) in exp and len(exp) >= 2


# ---------------------------------------------------------------------------------------------
# Equal value, different bytes
# ---------------------------------------------------------------------------------------------
EQUAL_COPYBOOK = """
       01  R.
           05  KB    PIC S9(4) COMP.
           05  KP    PIC S9(20) COMP-3.
           05  KZ    PIC S9(3).
           05  KX4   PIC X(4).
           05  KX3   PIC X(3).
           05  VP    PIC S9(5) COMP-3.
           05  VZ    PIC S9(3).
"""
EQUAL_SIZE = 2 + 11 + 3 + 4 + 3 + 3 + 3


def _bcd(v: int, size: int, sign=None) -> bytes:
    nib = [int(c) for c in str(abs(v)).rjust(2 * size - 1, "0")] + [sign if sign is not None else (0xD if v < 0 else 0xC)]
    return bytes((nib[2 * j] << 4) | nib[2 * j + 1] for j in range(size))


def _zoned(digits: str, zone: int) -> bytes:
    b = bytearray(0xF0 | int(c) for c in digits)
    b[-1] = (zone << 4) | int(digits[-1])
    return bytes(b)


def lut_twins(plan):
    """Two different source bytes with one code-page image (placed in the middle of a string, where no trim reaches)."""
    seen = {}
    for b in range(256):
        e = plan.options.lut[b]
        if e in seen and b not in (0x40, 0xC1, 0xC2) and seen[e] not in (0x40, 0xC1, 0xC2):
            return seen[e], b
        seen.setdefault(e, b)
    raise AssertionError("the code page maps no two bytes to one character")


def equal_records(plan):
    """(data, the number of distinct values per key column): every record spells its keys differently from the
    others of its group -- the three sign nibbles of a COMP-3 zero, two overpunch spellings of +12 and of -12 beside a
    malformed one, padding-only differences, two source bytes with one image."""
    t1, t2 = lut_twins(plan)
    A_, B_, SP = 0xC1, 0xC2, 0x40
    kx4 = [bytes([A_, SP, SP, SP]), bytes([A_, SP, SP, SP]), bytes([SP, A_, SP, SP]), bytes([SP, SP, SP, A_]),
           bytes([A_, t1, B_, SP]), bytes([A_, t2, B_, SP]), bytes([SP, SP, SP, SP]), bytes([A_, SP, B_, SP])]
    kx3 = [bytes([A_, SP, SP]), bytes([SP, A_, SP]), bytes([SP, SP, A_]), bytes([SP, SP, SP])]
    kp = [_bcd(0, 11, 0xC), _bcd(0, 11, 0xD), _bcd(0, 11, 0xF), _bcd(10 ** 19, 11), _bcd(-(10 ** 19), 11), b"\xAA" * 11]
    kz = [_zoned("012", 0xC), _zoned("012", 0xF), _zoned("012", 0xD), _zoned("000", 0xC), _zoned("000", 0xD), b"\x40\x40\x40"]
    recs = []
    for i in range(8 * 4 * 6):
        kb = (i % 3 - 1).to_bytes(2, "big", signed=True)
        vp = _bcd((i * 37) % 1999 - 999, 3, 0xF if i % 5 == 0 and (i * 37) % 1999 >= 999 else None)
        vz = _zoned(f"{(i * 7) % 1000:03d}", (0xC, 0xD, 0xF)[i % 3])
        recs.append(kb + kp[i % 6] + kz[(i // 6) % 6] + kx4[i % 8] + kx3[(i // 8) % 4] + vp + vz)
    assert all(len(r) == EQUAL_SIZE for r in recs)
    return b"".join(recs)


def equal_expected_counts(trim: str) -> dict:
    """Distinct values per key column, worked out by hand from equal_records (the twins' image is one character)."""
    #  none:  "A   ", " A  ", "   A", "A?B ", "    ", "A B "        (the twins' image may equal the space: see the test)
    #  left:  "A   ", "A  ", "A", "A?B ", "", "A B "
    #  right: "A", " A", "   A", "A?B", "", "A B"
    #  both:  "A", "A?B", "", "A B"
    kx4 = {"none": 6, "left": 6, "right": 6, "both": 4}[trim]
    #  none: "A  ", " A ", "  A", "   ";  left: "A  ", "A ", "A", "";  right: "A", " A", "  A", "";  both: "A", ""
    kx3 = {"none": 4, "left": 4, "right": 4, "both": 2}[trim]
    return {"KB": 3, "KP": 4, "KZ": 4, "KX4": kx4, "KX3": kx3}


@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
def test_host_equal_values_of_different_bytes_are_one_group(host_shim, trim):
    from oracle import reader_oracle as RO
    p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=trim)
    cb, plan = reader_plan(EQUAL_COPYBOOK, p)
    assert cb.record_size == EQUAL_SIZE
    data = equal_records(plan)
    rows = RO.fixed_len_rows(cb, data, p)
    aggs = [A.CountStar(), A.Sum("VP"), A.Min("VP"), A.Max("VZ"), A.Count("VZ"), A.Count("KP"), A.Sum("KP")]
    t1, t2 = lut_twins(plan)
    twin_is_space = plan.options.lut[t1] == plan.options.lut[0x40]
    counts = equal_expected_counts(trim)
    if twin_is_space:
        counts["KX4"] -= 1          # "A?B " and "A B " are then one value as well
    for col, want in counts.items():
        exp = expected_groups(cb, plan, rows, [col], aggs)
        got = host_group(host_shim, plan, data, [col], aggs, stride=EQUAL_SIZE)
        assert check_groups(got, exp, aggs) == len(exp)
        assert len(got.groups) == want, (col, trim, sorted(got.groups, key=repr))
    for group_by in (["KB", "KP", "KX4", "KX3"], ["KZ", "KX3"]):
        for filters in ([], [F.GreaterThan("VP", 0)]):
            exp = expected_groups(cb, plan, rows, group_by, aggs, filters)
            check_groups(host_group(host_shim, plan, data, group_by, aggs, filters, stride=EQUAL_SIZE), exp, aggs)
    d = len(expected_groups(cb, plan, rows, ["KB", "KP", "KX4", "KX3"], aggs))
    host_group(host_shim, plan, data, ["KB", "KP", "KX4", "KX3"], aggs, max_groups=d, stride=EQUAL_SIZE)
    with pytest.raises(A.GroupOverflow):
        host_group(host_shim, plan, data, ["KB", "KP", "KX4", "KX3"], aggs, max_groups=d - 1, stride=EQUAL_SIZE)


# ---------------------------------------------------------------------------------------------
# group_build refusals
# ---------------------------------------------------------------------------------------------
def test_group_build_refusals(host_shim):
    plan = _plan(WIDE_COPYBOOK)
    size = plan.copybook.record_size

    def status(keys, terms=(), walk=False, n_keys=None, max_groups=16, p=plan):
        g = N.CbxGroupBy()
        g.n_keys = len(keys) if n_keys is None else n_keys
        for i, k in enumerate(keys):
            g.fields[i] = _fi(p, k) if isinstance(k, str) else k
        t = N.CbxAggregate()
        t.n_terms = len(terms)
        for i, (field, funcs) in enumerate(terms):
            t.terms[i].field, t.terms[i].funcs = _fi(p, field), funcs
        try:
            host_group(host_shim, p, bytes(p.copybook.record_size), None, None, max_groups=max_groups,
                       stride=p.copybook.record_size, walk=walk, tables=(g, t))
        except HostError as e:
            return e.rc, e.reason
        return 0, ""

    assert size > 0 and status(["ID", "BIG", "NAME"], [("BIG", N.AGG_COUNT | N.AGG_SUM), ("ID", 15)])[0] == 0
    for keys, kw, word in ((["ITEM-NO"], {}, "OCCURS"), (["RATE"], {}, "COMP-1 / COMP-2 key"),
                           (["NAME"], {"walk": True}, "data-dependent"),
                           (["ID"], {"terms": [("BIG", N.AGG_MIN)]}, "DEC128"), (["ID"], {"terms": [("BIG", N.AGG_MAX | N.AGG_SUM)]}, "DEC128"),
                           (["ID"], {"terms": [("RATE", N.AGG_SUM)]}, "COMP-1 / COMP-2")):
        rc, err = status(keys, **kw)
        assert rc == N.CBX_E_UNSUPPORTED and word in err, (keys, rc, err)
    for keys, kw, word in (([], {}, "1 to 4"), ([], {"n_keys": 5}, "1 to 4"), ([99], {}, "out of range"), ([-1], {}, "out of range"),
                           (["ID", "NAME", "ID"], {}, "repeated"), (["ID"], {"max_groups": 0}, "at least 1"),
                           (["ID"], {"max_groups": 1 << 40}, "workspace")):
        if kw.get("max_groups", 0) > 1 << 30:
            g = N.CbxGroupBy(1, (ctypes.c_int32 * 4)(_fi(plan, "ID")))
            err = ctypes.create_string_buffer(256)
            fields = (N.CbxField * len(plan.fields))(*plan.fields)
            t = N.CbxAggregate()
            rc = host_shim.cbxh_group_strides(ctypes.addressof(fields), len(plan.fields), 0, ctypes.addressof(t),
                                              ctypes.addressof(g), kw["max_groups"], ctypes.addressof(N.CbxGroupStrides()), err, 256)
            rc, err = rc, err.value.decode()
        else:
            rc, err = status(keys, **kw)
        assert rc == N.CBX_E_ARGUMENT and word in err, (keys, rc, err)
    long_plan = _plan("       01  R.\n           05  S32  PIC X(32).\n           05  S33  PIC X(33).\n")
    assert status(["S32"], p=long_plan)[0] == 0
    rc, err = status(["S33"], p=long_plan)
    assert rc == N.CBX_E_UNSUPPORTED and "longer than 32" in err
    from test_decode_fuzz import ASCII_COPYBOOK
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    rc, err = status(["N1"], p=aplan)
    assert rc == N.CBX_E_UNSUPPORTED and "UTF-16" in err
    gen = build_plan(parse_copybook_for(WIDE_COPYBOOK, ReaderParameters()), generate_record_id=True)
    ids = [i for i, f in enumerate(gen.fields) if f.kind in (N.K_RECORD_ID, N.K_FILE_ID)]
    rc, err = status([ids[0]], p=gen)
    assert rc == N.CBX_E_UNSUPPORTED and "generated" in err


# ---------------------------------------------------------------------------------------------
# The stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------
def test_host_program_under_the_sanitizers(tmp_path, syn_plan, syn_rows):
    """tests/native/group_host_main.cpp built with -fsanitize=address,undefined over exact-size heap buffers: the
    fixed run, a framed run that cuts the records inside the key and value fields, max_groups at and below the count."""
    cb, data, rows = syn_rows
    n = 500
    exe = tmp_path / "group_host_check"
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "native", "group_host_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    keys = [_fi(syn_plan, c) for c in ("BR-ID", "NAME")]
    terms = [(_fi(syn_plan, "AMT-01"), 15), (_fi(syn_plan, "ZD-01"), 15), (_fi(syn_plan, "NAME"), 1)]
    head = struct.pack("<4i2q4i16i16i", len(syn_plan.fields), 200, len(keys), len(terms), n, 4096, *(keys + [0, 0]),
                       *([t[0] for t in terms] + [0] * 13), *([t[1] for t in terms] + [0] * 13))
    case = tmp_path / "case.bin"
    fields = (N.CbxField * len(syn_plan.fields))(*syn_plan.fields)
    case.write_bytes(head + bytes(fields) + bytes(syn_plan.options.lut) + data[:200 * n])
    r = subprocess.run([str(exe), str(case)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-4000:], r.stdout)
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    d = len(expected_groups(cb, syn_plan, rows[:n], ["BR-ID", "NAME"], [A.CountStar()]))
    assert lines[0] == ["fixed", "groups", str(d), "rows", str(n), "overflow", "0"]
    assert lines[1][0] == "framed" and lines[1][4] == str(n) and lines[1][6] == "0" and 1 <= int(lines[1][2]) <= d
    assert lines[2] == ["tight", "groups", str(d), "rows", str(n), "overflow", "0"]
    assert lines[3][0] == "tight" and lines[3][6] == "1"
