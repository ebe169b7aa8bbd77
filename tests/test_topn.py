"""Top-N pushdown, the parts that need no GPU: the sort orders and their compilation into the sort table (what is
Unhandled and why), the ABI structs' layout, and the host/device part of cobrix_amd/csrc/cbx_topn.h (topn_build,
topn_word, the pick step) run on the host (tests/native/topn_host.cpp) against the two statements of the contract
in topn_cases.py:

1. the concatenated words of every record equal the Python ENCODER of the oracle row's values;
2. the chosen index set equals the Python EVALUATOR -- sorted(kept, key = compare the values with the None and
   direction rules, then the index)[:limit] -- which works over the oracle's rows and knows nothing of the encoding.

The GPU tests (test_gpu_topn.py) use the same evaluator and the case table pinned here.
"""
from __future__ import annotations

import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from cobrix_amd import filter as F
from cobrix_amd import native as N
from cobrix_amd import topn as T
from cobrix_amd.plan import build_plan
from cobrix_amd.reader import ReaderParameters, parse_copybook_for
from cobrix_amd.synth import SYN200_COPYBOOK, syn200
from test_filter import (FUZZ_N, FUZZ_OPTIONS, LADDER_COPYBOOK, WIDE_COPYBOOK, ascii_records, fuzz_records, ladder_file,
                         ladder_params, leaf_names, narrow_file, narrow_params, reader_plan, row_value)
from topn_cases import (ALL_FLAGS, KEYS_CASES, KEYS_COPYBOOK, KEYS_OPTIONS, KEYS_SIZE, S, composite_keys, expected_indices, expected_info,
                        kept_indices, keys_records)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")


def _fi(plan, name):
    return plan.field_of_node[id(plan.copybook.get_field_by_name(name))]


def _plan(text: str, **kw):
    return build_plan(parse_copybook_for(text, ReaderParameters()), **kw)


@pytest.fixture(scope="module")
def syn_plan():
    return _plan(SYN200_COPYBOOK)


# ---------------------------------------------------------------------------------------------
# SortOrder, compile_order, order_rows
# ---------------------------------------------------------------------------------------------
def test_evaluator_null_and_direction_rules():
    for desc, nf in ALL_FLAGS:
        so = T.SortOrder("X", desc, nf)
        assert T.compare_values(None, None, so) == 0
        assert T.compare_values(None, 5, so) == (-1 if nf else 1) == -T.compare_values(5, None, so)
        assert T.compare_values(1, 2, so) == (1 if desc else -1)
        assert T.compare_values("ab", "ab\x00", so) == (1 if desc else -1)
        assert T.compare_values("ÿ", "z", so) == (-1 if desc else 1)      # UTF-8 bytes, unsigned
    # Spark's default null order: ASC -> NULLS FIRST, DESC -> NULLS LAST
    assert T.SortOrder("X").flags == 0 and T.SortOrder("X", True).flags == N.SORT_DESC | N.SORT_NULLS_LAST
    assert T.SortOrder("X", True, True).flags == N.SORT_DESC and T.SortOrder("X", False, False).flags == N.SORT_NULLS_LAST


def test_compile_order(syn_plan):
    t = T.compile_order(syn_plan, [S("AMT-01", True), S("NAME"), S("BR-ID", False, False), S("ZD-01", True, True)])
    assert t.n_keys == 4
    assert [(t.keys[k].field, t.keys[k].flags) for k in range(4)] == [
        (_fi(syn_plan, "AMT-01"), 3), (_fi(syn_plan, "NAME"), 0), (_fi(syn_plan, "BR-ID"), 2), (_fi(syn_plan, "ZD-01"), 1)]
    assert T.compile_order(syn_plan, []).n_keys == 0                       # the plain LIMIT


def test_compile_order_every_refusal(syn_plan):
    plan = _plan(WIDE_COPYBOOK)
    for so, word in ((S("ITEM-NO"), "OCCURS"), (S("VALS"), "OCCURS"), (S("RATE"), "COMP-1 / COMP-2"),
                     (S("NO-SUCH"), "not found"), (S("ITEMS"), "primitive"), ("ID", "SortOrder")):
        with pytest.raises(T.Unhandled, match=word):      # all or nothing: one key refuses the whole order
            T.compile_order(plan, [S("ID"), so])
    with pytest.raises(T.Unhandled, match="repeated"):
        T.compile_order(plan, [S("ID"), S("NAME"), S("ID", True)])
    with pytest.raises(T.Unhandled, match="up to 4"):
        T.compile_order(syn_plan, [S(c) for c in ("AMT-01", "AMT-02", "AMT-03", "AMT-04", "AMT-05")])
    cb = parse_copybook_for(WIDE_COPYBOOK, ReaderParameters(variable_size_occurs=True))
    walk = build_plan(cb, walk=True, variable_size_occurs=True, string_views=1)
    with pytest.raises(T.Unhandled, match="data-dependent"):
        T.compile_order(walk, [S("NAME")])
    from test_decode_fuzz import ASCII_COPYBOOK
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    with pytest.raises(T.Unhandled, match="UTF-16"):
        T.compile_order(aplan, [S("N2")])
    _, lplan = reader_plan(LADDER_COPYBOOK, ladder_params("both"))
    with pytest.raises(T.Unhandled, match="longer than 32"):
        T.compile_order(lplan, [S("X33")])
    assert T.compile_order(lplan, [S("X32")]).n_keys == 1


def test_order_rows_is_the_evaluators_order():
    from oracle import reader_oracle as RO
    p = ReaderParameters(**KEYS_OPTIONS)
    cb = parse_copybook_for(KEYS_COPYBOOK, p)
    rows = RO.fixed_len_rows(cb, keys_records(200), p)
    orders = [S("LOW", True), S("AMT", False, False), S("TXT")]
    got = T.order_rows(cb, rows, orders)
    _, all_idx = expected_indices(cb, rows, orders, 200)
    assert all_idx == list(range(200))
    import functools

    def cmp(a, b):
        for so in orders:
            c = T.compare_values(row_value(cb, rows[a], so.column), row_value(cb, rows[b], so.column), so)
            if c:
                return c
        return (a > b) - (a < b)
    assert [r["SEQ"] for r in got] == sorted(range(200), key=functools.cmp_to_key(cmp))


# ---------------------------------------------------------------------------------------------
# ABI structs
# ---------------------------------------------------------------------------------------------
TOPN_STRUCTS = {"cbx_sort_key": N.CbxSortKey, "cbx_sort_order": N.CbxSortOrder, "cbx_topn_info": N.CbxTopnInfo}


def test_topn_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of the Top-N structs as a C compiler sees include/cobrix_hip.h, and the constants."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cobrix_hip.h"', "int main(void) {"]
    for cname, py in TOPN_STRUCTS.items():
        src.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            src.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    consts = {"CBX_TOPN_MAX_KEYS": N.CBX_TOPN_MAX_KEYS, "CBX_SORT_DESC": N.SORT_DESC, "CBX_SORT_NULLS_LAST": N.SORT_NULLS_LAST,
              "CBX_ABI_VERSION": N.ABI_VERSION}
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
        py = TOPN_STRUCTS[cname]
        got = ctypes.sizeof(py) if what == "sizeof" else getattr(py, what).offset
        assert got == int(val), f"{cname}.{what}: ctypes {got} != C {val}"
    assert seen == len(consts) + sum(1 + len(py._fields_) for py in TOPN_STRUCTS.values())
    assert N.ABI_VERSION == 25 and set(N.TOPN_SYMBOLS) <= set(N.EXPORTED_SYMBOLS)
    assert set(N.TOPN_SYMBOLS) == {"cbx_top_n_records", "cbx_top_n_info", "cbx_top_n_pass_times"}


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
    so = tmp_path_factory.mktemp("topn_host") / "libcbx_topn_host.so"
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-o", str(so), os.path.join(ROOT, "tests", "native", "topn_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_topn_words.argtypes = [P, i32, i32, P, P, P, i64, P, P, P, i64, i32, i32, i32, P, i64, P, P, ctypes.c_char_p, i32]
    lib.cbxh_topn_select.argtypes = [P, i32, i32, P, P, P, P, i64, P, P, P, i64, i32, i32, i32, i64, P, P, P,
                                     ctypes.c_char_p, i32]
    return lib


class HostError(Exception):
    def __init__(self, rc, reason):
        super().__init__(f"{rc}: {reason}")
        self.rc, self.reason = rc, reason


class Source:
    """One record source of the host shim: fixed-length records (stride) or framed ones (rec_off, rec_len, rec_seg)."""

    def __init__(self, plan, data: bytes, stride: int = 0, framing=None, start_off: int = 0, walk: bool = False):
        self.plan, self.data, self.stride, self.start_off, self.walk = plan, data, stride, start_off, walk
        self.buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
        self.fields = (N.CbxField * len(plan.fields))(*plan.fields)
        self.off = self.ln = self.seg = None
        if framing is not None:
            self.off = np.ascontiguousarray(framing[0], dtype=np.int64)
            self.ln = np.ascontiguousarray(framing[1], dtype=np.int32)
            self.seg = np.ascontiguousarray(framing[2], dtype=np.int32) if framing[2] is not None else None
            self.n = len(self.off)
        else:
            self.n = len(data) // stride

    def _records(self):
        p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
        return (ctypes.addressof(self.plan.options.lut), self.buf.ctypes.data, len(self.data), p(self.off), p(self.ln),
                p(self.seg), self.n, self.stride, self.start_off, -1)

    def words(self, lib, table: N.CbxSortOrder):
        """(keys [n] as bytes, levels_total, words_per_key) of the host topn_word."""
        err = ctypes.create_string_buffer(256)
        cap = self.n * 60 + 1
        out = np.zeros(cap, dtype=np.uint64)
        lt = ctypes.c_int32(0)
        wpk = (ctypes.c_int32 * 4)()
        rc = lib.cbxh_topn_words(ctypes.addressof(self.fields), len(self.plan.fields), int(self.walk), ctypes.addressof(table),
                                 *self._records(), out.ctypes.data, cap, ctypes.byref(lt), wpk, err, 256)
        if rc != 0:
            raise HostError(rc, err.value.decode())
        w = out[:self.n * lt.value].astype(">u8").tobytes()
        return [w[8 * lt.value * i:8 * lt.value * (i + 1)] for i in range(self.n)], lt.value, list(wpk)

    def select(self, lib, table: N.CbxSortOrder, limit: int, flt=None):
        """(ascending indices, cbx_topn_info) of the host select."""
        err = ctypes.create_string_buffer(256)
        out = np.zeros(max(1, min(max(limit, 0), self.n)), dtype=np.int64)
        n_out = ctypes.c_int64(0)
        info = N.CbxTopnInfo()
        rc = lib.cbxh_topn_select(ctypes.addressof(self.fields), len(self.plan.fields), int(self.walk),
                                  ctypes.addressof(flt) if flt is not None else None, ctypes.addressof(table),
                                  *self._records(), limit, out.ctypes.data, ctypes.byref(n_out), ctypes.byref(info), err, 256)
        if rc != 0:
            raise HostError(rc, err.value.decode())
        return out[:n_out.value].tolist(), info


def _filter_table(plan, filters):
    if not filters:
        return None
    flt, un = F.compile_filters(plan, filters)
    assert not un, un.reasons
    return flt


def check_case(lib, cb, src: Source, rows, orders, limit, filters=(), stats=None):
    """One (orders, limit, filters) through both checks; returns the host's cbx_topn_info."""
    plan = src.plan
    assert len(rows) == src.n
    table = T.compile_order(plan, orders)
    keys = composite_keys(cb, plan, rows, orders)
    got_keys, lt, wpk = src.words(lib, table)
    bad = [(i, got_keys[i].hex(), keys[i].hex()) for i in range(src.n) if got_keys[i] != keys[i]]
    assert not bad, (orders, bad[:3])
    assert lt == (len(keys[0]) // 8 if keys else lt)
    kept, chosen = expected_indices(cb, rows, orders, limit, filters)
    got, info = src.select(lib, table, limit, _filter_table(plan, filters))
    assert got == chosen, (orders, limit, got[:10], chosen[:10])
    exp = expected_info(keys, kept, limit, src.n)
    have = {k: getattr(info, k) for k in ("n_live", "levels_run", "ties_after_level0", "ties_max")}
    assert have == {k: exp[k] for k in have}, (orders, limit, have, exp)
    assert info.levels_total == lt and list(info.words_per_key)[:len(orders)] == wpk[:len(orders)]
    if stats is not None:
        stats.append({"orders": orders, "limit": limit, "kept": len(kept), "levels_run": info.levels_run,
                      "index_decides": info.levels_run == info.levels_total and info.levels_run > 0,
                      "all_null": bool(orders) and bool(kept) and all(
                          row_value(cb, rows[i], so.column) is None for i in kept for so in orders)})
    return info


def assert_table_properties(stats, need_levels3=True, need_all_null=True):
    """The case table's own properties: without them a source's test could pass vacuously."""
    flags = {(so.descending, so.nulls_first_resolved) for s in stats for so in s["orders"]}
    assert flags == set(ALL_FLAGS), flags
    assert any(s["index_decides"] for s in stats), "no case where the boundary tie class needs the index word"
    assert any(s["limit"] > s["kept"] > 0 for s in stats), "no case with limit > kept"
    if need_levels3:
        assert any(s["levels_run"] >= 3 for s in stats), "no case reaches three levels"
    if need_all_null:
        assert any(s["all_null"] for s in stats), "no case with every key null"


def orders_for(plan, cb, names, rng, n_cases=12):
    """Sort orders over the accepted leaves `names`: every leaf once alone (flags cycling), then mixed 2-4 key
    orders."""
    out = []
    for k, nm in enumerate(names):
        d, nf = ALL_FLAGS[k % 4]
        out.append([S(nm, d, nf)])
    for _ in range(n_cases):
        ks = rng.sample(names, min(len(names), rng.randint(2, 4)))
        out.append([S(nm, *ALL_FLAGS[rng.randrange(4)]) for nm in ks])
    return out


def accepted_names(plan, cb):
    names = []
    for nm in leaf_names(cb):
        try:
            T.compile_order(plan, [S(nm)])
            names.append(nm)
        except T.Unhandled:
            pass
    return names


def run_source(lib, cb, src, rows, rng, filters_list=((),), constant=None, n_mixed=12, need_levels3=True, need_all_null=True,
               null_filter=None):
    """Every accepted leaf of the copybook as a sort key, mixed orders, limits around the kept count; `constant`: a
    leaf whose value is the same in most rows (a tie class the index word must split)."""
    plan = src.plan
    names = accepted_names(plan, cb)
    stats = []
    n = src.n
    for filters in filters_list:
        kept = len(kept_indices(cb, rows, filters))
        limits = sorted({1, 2, max(1, kept // 3), max(1, kept - 1), kept, kept + 1, n + 5, 0})
        for k, orders in enumerate(orders_for(plan, cb, names, rng, n_mixed)):
            check_case(lib, cb, src, rows, orders, limits[k % len(limits)], filters, stats)
        check_case(lib, cb, src, rows, [], max(1, kept // 2), filters, stats)         # the plain LIMIT
        check_case(lib, cb, src, rows, [S(names[0])], kept + 1, filters, stats)
        if constant:
            # several keys in front, so the tie class survives at least two words before the index decides
            for d, nf in ALL_FLAGS:
                check_case(lib, cb, src, rows, [S(c, d, nf) for c in constant], max(1, kept // 2), filters, stats)
    if null_filter is not None:
        f, cols = null_filter
        check_case(lib, cb, src, rows, [S(c, k % 2 == 1) for k, c in enumerate(cols)], 3, [f], stats)
    assert_table_properties(stats, need_levels3, need_all_null)
    return stats


def test_topn_build_refusals(host_shim):
    plan = _plan(WIDE_COPYBOOK)
    size = plan.copybook.record_size

    def status(keys, walk=False, n_keys=None, p=plan):
        t = N.CbxSortOrder()
        t.n_keys = len(keys) if n_keys is None else n_keys
        for i, (field, flags) in enumerate(keys):
            t.keys[i].field = _fi(p, field) if isinstance(field, str) else field
            t.keys[i].flags = flags
        try:
            Source(p, bytes(p.copybook.record_size), p.copybook.record_size, walk=walk).words(host_shim, t)
        except HostError as e:
            return e.rc, e.reason
        return 0, ""

    assert size > 0 and status([("ID", 0), ("BIG", 3), ("NAME", 1), ("CNT", 2)])[0] == 0
    assert status([])[0] == 0                                                       # the plain LIMIT
    for keys, word in (([("ITEM-NO", 0)], "OCCURS"), ([("VALS", 1)], "OCCURS"), ([("RATE", 0)], "COMP-1 / COMP-2")):
        rc, err = status(keys)
        assert rc == N.CBX_E_UNSUPPORTED and word in err and err.startswith("cbx_sort_order: key 0: "), (keys, rc, err)
    rc, err = status([("NAME", 0)], walk=True)
    assert rc == N.CBX_E_UNSUPPORTED and "data-dependent" in err
    for keys, kw, word in (([(99, 0)], {}, "out of range"), ([(-1, 0)], {}, "out of range"), ([("ID", 4)], {}, "flag bits"),
                           ([("ID", -1)], {}, "flag bits"), ([("ID", 0), ("BIG", 0), ("ID", 1)], {}, "repeated"),
                           ([], {"n_keys": N.CBX_TOPN_MAX_KEYS + 1}, "sort keys"), ([], {"n_keys": -1}, "sort keys")):
        rc, err = status(keys, **kw)
        assert rc == N.CBX_E_ARGUMENT and word in err, (keys, rc, err)
    from test_decode_fuzz import ASCII_COPYBOOK
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    rc, err = status([("N1", 0)], p=aplan)
    assert rc == N.CBX_E_UNSUPPORTED and "UTF-16" in err
    _, lplan = reader_plan(LADDER_COPYBOOK, ladder_params("both"))
    rc, err = status([("X33", 0)], p=lplan)
    assert rc == N.CBX_E_UNSUPPORTED and "longer than 32" in err
    gen = build_plan(parse_copybook_for(WIDE_COPYBOOK, ReaderParameters()), generate_record_id=True)
    ids = [i for i, f in enumerate(gen.fields) if f.kind in (N.K_RECORD_ID, N.K_FILE_ID)]
    rc, err = status([(ids[0], 0)], p=gen)
    assert rc == N.CBX_E_UNSUPPORTED and "generated" in err
    # a filter the stage refuses refuses the call
    t = T.compile_order(plan, [S("ID")])
    flt = N.CbxFilter()
    flt.n_terms = 1
    flt.terms[0].field, flt.terms[0].op = _fi(plan, "ITEM-NO"), N.OP_IS_NULL
    with pytest.raises(HostError, match="OCCURS"):
        Source(plan, bytes(size), size).select(host_shim, t, 1, flt)
    with pytest.raises(HostError, match="limit"):
        Source(plan, bytes(size), size).select(host_shim, t, -1)


@pytest.fixture(scope="module")
def keys_source():
    from oracle import reader_oracle as RO
    p = ReaderParameters(**KEYS_OPTIONS)
    cb, plan = reader_plan(KEYS_COPYBOOK, p)
    assert cb.record_size == KEYS_SIZE
    data = keys_records(4097)
    rows = RO.fixed_len_rows(cb, data, p)
    return cb, plan, data, rows


def test_keys_records_hold_what_their_docstring_says(keys_source):
    cb, plan, data, rows = keys_source
    lng = [r["LNG"] for r in rows[:1000]]
    assert min(lng) == -(1 << 63) and max(lng) == (1 << 63) - 1 and None not in lng
    big = [r["BIG"] for r in rows[:1000]]
    assert 10 ** 38 - 1 in big and -(10 ** 38 - 1) in big and sum(v is None for v in big) == 90
    assert {r["CST"] for r in rows} == {42} and {r["LOW"] for r in rows} == {-2, -1, 0, 1, 2}
    assert sum(r["AMT"] is None for r in rows[:1000]) == 142 and "" in {r["TXT"] for r in rows}
    assert any("\u00a3" in r["HEX"] for r in rows) and any("\u00ac" in r["TXT"] for r in rows) and plan.fields[_fi(plan, "BIG")].out_type == N.O_DEC128


@pytest.mark.parametrize("case", KEYS_CASES, ids=[c[0] for c in KEYS_CASES])
def test_keys_case_table_is_pinned(host_shim, keys_source, case):
    """Every literal of KEYS_CASES (the GPU module asserts cbx_top_n_info against them) equals what the evaluator and
    the encoder derive from the oracle's rows, and the host select agrees."""
    cb, plan, data, rows = keys_source
    name, n, orders, limit, _, _, (n_live, levels_run, ties0) = case
    src = Source(plan, data[:n * KEYS_SIZE], KEYS_SIZE)
    keys = composite_keys(cb, plan, rows[:n], orders)
    exp = expected_info(keys, list(range(n)), limit, n)
    assert (exp["n_live"], exp["levels_run"], exp["ties_after_level0"]) == (n_live, levels_run, ties0), (name, exp)
    if n:
        check_case(host_shim, cb, src, rows[:n], orders, limit)


def test_keys_case_table_properties(keys_source):
    cb, plan, data, rows = keys_source
    assert {c[1] for c in KEYS_CASES} >= {0, 1, 63, 64, 65, 1000, 4097}
    assert {c[4] for c in KEYS_CASES} == {0, 1, 3} and any(c[5] for c in KEYS_CASES)
    flags = {(so.descending, so.nulls_first_resolved) for c in KEYS_CASES for so in c[2]}
    assert flags == set(ALL_FLAGS)
    assert any(c[6][1] >= 3 for c in KEYS_CASES) and any(c[3] > c[1] > 0 for c in KEYS_CASES)
    assert any(len(c[2]) == 4 for c in KEYS_CASES) and any(len(c[2]) == 2 for c in KEYS_CASES) and any(not c[2] for c in KEYS_CASES)
    assert any(c[6][2] > c[3] for c in KEYS_CASES)       # a tie class larger than the limit: the index word decides


def test_host_keys_every_flag_filter_and_all_null(host_shim, keys_source):
    cb, plan, data, rows = keys_source
    n = 1000
    src = Source(plan, data[:n * KEYS_SIZE], KEYS_SIZE)
    stats = run_source(host_shim, cb, src, rows[:n], random.Random(3),
                       filters_list=((), [F.GreaterThan("LOW", 0)], [F.IsNull("AMT")]),
                       constant=["CST", "LOW"], null_filter=(F.And(F.IsNull("AMT"), F.IsNull("BIG")), ["AMT", "BIG"]))
    assert len(stats) > 60


@pytest.fixture(scope="module")
def syn_rows():
    from oracle import oracle as O
    cb = parse_copybook_for(SYN200_COPYBOOK, ReaderParameters())
    data = syn200(1000, seed=5, malformed_rate=0.2).numpy().tobytes()
    return cb, data, O.rows(O.decode_fixed(cb, data), collapse_root=True)


def test_host_syn200(host_shim, syn_plan, syn_rows):
    cb, data, rows = syn_rows
    src = Source(syn_plan, data, 200)
    names = accepted_names(syn_plan, cb)
    assert "FX_RATE" not in names and "NAME" in names and "AMT_01" in names and len(names) >= 27
    brs = sorted(v for v in (row_value(cb, r, "BR-ID") for r in rows) if v is not None)
    stats = run_source(host_shim, cb, src, rows, random.Random(5),
                       filters_list=((), [F.LessThan("BR-ID", brs[len(brs) // 2])], [F.LessThan("NAME", "M")]),
                       constant=None, need_levels3=False,
                       null_filter=(F.And(F.IsNull("AMT-01"), F.IsNull("QTY-01")), ["AMT-01", "QTY-01"]))
    assert len(stats) > 100


@pytest.mark.parametrize("start,end", [(0, 0), (3, 2)])
@pytest.mark.parametrize("code_page,trim", FUZZ_OPTIONS)
def test_host_every_decoder_kind_ebcdic(host_shim, code_page, trim, start, end):
    from oracle import reader_oracle as RO
    from test_decode_fuzz import FUZZ_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim,
                         start_offset=start, end_offset=end)
    cb, plan = reader_plan(FUZZ_COPYBOOK, p)
    data = fuzz_records(cb, FUZZ_N, 31, start, end)
    rows = RO.fixed_len_rows(cb, data, p)
    src = Source(plan, data, cb.record_size + start + end, start_off=start)
    names = accepted_names(plan, cb)
    assert not {"F01", "F02"} & set(names) and len(names) > 55
    stats = run_source(host_shim, cb, src, rows, random.Random(7), filters_list=((), [F.IsNotNull("P05")]),
                       need_levels3=False, need_all_null=False)
    assert len(stats) > 2 * 60


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_host_every_decoder_kind_ascii(host_shim, charset):
    from oracle import reader_oracle as RO
    from test_decode_fuzz import ASCII_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
    cb, plan = reader_plan(ASCII_COPYBOOK, p)
    data = ascii_records(cb, FUZZ_N, 32)
    rows = RO.fixed_len_rows(cb, data, p)
    src = Source(plan, data, cb.record_size)
    stats = run_source(host_shim, cb, src, rows, random.Random(9), filters_list=((), [F.GreaterThan("A02", 0)]),
                       need_levels3=False, need_all_null=False)
    assert len(stats) > 20


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_width_ladder_cut_at_every_length(host_shim, trim):
    """One ladder record per length 1..L: every key is NULL, "" (a string starting at the record's end), a truncated
    string and a whole value somewhere; the short records make all-null key sets."""
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    raw, off, ln = ladder_file(seed=34, every_length=True)
    rows = RO.var_len_rows(cb, raw, p)
    src = Source(plan, raw, framing=(off, ln, None))
    names = accepted_names(plan, cb)
    assert "X32" in names and "X33" not in names
    vals = [row_value(cb, r, "X08") for r in rows]
    assert None in vals and "" in vals
    stats = run_source(host_shim, cb, src, rows, random.Random(11), filters_list=((), [F.IsNotNull("P08")]),
                       need_levels3=True, null_filter=(F.IsNull("X47"), ["P47", "Z47"]))
    assert len(stats) > 2 * 50


def test_host_segment_redefines(host_shim):
    """RDW_NARROW with its redefine map: a key of the inactive redefine is NULL."""
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
    src = Source(plan, raw, framing=(off, ln, seg))
    stats = run_source(host_shim, cb, src, rows, random.Random(13), filters_list=((), [F.EqualTo("SEGMENT-ID", "C")]),
                       constant=["SEGMENT-ID", "TAXPAYER-TYPE"], need_levels3=False,
                       null_filter=(F.EqualTo("SEGMENT-ID", "P"), ["COMPANY-NAME", "TAXPAYER-NUM"]))
    assert len(stats) > 20
    # the segment matters: with no active segment every key of a redefine is NULL, and the first n by index win
    bare = Source(plan, raw, framing=(off, ln, None))
    got, info = bare.select(host_shim, T.compile_order(plan, [S("COMPANY-NAME"), S("PHONE-NUMBER", True)]), 7)
    assert got == list(range(7)) and info.levels_run == info.levels_total


@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
def test_host_equal_values_of_different_bytes_tie(host_shim, trim):
    """test_group.py's records: the sign nibbles of a COMP-3 zero, overpunch spellings of one zoned number, padding-only
    differences and two source bytes with one image order as EQUAL values -- they tie and the index decides."""
    from oracle import reader_oracle as RO
    from test_group import EQUAL_COPYBOOK, EQUAL_SIZE, equal_expected_counts, equal_records, lut_twins
    p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=trim)
    cb, plan = reader_plan(EQUAL_COPYBOOK, p)
    data = equal_records(plan)
    rows = RO.fixed_len_rows(cb, data, p)
    src = Source(plan, data, EQUAL_SIZE)
    counts = equal_expected_counts(trim)
    if plan.options.lut[lut_twins(plan)[0]] == plan.options.lut[0x40]:
        counts["KX4"] -= 1          # the twins' image is the space: "A?B " and "A B " are then one value as well
    for col, distinct in counts.items():
        keys, _, _ = src.words(host_shim, T.compile_order(plan, [S(col)]))
        assert len({k[:-8] for k in keys}) == distinct, col                  # one composite key per VALUE
    stats = run_source(host_shim, cb, src, rows, random.Random(15), constant=["KB", "KZ", "KX3"], n_mixed=20,
                       need_all_null=False)
    assert len(stats) > 30


# ---------------------------------------------------------------------------------------------
# The stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------
def test_host_program_under_the_sanitizers(tmp_path):
    """tests/native/topn_host_main.cpp built with -fsanitize=address,undefined: random records in exact-size heap
    buffers, strides that cut the records inside the key fields, every key kind, flag set and level."""
    exe = tmp_path / "topn_host_check"
    native = os.path.join(ROOT, "tests", "native")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"), "-o", str(exe),
                        os.path.join(native, "topn_host.cpp"), os.path.join(native, "topn_host_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-4000:], r.stdout)
    assert "no sanitizer report" in r.stdout
