"""Grouped aggregate pushdown on the GPU (cbx_aggregate_grouped) against the contract: per distinct key of the GROUP BY
columns, COUNT(*), COUNT, MIN, MAX and SUM over the rows the filters keep equal the Python evaluator of test_group.py
(`expected_groups`: the ORACLE's rows grouped by `row_value` of the key columns, `expected_aggregates` per group) --
never the code under test.  Sums are compared bit for bit, keys and values in Spark's types.
"""
from __future__ import annotations

import ctypes
from decimal import Decimal

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from cobrix_amd import aggregate as A  # noqa: E402
from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.options import parse_options  # noqa: E402
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader, parse_copybook_for  # noqa: E402
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, SYN200_COPYBOOK, rdw_file, rdw_narrow, syn200  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_aggregate import ALL_FUNCS  # noqa: E402
from test_filter import FUZZ_N, narrow_file, narrow_params, py_keep  # noqa: E402
from test_gpu_filter import NARROW_OPTIONS, OCCURS_COPYBOOK, SHORT_COPYBOOK, narrow_cases, syn_predicates  # noqa: E402
from test_group import (EQUAL_COPYBOOK, EQUAL_SIZE, check_groups, equal_expected_counts, equal_records,  # noqa: E402
                        expected_groups, lut_twins)

PARAMS = ReaderParameters(schema_policy="collapse_root")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _device(data: bytes, odd: bool = False):
    t = torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8)
    if not odd:
        return t.cuda()
    buf = torch.zeros(len(data) + 9, dtype=torch.uint8, device="cuda")   # a batch cut out of a larger buffer
    buf[9:] = t.cuda()
    return buf[9:]


# ---------------------------------------------------------------------------------------------
# Key patterns on a small copybook: a binary key, a string key, a long, a 38-digit decimal, a nullable COMP-3
# ---------------------------------------------------------------------------------------------
PAT_COPYBOOK = """
       01  R.
           05  K     PIC S9(9) COMP.
           05  S     PIC X(4).
           05  V     PIC S9(18) COMP.
           05  BIG   PIC S9(38) COMP-3.
           05  P     PIC S9(5) COMP-3.
"""
PAT_SIZE = 4 + 4 + 8 + 20 + 3
PAT_AGGS = [A.CountStar()] + [fn("V") for fn in ALL_FUNCS] + [A.Count("BIG"), A.Sum("BIG")] + [fn("P") for fn in ALL_FUNCS] + \
    [A.Count("S"), A.Sum("K")]
TOP38 = 10 ** 38 - 1


def _bcd(v: int, size: int) -> bytes:
    nib = [int(c) for c in str(abs(v)).rjust(2 * size - 1, "0")] + [0xD if v < 0 else 0xC]
    return bytes((nib[2 * j] << 4) | nib[2 * j + 1] for j in range(size))


def pat_record(k: int, s: int, v: int, big: int, p) -> bytes:
    """s: a number spelt as four EBCDIC digits; p: None gives a malformed (null) COMP-3."""
    return k.to_bytes(4, "big", signed=True) + f"{s:04d}".encode("cp037") + v.to_bytes(8, "big", signed=True) + \
        _bcd(big, 20) + (_bcd(p, 3) if p is not None else b"\xff\xff\xff")


def pat_data(n: int, key) -> bytes:
    return b"".join(pat_record(key(i), i % 1031, (i * 2654435761) % (1 << 40) - (1 << 39), (i * 7919 - 3000) * 10 ** 20,
                               None if i % 11 == 0 else (i * 37) % 1999 - 999) for i in range(n))


@pytest.fixture(scope="module")
def pat_reader():
    rd = FixedLenNestedReader(PAT_COPYBOOK, PARAMS)
    assert rd.get_record_size() == PAT_SIZE
    yield rd
    rd.close()


PATTERNS = {"one": lambda i: -5, "seven": lambda i: (i * 3) % 7 - 3, "distinct": lambda i: 100000 - 3 * i}


@pytest.fixture(scope="module")
def pat(pat_reader):
    """{pattern: (data of 4096 records, their oracle rows)} -- computed once, shared, never changed."""
    out = {}
    for name, key in PATTERNS.items():
        data = pat_data(4096, key)
        out[name] = (data, RO.fixed_len_rows(pat_reader.copybook, data, PARAMS))
    return out


def _pat_check(rd, data, rows, group_by, aggs=PAT_AGGS, filters=(), max_groups=None, mw=0, odd=False):
    exp = expected_groups(rd.copybook, rd.plan, rows, group_by, aggs, filters)
    t = _device(data, odd)
    got = rd.aggregate_by_device(t, len(data), group_by, aggs, list(filters) or None,
                                 max_groups=max_groups if max_groups is not None else max(1, len(exp)), max_workgroups=mw)
    assert check_groups(got, exp, aggs) == len(exp)
    return got, exp


@pytest.mark.parametrize("n,mw,odd", [(0, 0, False), (1, 0, False), (63, 0, False), (64, 0, False), (65, 0, False),
                                      (257, 0, False), (257, 0, True), (4096, 0, False), (4096, 1, False), (4096, 3, False)])
def test_boundaries(pat_reader, pat, n, mw, odd):
    """A partial last tile, idle waves, two workgroups, 64 tiles on 1 and 3 workgroups, an odd data pointer; one group,
    seven groups and all-distinct keys (max_groups = the distinct count: a table filled to half)."""
    for name, (data, rows) in pat.items():
        got, exp = _pat_check(pat_reader, data[:n * PAT_SIZE], rows[:n], ["K"], mw=mw, odd=odd)
        assert len(exp) == {"one": min(n, 1), "seven": min(n, 7), "distinct": n}[name]
        assert got.n_rows == n and (n > 0 or got.groups == {})


def test_host_bytes_entry_point(pat_reader, pat):
    data, rows = pat["seven"]
    got = pat_reader.aggregate_by(data[:130 * PAT_SIZE], ["K"], PAT_AGGS)
    check_groups(got, expected_groups(pat_reader.copybook, pat_reader.plan, rows[:130], ["K"], PAT_AGGS), PAT_AGGS)
    with pytest.raises(ValueError):
        pat_reader.aggregate_by(data[:130 * PAT_SIZE - 1], ["K"], PAT_AGGS)


# ---------------------------------------------------------------------------------------------
# Probing, overflow, cache eviction, high-cardinality tiles
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def modular(pat_reader):
    """16,384 records, K = i mod 97 and S = i mod 1031 (pat_data spells it): one workgroup sees 256 tiles, every cache
    entry is evicted many times."""
    data = pat_data(16384, lambda i: i % 97)
    return data, RO.fixed_len_rows(pat_reader.copybook, data, PARAMS)


def test_probing_sixteen_slots_eight_keys(pat_reader):
    data = pat_data(512, lambda i: (i * 5) % 8 * 1000003)
    rows = RO.fixed_len_rows(pat_reader.copybook, data, PARAMS)
    got, exp = _pat_check(pat_reader, data, rows, ["K"], max_groups=8)
    assert len(exp) == 8
    with pytest.raises(A.GroupOverflow, match="max_groups = 7"):
        pat_reader.aggregate_by(data, ["K"], PAT_AGGS, max_groups=7)


@pytest.mark.parametrize("group_by,distinct", [(["K"], 97), (["S"], 1031)])
@pytest.mark.parametrize("mw", [0, 1])
def test_max_groups_exact_and_cache_eviction(pat_reader, modular, group_by, distinct, mw):
    """max_groups = the distinct count must succeed (no spurious overflow), one less must raise -- and return."""
    data, rows = modular
    aggs = [A.CountStar(), A.Sum("V"), A.Min("V"), A.Max("P"), A.Count("P"), A.Sum("BIG")]
    got, exp = _pat_check(pat_reader, data, rows, group_by, aggs, max_groups=distinct, mw=mw)
    assert len(exp) == distinct
    with pytest.raises(A.GroupOverflow, match="max_groups"):
        pat_reader.aggregate_by(data, group_by, aggs, max_groups=distinct - 1)
    # the reader is usable after an overflow
    assert pat_reader.aggregate_by(data[:PAT_SIZE], group_by, aggs, max_groups=1).n_rows == 1


def test_tiles_of_sixty_four_keys_beside_tiles_of_one(pat_reader):
    """Even tiles hold 64 distinct keys (past the distinct-id bound: single-value flushes), odd tiles one key; and a
    tile of nine keys, one past the bound."""
    data = pat_data(1024, lambda i: 100 + i % 64 if (i // 64) % 2 == 0 else (7 if i // 64 != 5 else i % 9))
    rows = RO.fixed_len_rows(pat_reader.copybook, data, PARAMS)
    for mw in (0, 1):
        got, exp = _pat_check(pat_reader, data, rows, ["K"], mw=mw)
        assert len(exp) == 64 + 9
    _pat_check(pat_reader, data, rows, ["K", "S"], mw=1)


# ---------------------------------------------------------------------------------------------
# Exact arithmetic per group
# ---------------------------------------------------------------------------------------------
def _exact_check(rd, recs, aggs=PAT_AGGS):
    data = b"".join(recs)
    rows = RO.fixed_len_rows(rd.copybook, data, PARAMS)
    got0, exp = _pat_check(rd, data, rows, ["K"], aggs, mw=0)
    got1, _ = _pat_check(rd, data, rows, ["K"], aggs, mw=1)
    assert {k: g.raw for k, g in got0.groups.items()} == {k: g.raw for k, g in got1.groups.items()}
    return got0


def test_sum_uses_the_third_limb_per_group(pat_reader):
    """Two groups of 300 rows of +(10^38 - 1) and -(10^38 - 1), interleaved: |sum| > 2^127 in each."""
    got = _exact_check(pat_reader, [pat_record(i % 2, 0, 0, TOP38 if i % 2 else -TOP38, 1) for i in range(600)])
    for k, sign in ((0, -1), (1, 1)):
        big = got.groups[(k,)].raw["terms"][1]
        assert big["sum"] == sign * 300 * TOP38 and abs(big["sum"]) > 2 ** 127 and big["count"] == 300
        assert dict(zip(PAT_AGGS, got.groups[(k,)].values))[A.Sum("BIG")] is None          # Spark: overflow -> null


def test_long_sum_wraps_and_int64_extremes(pat_reader):
    v = 10 ** 18 - 1
    recs = [pat_record(3, 0, v, 0, 1) for _ in range(10)] + \
           [pat_record(4, 0, -2 ** 63 if i % 2 else 2 ** 63 - 1, 0, 1) for i in range(130)]
    got = _exact_check(pat_reader, recs)
    a = dict(zip(PAT_AGGS, got.groups[(3,)].values))
    assert got.groups[(3,)].raw["terms"][0]["sum"] == 10 * v > 2 ** 63 and a[A.Sum("V")] == 10 * v - 2 ** 64
    t = got.groups[(4,)].raw["terms"][0]
    assert (t["min"], t["max"], t["sum"]) == (-2 ** 63, 2 ** 63 - 1, -65)


def test_carries_cross_limbs_under_concurrent_adds(pat_reader):
    """Low limbs of all ones beside values that fill the second limb, in two groups spread over many tiles and
    workgroups: every flush carries out of limb 0, many out of limb 1; one workgroup and many give the same sums."""
    vals = [2 ** 64 - 1, 2 ** 126 - 1, -(2 ** 64 - 1), 2 ** 64 - 1, 2 ** 126 + 2 ** 64 - 1, -1, 2 ** 126 - 1, 2 ** 64]
    recs = [pat_record(i % 2, i % 5, -1 if i % 3 else 2 ** 63 - 1, vals[(i // 2) % 8], 1) for i in range(2048)]
    got = _exact_check(pat_reader, recs)
    assert all(abs(g.raw["terms"][1]["sum"]) > 2 ** 128 for g in got.groups.values())
    # and with 65 groups per tile neighbourhood: the single-value flushes carry too
    recs = [pat_record(i % 65, 0, -1, vals[i % 8], 1) for i in range(2080)]
    _exact_check(pat_reader, recs)


def test_a_group_whose_values_are_all_null(pat_reader):
    recs = [pat_record(i % 3, 0, i, i, None if i % 3 == 1 else i) for i in range(200)]
    got = _exact_check(pat_reader, recs)
    a = dict(zip(PAT_AGGS, got.groups[(1,)].values))
    assert [a[fn("P")] for fn in ALL_FUNCS] == [0, None, None, None] and a[A.CountStar()] == 67
    assert got.groups[(1,)].raw["terms"][2] == {"field": got.groups[(1,)].raw["terms"][2]["field"], "count": 0, "min": None,
                                                "max": None, "sum": None}


# ---------------------------------------------------------------------------------------------
# NULL and equal-value keys
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
def test_equal_values_of_different_bytes_are_one_group(trim):
    p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=trim)
    rd = FixedLenNestedReader(EQUAL_COPYBOOK, p)
    cb, plan = rd.copybook, rd.plan
    data = equal_records(plan)
    rows = RO.fixed_len_rows(cb, data, p)
    aggs = [A.CountStar(), A.Sum("VP"), A.Min("VP"), A.Max("VZ"), A.Count("VZ"), A.Count("KP"), A.Sum("KP")]
    t1, _ = lut_twins(plan)
    counts = equal_expected_counts(trim)
    if plan.options.lut[t1] == plan.options.lut[0x40]:
        counts["KX4"] -= 1
    t = _device(data)
    for col, want in counts.items():
        exp = expected_groups(cb, plan, rows, [col], aggs)
        got = rd.aggregate_by_device(t, len(data), [col], aggs, max_groups=len(exp))
        assert check_groups(got, exp, aggs) == want, (col, trim, sorted(got.groups, key=repr))
    assert (None,) in expected_groups(cb, plan, rows, ["KP"], aggs) and (None,) in expected_groups(cb, plan, rows, ["KZ"], aggs)
    for group_by in (["KB", "KP", "KX4", "KX3"], ["KZ", "KX3"]):
        for filters in ([], [F.GreaterThan("VP", 0)]):
            exp = expected_groups(cb, plan, rows, group_by, aggs, filters)
            got = rd.aggregate_by_device(t, len(data), group_by, aggs, filters or None, max_groups=len(exp), max_workgroups=1)
            check_groups(got, exp, aggs)
    rd.close()


def test_short_records_cut_a_numeric_and_a_string_key():
    """NUM occupies bytes 4-6, TXT bytes 7-12: records cut inside NUM (NULL key), at TXT's start ("" key), inside TXT,
    in front of both (NULL)."""
    def ebcdic(s):
        return s.encode("cp037")
    full = [ebcdic("AAAA") + bytes([0x12, 0x34, 0x5C]) + ebcdic("abcdef"),
            ebcdic("BBBB") + bytes([0x00, 0x07, 0x7D]) + ebcdic("abc   "),
            ebcdic("CCCC") + bytes([0x99, 0x99, 0x9C]) + ebcdic("  zz  ")]
    recs = [full[k % 3][:cut] for k, cut in enumerate([13, 10, 7, 6, 5, 3, 13, 10, 8, 7, 4, 13, 12, 9])]
    raw = rdw_file(recs)
    p = ReaderParameters(is_record_sequence=True, schema_policy="collapse_root", generate_record_id=True)
    rd = VarLenNestedReader(SHORT_COPYBOOK, p)
    cb = rd.copybook
    rows = RO.var_len_rows(cb, raw, p)
    aggs = [A.CountStar(), A.Count("A")] + [fn("NUM") for fn in ALL_FUNCS] + [A.Count("TXT")]
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    for group_by in (["NUM"], ["TXT"], ["TXT", "NUM"], ["A"]):
        for filters in ([], [F.IsNull("NUM")]):
            exp = expected_groups(cb, rd.plan, rows, group_by, aggs, filters)
            check_groups(rd.aggregate_by(raw, group_by, aggs, filters or None), exp, aggs)
            check_groups(rd.aggregate_by_device(t, vb, (off, ln), group_by, aggs, filters or None, max_groups=len(exp)), exp, aggs)
    exp = expected_groups(cb, rd.plan, rows, ["TXT"], aggs)
    assert (None,) in exp and ("",) in exp and (None,) in expected_groups(cb, rd.plan, rows, ["NUM"], aggs)
    rd.close()


# ---------------------------------------------------------------------------------------------
# SYN200: the fused filter, consistency with the ungrouped call, batches, pass times
# ---------------------------------------------------------------------------------------------
SYN_N = 1000
SYN_AGGS = [A.CountStar()] + [fn(c) for c in ("AMT-01", "ZD-01", "BR-ID") for fn in ALL_FUNCS] + [A.Count("NAME"), A.Count("FX-RATE")]


@pytest.fixture(scope="module")
def syn():
    rd = FixedLenNestedReader(SYN200_COPYBOOK, PARAMS)
    recs = syn200(4096, seed=11, malformed_rate=0.2)
    rows = RO.fixed_len_rows(rd.copybook, recs[:SYN_N].numpy().tobytes(), PARAMS)
    yield rd, recs, rows
    rd.close()


def _own_groups(rd, batch, group_by, aggs):
    """The evaluator over this library's own decoded rows (the rows of decode(filters=))."""
    assert batch.unhandled_filters == []
    return expected_groups(rd.copybook, rd.plan, batch.to_rows(), group_by, aggs)


def test_fused_filter_syn200(syn):
    rd, recs, rows = syn
    cb = rd.copybook
    data = recs[:SYN_N].numpy().tobytes()
    t = _device(data)
    for group_by in (["BR-ID"], ["ZD-01", "NAME"]):
        for key, filters in list(syn_predicates(cb, rows).items()) + [("none", [])]:
            exp = expected_groups(cb, rd.plan, rows, group_by, SYN_AGGS, filters)
            got = rd.aggregate_by_device(t, len(data), group_by, SYN_AGGS, filters or None, max_groups=2048)
            check_groups(got, exp, SYN_AGGS)
            check_groups(got, _own_groups(rd, rd.decode_device(t, len(data), filters=filters or None), group_by, SYN_AGGS), SYN_AGGS)
            assert 0 < got.n_rows <= SYN_N, key
    with pytest.raises(A.Unhandled, match="COMP-1 / COMP-2"):
        rd.aggregate_by_device(t, len(data), ["BR-ID"], [A.CountStar()], [F.GreaterThan("FX-RATE", 1)])
    with pytest.raises(A.Unhandled, match="COMP-1 / COMP-2 key"):
        rd.aggregate_by_device(t, len(data), ["FX-RATE"], [A.CountStar()])


def test_merged_groups_equal_the_ungrouped_aggregate(syn):
    rd, recs, _ = syn
    data = recs.numpy().tobytes()
    t = _device(data)
    for filters in (None, [F.LessThan("AMT-02", 0)]):
        got = rd.aggregate_by_device(t, len(data), ["BR-ID"], SYN_AGGS, filters, max_groups=4096)
        whole = rd.aggregate_device(t, len(data), SYN_AGGS, filters)
        merged = None
        for g in got.groups.values():
            merged = g if merged is None else merged.merge(g)
        assert merged.raw == whole.raw and merged.values == whole.values and len(got.groups) > 1000


def test_three_batches_merge_to_the_single_call(syn):
    rd, recs, rows = syn
    data = recs[:SYN_N].numpy().tobytes()
    t = _device(data)
    f = [F.GreaterThan("AMT-01", 0)]
    whole = rd.aggregate_by_device(t, len(data), ["ZD-01", "NAME"], SYN_AGGS, f, max_groups=1024)
    cuts = [0, 200 * 333, 200 * 397, len(data)]
    a, b, c = (rd.aggregate_by_device(t[x:y], y - x, ["ZD-01", "NAME"], SYN_AGGS, f, max_groups=1024, max_workgroups=mw)
               for (x, y), mw in zip(zip(cuts, cuts[1:]), (0, 1, 2)))
    for m in (a.merge(b).merge(c), c.merge(a.merge(b))):
        assert m.rows() == whole.rows() and {k: g.raw for k, g in m.groups.items()} == {k: g.raw for k, g in whole.groups.items()}
    check_groups(whole, expected_groups(rd.copybook, rd.plan, rows, ["ZD-01", "NAME"], SYN_AGGS, f), SYN_AGGS)


def test_pass_times_only_under_profiling(syn):
    rd, recs, _ = syn
    t = _device(recs[:SYN_N].numpy().tobytes())
    rd.aggregate_by_device(t, SYN_N * 200, ["BR-ID"], SYN_AGGS)
    assert rd.group_pass_times() == (0.0, 0.0, 0.0)
    N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 1))
    try:
        rd.aggregate_by_device(t, SYN_N * 200, ["BR-ID"], SYN_AGGS)
        assert all(x > 0 for x in rd.group_pass_times())
    finally:
        N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 0))


def test_projected_reader_groups_through_its_full_plan(syn):
    _, recs, rows = syn
    rd = FixedLenNestedReader(SYN200_COPYBOOK, PARAMS, columns=["REC-ID"])
    data = recs[:300].numpy().tobytes()
    exp = expected_groups(rd.copybook, rd.plan, rows[:300], ["BR-ID"], SYN_AGGS)
    check_groups(rd.aggregate_by(data, ["BR-ID"], SYN_AGGS), exp, SYN_AGGS)
    rd.close()


# ---------------------------------------------------------------------------------------------
# The variable-length sources
# ---------------------------------------------------------------------------------------------
NARROW_AGGS = [A.CountStar()] + [fn("TAXPAYER-NUM") for fn in ALL_FUNCS] + [A.Count(c) for c in ("COMPANY-NAME", "PHONE-NUMBER")]
NARROW_KEYS = (["SEGMENT-ID"], ["TAXPAYER-TYPE"], ["SEGMENT-ID", "TAXPAYER-TYPE", "TAXPAYER-NUM"])


def test_fused_filter_rdw_narrow():
    """The selection source on the multisegment RDW file (Seg_Id levels, a sparse index): aggregate_by(filters=f) equals
    the evaluator over the oracle's kept rows and over the rows of read(filters=f)."""
    d, _ = rdw_narrow(1000, seed=9)
    raw = d.numpy().tobytes()
    p, _ = parse_options(NARROW_OPTIONS)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    cb = rd.copybook
    rows = RO.var_len_rows(cb, raw, p)
    for filters in list(narrow_cases(cb, rows).values())[:3] + [[]]:
        for group_by in NARROW_KEYS:
            exp = expected_groups(cb, rd.plan, rows, group_by, NARROW_AGGS, filters)
            got = rd.aggregate_by(raw, group_by, NARROW_AGGS, filters or None, max_groups=2048)
            check_groups(got, exp, NARROW_AGGS)
        check_groups(got, _own_groups(rd, rd.read(raw, filters=filters or None), group_by, NARROW_AGGS), NARROW_AGGS)
    assert (None,) in expected_groups(cb, rd.plan, rows, ["TAXPAYER-TYPE"], NARROW_AGGS)
    rd.close()


def test_framed_source_with_the_segment_map():
    p = narrow_params()
    cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(FUZZ_N, 21)
    rows = RO.var_len_rows(cb, raw, p)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert rd.plan.options.has_segments and not rd.plan.seg_id_columns
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    for filters in ([], [F.EqualTo("SEGMENT-ID", "C")]):
        for group_by in NARROW_KEYS:
            exp = expected_groups(cb, rd.plan, rows, group_by, NARROW_AGGS, filters)
            check_groups(rd.aggregate_by_device(t, vb, (off, ln), group_by, NARROW_AGGS, filters or None, max_groups=512), exp,
                         NARROW_AGGS)
    rd.close()


def test_selection_source_segment_filter_and_index_entries():
    opts = dict(NARROW_OPTIONS, segment_filter="C")
    p, _ = parse_options(opts)
    raw = rdw_narrow(1000, seed=9)[0].numpy().tobytes()
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    cb = rd.copybook
    rows = RO.var_len_rows(cb, raw, p)
    assert 0 < len(rows) < 1000
    group_by = ["TAXPAYER-TYPE"]
    whole = rd.aggregate_by(raw, group_by, NARROW_AGGS)
    check_groups(whole, expected_groups(cb, rd.plan, rows, group_by, NARROW_AGGS), NARROW_AGGS)
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    entries = rd.generate_index(t, len(raw), off, ln, 0)
    assert len(entries) > 3
    host_off = off.cpu().numpy()
    merged = None
    for a, b in ((0, 1), (1, 3), (3, len(entries))):
        sub = entries[a:b]
        lo = int(np.searchsorted(host_off, sub[0].offset_from))
        hi = int(np.searchsorted(host_off, entries[b].offset_from)) if b < len(entries) else len(host_off)
        sel = rd.select(t, vb, off[lo:hi], ln[lo:hi], sub, 0)
        part = rd.aggregate_by_device(t, vb, sel, group_by, NARROW_AGGS)
        ids = {r["Record_Id"] for r in rd.decode_selected(t, vb, sel).to_rows()}
        check_groups(part, expected_groups(cb, rd.plan, [r for r in rows if r["Record_Id"] in ids], group_by, NARROW_AGGS), NARROW_AGGS)
        merged = part if merged is None else merged.merge(part)
    assert merged.rows() == whole.rows()
    rd.close()


# ---------------------------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------------------------
def _raw_call(rd, gtable, table, t, n_bytes, n_rec, stride, max_groups=16):
    room = min(max(1, max_groups), 64)        # (a refused max_groups writes nothing)
    n_rows = (ctypes.c_int64 * room)()
    values = (N.CbxAggregateValue * (room * max(1, table.n_terms)))()
    cells = (N.CbxGroupKey * (room * N.CBX_GROUP_MAX_KEYS))()
    key_bytes = (ctypes.c_uint8 * (room * 3 * 32 * N.CBX_GROUP_MAX_KEYS))()
    out = N.CbxGroupOutput(ctypes.addressof(n_rows), ctypes.addressof(values), ctypes.addressof(cells), ctypes.addressof(key_bytes))
    hdr = N.CbxGroupHeader()
    N.check(N.load().cbx_aggregate_grouped(rd.native.handle, t.data_ptr(), n_bytes, None, None, None, n_rec, stride, 0, None,
                                           ctypes.byref(table), ctypes.byref(gtable), max_groups, 0, ctypes.byref(out),
                                           ctypes.byref(hdr), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return hdr


def _tables(keys, terms=()):
    g = N.CbxGroupBy()
    g.n_keys = len(keys)
    for i, k in enumerate(keys):
        g.fields[i] = k
    t = N.CbxAggregate()
    t.n_terms = len(terms)
    for i, (field, funcs) in enumerate(terms):
        t.terms[i].field, t.terms[i].funcs = field, funcs
    return g, t


def test_c_level_refusals(pat_reader, syn):
    rd = FixedLenNestedReader(OCCURS_COPYBOOK, ReaderParameters())
    fi = rd.plan.field_of_node[id(rd.copybook.get_field_by_name("ITEM-NO"))]
    data = torch.zeros(22, dtype=torch.uint8, device="cuda")

    def code(reader, keys, terms=(), n_rec=2, stride=11, t=data, n_bytes=22, **kw):
        with pytest.raises(N.CbxError) as e:
            _raw_call(reader, *_tables(keys, terms), t, n_bytes, n_rec, stride, **kw)
        return e.value.code, str(e.value)

    c, msg = code(rd, [fi])
    assert c == N.CBX_E_UNSUPPORTED and "OCCURS" in msg
    for keys, kw in (([], {}), ([0, 0], {}), ([99], {}), ([0], {"max_groups": 0}), ([0], {"n_rec": 3}),
                     ([0], {"max_groups": 1 << 40})):
        assert code(rd, keys, **kw)[0] == N.CBX_E_ARGUMENT, (keys, kw)
    hdr = _raw_call(rd, *_tables([0], [(0, 15)]), data, 22, 2, 11)
    assert (hdr.n_rows, hdr.n_groups, hdr.overflow) == (2, 1, 0)
    with pytest.raises(A.Unhandled, match="OCCURS"):
        rd.aggregate_by(bytes(22), ["ITEM-NO"], [A.CountStar()])
    rd.close()
    srd, recs, _ = syn
    fx, nm, cust = (srd.plan.field_of_node[id(srd.copybook.get_field_by_name(c))] for c in ("FX-RATE", "NAME", "CUST-KEY"))
    t = _device(recs[:2].numpy().tobytes())
    c, msg = code(srd, [fx], t=t, n_bytes=400, stride=200)
    assert c == N.CBX_E_UNSUPPORTED and "COMP-1 / COMP-2 key" in msg
    c, msg = code(srd, [nm], [(fx, N.AGG_SUM)], t=t, n_bytes=400, stride=200)
    assert c == N.CBX_E_UNSUPPORTED and "COMP-1 / COMP-2" in msg
    big = pat_reader.plan.field_of_node[id(pat_reader.copybook.get_field_by_name("BIG"))]
    pt = _device(pat_record(1, 1, 1, 1, 1) * 2)
    for funcs in (N.AGG_MIN, N.AGG_MAX | N.AGG_SUM):
        c, msg = code(pat_reader, [0], [(big, funcs)], t=pt, n_bytes=2 * PAT_SIZE, stride=PAT_SIZE)
        assert c == N.CBX_E_UNSUPPORTED and "DEC128" in msg
    assert _raw_call(pat_reader, *_tables([0], [(big, N.AGG_COUNT | N.AGG_SUM)]), pt, 2 * PAT_SIZE, 2, PAT_SIZE).n_groups == 1
    with pytest.raises(A.Unhandled, match="DEC128"):
        pat_reader.aggregate_by_device(pt, 2 * PAT_SIZE, ["K"], [A.Min("BIG")])
    hdr = _raw_call(srd, *_tables([cust]), t, 400, 2, 200, max_groups=1)      # two keys, room for one: the flag, status OK
    assert hdr.overflow == 1
    long_rd = FixedLenNestedReader("       01  R.\n           05  S33  PIC X(33).\n", ReaderParameters())
    c, msg = code(long_rd, [0], t=torch.zeros(66, dtype=torch.uint8, device="cuda"), n_bytes=66, stride=33)
    assert c == N.CBX_E_UNSUPPORTED and "longer than 32" in msg
    long_rd.close()


def test_hierarchical_reader_raises():
    opts = {"is_record_sequence": "true", "segment_field": "SEGMENT_ID",
            "redefine_segment_id_map:1": "STATIC-DETAILS => C", "redefine-segment-id-map:2": "CONTACTS => P",
            "segment-children:1": "STATIC-DETAILS => CONTACTS"}
    p, _ = parse_options(opts)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert rd.hierarchical
    raw = rdw_narrow(50, seed=4)[0].numpy().tobytes()
    with pytest.raises(N.CbxError) as e:
        rd.aggregate_by(raw, ["SEGMENT-ID"], [A.CountStar()])
    assert e.value.code == N.CBX_E_UNSUPPORTED
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    with pytest.raises(N.CbxError) as e:
        rd.aggregate_by_device(t, vb, (off, ln), ["SEGMENT-ID"], [A.CountStar()])
    assert e.value.code == N.CBX_E_UNSUPPORTED
    rd.close()
