"""Aggregate pushdown on the GPU (cbx_aggregate_records) against the contract: COUNT(*), COUNT, MIN, MAX and SUM
over the rows the filters keep equal the Python evaluator of test_aggregate.py (exact ints and Decimals) over
the ORACLE's rows -- never the code under test -- and over this library's own decoded rows; sums are compared
bit for bit (the accumulators are exact), Spark's result types value for value.
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
from cobrix_amd.reader import (FixedLenNestedReader, ReaderParameters, VarLenNestedReader,  # noqa: E402
                               parse_copybook_for)
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, SYN200_COPYBOOK, rdw_file, rdw_narrow, syn200  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_aggregate import (ALL_FUNCS, ASCII_RESTRICTED, FUZZ_RESTRICTED, LADDER_RESTRICTED, NARROW_RESTRICTED,  # noqa: E402
                            SYN_RESTRICTED, check_aggregates, expected_aggregates)
from test_decode_fuzz import ASCII_COPYBOOK, FUZZ_COPYBOOK  # noqa: E402
from test_filter import (FUZZ_N, LADDER_COPYBOOK, ascii_records, fuzz_records, ladder_file, ladder_params,  # noqa: E402
                         narrow_file, narrow_params, py_keep, row_value)
from test_gpu_filter import (FUZZ_GPU_OPTIONS, NARROW_OPTIONS, OCCURS_COPYBOOK, SHORT_COPYBOOK, narrow_cases,  # noqa: E402
                             syn_predicates)


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


def _fixed_fn(rd, t, n_bytes, filters=(), max_workgroups=0):
    return lambda aggs: rd.aggregate_device(t, n_bytes, aggs, list(filters) or None, max_workgroups=max_workgroups)


# ---------------------------------------------------------------------------------------------
# Fixed-length SYN200, a fifth of the numeric fields malformed
# ---------------------------------------------------------------------------------------------
SYN_N = 1000
SYN_PARAMS = ReaderParameters(schema_policy="collapse_root")


@pytest.fixture(scope="module")
def syn():
    """(reader, records [SYN_N, 200], oracle rows of all of them) -- computed once, shared, never changed."""
    rd = FixedLenNestedReader(SYN200_COPYBOOK, SYN_PARAMS)
    recs = syn200(SYN_N, seed=11, malformed_rate=0.2)
    rows = RO.fixed_len_rows(rd.copybook, recs.numpy().tobytes(), SYN_PARAMS)
    assert len(rows) == SYN_N
    yield rd, recs, rows
    rd.close()


@pytest.mark.parametrize("n,max_workgroups,odd", [(0, 0, False), (1, 0, False), (63, 0, False), (64, 0, False),
                                                  (65, 0, False), (255, 0, False), (257, 0, False), (1000, 0, False),
                                                  (1000, 1, False), (1000, 2, False), (1000, 3, False), (1000, 0, True)])
def test_syn200_every_field(syn, n, max_workgroups, odd):
    """Every numeric field with all four functions and COUNT of the string and COMP-2 fields: a partial last tile
    (63, 65, 255, 257, 1000), a workgroup with idle waves (65: two tiles for four waves), two workgroups (257),
    and 16 tiles on 1, 2 and 3 workgroups -- four, two and two grid-stride rounds; at an odd device address."""
    rd, recs, rows = syn
    data = recs[:n].numpy().tobytes()
    t = _device(data, odd)
    fn = _fixed_fn(rd, t, len(data), max_workgroups=max_workgroups)
    mixed = n >= 255
    assert check_aggregates(rd.copybook, rd.plan, rows[:n], fn, (), SYN_RESTRICTED, require_mixed=mixed) > 100
    # and against this library's own decode of the same bytes
    own = rd.decode_device(t, len(data)).to_rows()
    assert len(own) == n
    assert check_aggregates(rd.copybook, rd.plan, own, fn, (), SYN_RESTRICTED, require_mixed=mixed) > 100
    if n == 0:
        r = fn([A.CountStar(), A.Sum("AMT-01"), A.Count("NAME")])
        assert r.values == [0, None, 0] and r.raw["terms"][0] == {"field": r.raw["terms"][0]["field"], "count": 0,
                                                                  "min": None, "max": None, "sum": None}


def test_syn200_host_bytes_entry_point(syn):
    rd, recs, rows = syn
    data = recs[:130].numpy().tobytes()
    aggs = [A.CountStar(), A.Min("AMT-01"), A.Max("AMT-01"), A.Sum("AMT-01"), A.Count("AMT-01"), A.Sum("BR-ID")]
    n_rows, values, _ = expected_aggregates(rd.copybook, rd.plan, rows[:130], aggs)
    got = rd.aggregate(data, aggs)
    assert got.n_rows == n_rows == 130 and got.values == values
    with pytest.raises(ValueError):
        rd.aggregate(data[:-1], aggs)            # the file-size rule of decode()


# ---------------------------------------------------------------------------------------------
# Extremes: 38-digit decimals, longs at the 64-bit boundary, all-null and one-value columns
# ---------------------------------------------------------------------------------------------
EXTREME_COPYBOOK = """
       01  R.
           05  BIG   PIC S9(38) COMP-3.
           05  LNG   PIC S9(18) COMP.
           05  INT   PIC S9(9) COMP.
           05  NUL   PIC S9(7) COMP-3.
           05  ONE   PIC S9(5) COMP-3.
"""
TOP38 = 10 ** 38 - 1


def _bcd(v: int, size: int) -> bytes:
    nib = [int(c) for c in str(abs(v)).rjust(2 * size - 1, "0")] + [0xD if v < 0 else 0xC]
    return bytes((nib[2 * j] << 4) | nib[2 * j + 1] for j in range(size))


def _extreme_record(big: int, lng: int, i: int, one=None) -> bytes:
    """NUL is malformed in every record (sign nibble F on a signed field is fine: digits A-F are not), ONE malformed
    unless given."""
    return _bcd(big, 20) + lng.to_bytes(8, "big", signed=True) + i.to_bytes(4, "big", signed=True) + b"\xff\xff\xff\xff" + \
        (_bcd(one, 3) if one is not None else b"\x00\x00\x00")


@pytest.fixture(scope="module")
def extreme_reader():
    rd = FixedLenNestedReader(EXTREME_COPYBOOK, SYN_PARAMS)
    assert rd.get_record_size() == 39
    yield rd
    rd.close()


EXTREME_AGGS = [A.CountStar()] + [fn(c) for c in ("BIG", "LNG", "INT", "NUL", "ONE") for fn in ALL_FUNCS]


def _extreme_check(rd, data):
    rows = RO.fixed_len_rows(rd.copybook, data, SYN_PARAMS)
    n_rows, values, raw = expected_aggregates(rd.copybook, rd.plan, rows, EXTREME_AGGS)
    got = rd.aggregate(data, EXTREME_AGGS)
    assert got.n_rows == n_rows == len(data) // 39
    by_name = {c: got.raw["terms"][k] for k, c in enumerate(("BIG", "LNG", "INT", "NUL", "ONE"))}
    for c, e in raw.items():
        t = by_name[c]
        assert (t["count"], t["min"], t["max"], t["sum"]) == (e["count"], e["min"], e["max"], e["sum"]), (c, t, e)
    assert got.values == values
    return rows, by_name, dict(zip(EXTREME_AGGS, got.values))


@pytest.mark.parametrize("sign", [1, -1])
def test_extreme_sum_uses_the_third_limb(extreme_reader, sign):
    """600 rows of +(10^38 - 1), and of -(10^38 - 1): |sum| = 6 * 10^40 - 600 > 2^127, so the 192-bit sum's third limb
    carries it; Spark's decimal(38, 0) sum overflows to null.  NUL is null in every row."""
    data = b"".join(_extreme_record(sign * TOP38, 0, 0) for _ in range(600))
    rows, terms, values = _extreme_check(extreme_reader, data)
    assert all(r["BIG"] == sign * TOP38 and r["NUL"] is None for r in rows)
    assert terms["BIG"]["sum"] == sign * 600 * TOP38 and abs(terms["BIG"]["sum"]) > 2 ** 127
    assert values[A.Sum("BIG")] is None and values[A.Min("BIG")] == values[A.Max("BIG")] == Decimal(sign * TOP38)
    assert terms["NUL"] == {"field": terms["NUL"]["field"], "count": 0, "min": None, "max": None, "sum": None}
    assert [values[fn("NUL")] for fn in ALL_FUNCS] == [0, None, None, None]


def test_extreme_long_sum_wraps(extreme_reader):
    """10 rows of 10^18 - 1 in the long column: the exact sum exceeds 2^63, Spark's long sum is its low 64 bits."""
    v = 10 ** 18 - 1
    data = b"".join(_extreme_record(1, v, 7) for _ in range(10))
    rows, terms, values = _extreme_check(extreme_reader, data)
    assert all(r["LNG"] == v for r in rows)
    assert terms["LNG"]["sum"] == 10 * v > 2 ** 63
    assert values[A.Sum("LNG")] == 10 * v - 2 ** 64 < 0 and values[A.Sum("INT")] == 70


def test_extreme_alternating_signs_and_one_value_in_the_last_lane(extreme_reader):
    """640 rows (ten whole tiles) alternating the most negative and most positive values of each column: MIN / MAX
    across the 64-bit boundary (DEC128), at the int64 and int32 limits; ONE has a single non-null value, in the
    last lane of the last tile."""
    n = 640
    recs = [_extreme_record(-TOP38, -2 ** 63, -2 ** 31) if i % 2 == 0 else _extreme_record(TOP38, 2 ** 63 - 1, 2 ** 31 - 1,
                                                                                           one=-4321 if i == n - 1 else None)
            for i in range(n)]
    rows, terms, values = _extreme_check(extreme_reader, b"".join(recs))
    assert [r["ONE"] for r in rows[-2:]] == [None, -4321] and sum(r["ONE"] is not None for r in rows) == 1
    assert rows[0]["LNG"] == -2 ** 63 and rows[1]["LNG"] == 2 ** 63 - 1 and rows[0]["INT"] == -2 ** 31
    assert (terms["BIG"]["min"], terms["BIG"]["max"], terms["BIG"]["sum"]) == (-TOP38, TOP38, 0)
    assert (terms["LNG"]["min"], terms["LNG"]["max"], terms["LNG"]["sum"]) == (-2 ** 63, 2 ** 63 - 1, -320)
    assert (terms["INT"]["min"], terms["INT"]["max"], terms["INT"]["sum"]) == (-2 ** 31, 2 ** 31 - 1, -320)
    assert terms["ONE"]["count"] == 1 and terms["ONE"]["min"] == terms["ONE"]["max"] == terms["ONE"]["sum"] == -4321
    assert values[A.Min("ONE")] == values[A.Sum("ONE")] == -4321 and values[A.Count("ONE")] == 1


# ---------------------------------------------------------------------------------------------
# The fused filter
# ---------------------------------------------------------------------------------------------
SYN_FILTER_AGGS = [A.CountStar()] + [fn(c) for c in ("AMT-01", "ACCT-NO", "ZD-01", "BR-ID", "QTY-01") for fn in ALL_FUNCS] + \
    [A.Count("NAME"), A.Count("FX-RATE")]


def _filtered_check(rd, cb, aggs, got, batch, oracle_rows, filters):
    own = batch.to_rows()
    assert batch.unhandled_filters == []
    assert got.n_rows == batch.n_rec == len(own)
    for rows in (own, [r for r in oracle_rows if py_keep(cb, r, filters)]):
        n_rows, values, _ = expected_aggregates(cb, rd.plan, rows, aggs)
        assert got.n_rows == n_rows and got.values == values, (filters, got.values, values)
    return got.n_rows


def test_fused_filter_syn200(syn):
    """The predicate families of test_gpu_filter.py: aggregate(filters=f) equals the evaluator over the rows of
    decode(filters=f) (and over the oracle's kept rows); n_rows is that batch's n_rec."""
    rd, recs, rows = syn
    cb = rd.copybook
    data = recs.numpy().tobytes()
    t = _device(data)
    kept = {}
    for key, filters in syn_predicates(cb, rows).items():
        got = rd.aggregate_device(t, len(data), SYN_FILTER_AGGS, filters)
        kept[key] = _filtered_check(rd, cb, SYN_FILTER_AGGS, got, rd.decode_device(t, len(data), filters=filters), rows, filters)
    assert all(0 < k < SYN_N for k in kept.values()), kept
    # keep-all, keep-none, keep-one (the last record: the last lane of a partial tile)
    ids = [row_value(cb, r, "REC-ID") for r in rows]
    absent = next(v for v in range(10 ** 9) if v not in set(ids))
    for f, k in ((F.Not(F.In("REC-ID", [absent])), SYN_N), (F.In("REC-ID", [absent]), 0), (F.In("REC-ID", [ids[-1]]), 1),
                 (F.In("REC-ID", [ids[0], ids[64]]), 2)):
        got = rd.aggregate_device(t, len(data), SYN_FILTER_AGGS, [f], max_workgroups=2)
        assert _filtered_check(rd, cb, SYN_FILTER_AGGS, got, rd.decode_device(t, len(data), filters=[f]), rows, [f]) == k
        if k == 0:
            assert got.values == [0] + [0, None, None, None] * 5 + [0, 0]


def test_unhandled_filter_makes_the_whole_call_unhandled(syn):
    rd, recs, rows = syn
    t = _device(recs[:64].numpy().tobytes())
    with pytest.raises(A.Unhandled, match="COMP-1 / COMP-2"):
        rd.aggregate_device(t, 64 * 200, [A.CountStar()], [F.IsNull("AMT-02"), F.GreaterThan("FX-RATE", 1)])
    with pytest.raises(A.Unhandled, match="string field"):
        rd.aggregate_device(t, 64 * 200, [A.CountStar(), A.Min("NAME")])
    assert rd.aggregate_device(t, 64 * 200, [A.CountStar()], [F.IsNull("AMT-02")]).n_rows == \
        sum(r["AMT_02"] is None for r in rows[:64])


@pytest.fixture(scope="module")
def narrow():
    """The multisegment RDW file of test_gpu_filter.py: Seg_Id levels, record ids, a sparse index."""
    d, hdr = rdw_narrow(1000, seed=9)
    raw = bytearray(d.numpy().tobytes())
    c_recs = [int(h) for h in hdr.tolist() if raw[int(h) + 4] == 0xC3]
    for k, h in enumerate(c_recs[::2]):
        raw[h + 4 + 56:h + 4 + 60] = (1000 + 37 * k).to_bytes(4, "big")
    raw = bytes(raw)
    p, var_len = parse_options(NARROW_OPTIONS)
    assert var_len
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    rows = RO.var_len_rows(rd.copybook, raw, p)
    assert len(rows) > 900
    yield rd, p, raw, rows
    rd.close()


NARROW_AGGS = [A.CountStar()] + [fn("TAXPAYER-NUM") for fn in ALL_FUNCS] + \
    [A.Count(c) for c in ("SEGMENT-ID", "COMPANY-NAME", "PHONE-NUMBER", "CONTACT-PERSON", "TAXPAYER-STR")]


def test_fused_filter_rdw_narrow(narrow):
    """read(filters=f) rows against aggregate(filters=f) on the narrow RDW file (the selection source: segments
    from select()); fields of the inactive redefine are null."""
    rd, p, raw, rows = narrow
    cb = rd.copybook
    for key, filters in narrow_cases(cb, rows).items():
        got = rd.aggregate(raw, NARROW_AGGS, filters)
        k = _filtered_check(rd, cb, NARROW_AGGS, got, rd.read(raw, filters=filters), rows, filters)
        assert 0 < k < len(rows), key
    got = rd.aggregate(raw, NARROW_AGGS)
    _filtered_check(rd, cb, NARROW_AGGS, got, rd.read(raw), rows, [])
    v = dict(zip(NARROW_AGGS, got.values))
    c, ph = (sum(r[g] is not None for r in rows) for g in ("STATIC_DETAILS", "CONTACTS"))
    assert v[A.Count("COMPANY-NAME")] == c and v[A.Count("PHONE-NUMBER")] == ph and c + ph == len(rows) == v[A.Count("SEGMENT-ID")]
    assert 0 < v[A.Count("TAXPAYER-NUM")] < c


# ---------------------------------------------------------------------------------------------
# Variable-length sources
# ---------------------------------------------------------------------------------------------
def test_rdw_narrow_framed_source_with_segment_map():
    """Framed records, segment_field and the redefine map but no Seg_Id levels: the active segment comes from the
    plan's segment map; some records carry an id the map does not name (both redefines null)."""
    p = narrow_params()
    cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(FUZZ_N, 21)
    rows = RO.var_len_rows(cb, raw, p)
    assert any(r["STATIC_DETAILS"] is None and r["CONTACTS"] is None for r in rows)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert rd.plan.options.has_segments and not rd.plan.seg_id_columns
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    for filters in ([], [F.EqualTo("SEGMENT-ID", "C")], [F.IsNotNull("PHONE-NUMBER")]):
        fn = lambda aggs: rd.aggregate_device(t, vb, (off, ln), aggs, filters or None)   # noqa: E731
        assert check_aggregates(cb, rd.plan, rows, fn, filters, NARROW_RESTRICTED, require_mixed=False) > 6
        assert fn(NARROW_AGGS).values == rd.aggregate(raw, NARROW_AGGS, filters or None).values   # the selection source
    got = rd.aggregate_device(t, vb, (off, ln), NARROW_AGGS)
    c = sum(r["STATIC_DETAILS"] is not None for r in rows)
    assert got.n_rows == FUZZ_N and 0 < got.values[1] < c < FUZZ_N     # 0 < count < n_rows
    rd.close()


def test_framed_source_on_a_reader_with_segment_levels(narrow):
    """Unlike the filter stage, framed records are taken on a reader with Seg_Id levels (no Seg_Id state is carried)."""
    rd, p, raw, rows = narrow
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    assert rd.plan.seg_id_columns
    f = [F.EqualTo("SEGMENT-ID", "C")]
    assert rd.aggregate_device(t, vb, (off, ln), NARROW_AGGS, f).values == rd.aggregate(raw, NARROW_AGGS, f).values


def test_selection_source_segment_filter_and_index_entries():
    """segment_filter drops records in select(); a subset of the sparse-index entries selects part of the file: the
    aggregate runs over exactly the rows decode_selected returns for the same selection."""
    opts = dict(NARROW_OPTIONS, segment_filter="C")
    p, _ = parse_options(opts)
    raw = rdw_narrow(1000, seed=9)[0].numpy().tobytes()
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    cb = rd.copybook
    rows = RO.var_len_rows(cb, raw, p)
    assert 0 < len(rows) < 1000 and all(r["STATIC_DETAILS"] is not None for r in rows)
    got = rd.aggregate(raw, NARROW_AGGS)
    _filtered_check(rd, cb, NARROW_AGGS, got, rd.read(raw), rows, [])
    assert got.values[5] == got.n_rows == len(rows) and got.values[7] == 0      # SEGMENT-ID count; no PHONE-NUMBER
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    entries = rd.generate_index(t, len(raw), off, ln, 0)
    assert len(entries) > 3
    parts = []
    host_off = off.cpu().numpy()
    for a, b in ((0, 1), (1, 3), (3, len(entries))):
        # the framed records of entries [a, b): from the first entry's offset up to the next entry's
        sub = entries[a:b]
        lo = int(np.searchsorted(host_off, sub[0].offset_from))
        hi = int(np.searchsorted(host_off, entries[b].offset_from)) if b < len(entries) else len(host_off)
        sel = rd.select(t, vb, off[lo:hi], ln[lo:hi], sub, 0)
        part = rd.aggregate_device(t, vb, sel, NARROW_AGGS)
        own = rd.decode_selected(t, vb, sel).to_rows()
        ids = {r["Record_Id"] for r in own}
        assert 0 < len(own) < len(rows)
        _filtered_check(rd, cb, NARROW_AGGS, part, rd.decode_selected(t, vb, sel), [r for r in rows if r["Record_Id"] in ids], [])
        parts.append(part)
    merged = parts[0].merge(parts[1]).merge(parts[2])
    assert merged.raw == got.raw and merged.values == got.values
    rd.close()


def test_short_records_cut_a_numeric_and_a_string_field():
    """NUM occupies bytes 4-6, TXT bytes 7-12 (test_gpu_filter.SHORT_COPYBOOK): records cut inside NUM (null), at
    TXT's start (an empty string: counted), inside TXT (counted), in front of both."""
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
    assert sum(r["NUM"] is None for r in rows) == 4 and sum(r["TXT"] is None for r in rows) > 0
    aggs = [A.CountStar(), A.Count("A")] + [fn("NUM") for fn in ALL_FUNCS] + [A.Count("TXT")]
    for filters in ([], [F.LessThan("TXT", "b")], [F.IsNull("NUM")]):
        got = rd.aggregate(raw, aggs, filters or None)
        _filtered_check(rd, cb, aggs, got, rd.read(raw, filters=filters or None), rows, filters)
        t = rd._device_file(raw)
        off, ln, vb = rd.frame_file(t, len(raw))
        assert rd.aggregate_device(t, vb, (off, ln), aggs, filters or None).values == got.values
    got = rd.aggregate(raw, aggs)
    assert got.values[0] == 14 and got.values[2] == 10 and got.values[3] < 0 < got.values[4] and 0 < got.values[6] < 14
    rd.close()


# ---------------------------------------------------------------------------------------------
# Every decoder kind
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code_page,trim,fmt", FUZZ_GPU_OPTIONS)
def test_fuzz_copybook_every_field(code_page, trim, fmt):
    """Every zoned / binary / COMP-3 shape of the decode fuzz, 321 records (two workgroups, the second with one
    record), COUNT of three strings and two floats; plain, filtered, and at an odd device address on one workgroup."""
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim,
                         floating_point_format=fmt)
    cb = parse_copybook_for(FUZZ_COPYBOOK, p)
    data = fuzz_records(cb, FUZZ_N, 31)
    rows = RO.fixed_len_rows(cb, data, p)
    assert len(rows) == FUZZ_N
    rd = FixedLenNestedReader(FUZZ_COPYBOOK, p)
    for filters, odd, mw in (([], False, 0), ([F.GreaterThan("B05", 0)], False, 0), ([], True, 1)):
        t = _device(data, odd)
        n = check_aggregates(cb, rd.plan, rows, _fixed_fn(rd, t, len(data), filters, mw), filters, FUZZ_RESTRICTED)
        assert n > 4 * 60
    rd.close()


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_ascii_copybook_every_field(charset):
    p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
    cb = parse_copybook_for(ASCII_COPYBOOK, p)
    data = ascii_records(cb, FUZZ_N, 32)
    rows = RO.fixed_len_rows(cb, data, p)
    rd = FixedLenNestedReader(ASCII_COPYBOOK, p)
    t = _device(data)
    for filters in ([], [F.GreaterThan("A02", 0)]):
        assert check_aggregates(cb, rd.plan, rows, _fixed_fn(rd, t, len(data), filters), filters, ASCII_RESTRICTED) > 40
    rd.close()


@pytest.mark.parametrize("trim", ["none", "both"])
def test_width_ladder_cut_at_every_length(trim):
    """One ladder record per length 1..L (framed source): every numeric field cut inside at every byte is null, every
    string that starts inside the record counts."""
    p = ladder_params(trim)
    cb = parse_copybook_for(LADDER_COPYBOOK, p)
    raw, _, ln = ladder_file(seed=34, every_length=True)
    assert ln.tolist() == list(range(1, cb.record_size + 1))
    rows = RO.var_len_rows(cb, raw, p)
    rd = VarLenNestedReader(LADDER_COPYBOOK, p)
    t = rd._device_file(raw)
    off, dl, vb = rd.frame_file(t, len(raw))
    for filters in ([], [F.IsNotNull("P08")]):
        fn = lambda aggs: rd.aggregate_device(t, vb, (off, dl), aggs, filters or None)   # noqa: E731
        assert check_aggregates(cb, rd.plan, rows, fn, filters, LADDER_RESTRICTED) > 4 * 38
    rd.close()


# ---------------------------------------------------------------------------------------------
# Batches, profiling, refusals
# ---------------------------------------------------------------------------------------------
def test_three_batches_merge_to_the_single_call(syn):
    rd, recs, rows = syn
    data = recs.numpy().tobytes()
    t = _device(data)
    f = [F.GreaterThan("AMT-01", 0)]
    whole = rd.aggregate_device(t, len(data), SYN_FILTER_AGGS, f)
    cuts = [0, 200 * 333, 200 * 397, len(data)]
    parts = [rd.aggregate_device(t[a:b], b - a, SYN_FILTER_AGGS, f, max_workgroups=mw) for (a, b), mw in zip(zip(cuts, cuts[1:]), (0, 1, 2))]
    assert all(p.n_rows > 0 for p in parts)
    for m in (parts[0].merge(parts[1]).merge(parts[2]), parts[0].merge(parts[1].merge(parts[2])),
              parts[2].merge(parts[0]).merge(parts[1])):
        assert m.raw == whole.raw and m.values == whole.values
    n_rows, values, _ = expected_aggregates(rd.copybook, rd.plan, rows, SYN_FILTER_AGGS, f)
    assert whole.n_rows == n_rows and whole.values == values


def test_pass_times_only_under_profiling(syn):
    rd, recs, rows = syn
    t = _device(recs.numpy().tobytes())
    rd.aggregate_device(t, SYN_N * 200, SYN_FILTER_AGGS)
    assert rd.aggregate_pass_times() == (0.0, 0.0)
    N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 1))
    try:
        rd.aggregate_device(t, SYN_N * 200, SYN_FILTER_AGGS)
        acc, comb = rd.aggregate_pass_times()
        assert acc > 0 and comb > 0
    finally:
        N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 0))


def _raw_call(rd, table, t, n_bytes, n_rec, stride, max_workgroups=0):
    res = N.CbxAggregateResult()
    N.check(N.load().cbx_aggregate_records(rd.native.handle, t.data_ptr(), n_bytes, None, None, None, n_rec, stride, 0, None,
                                           ctypes.byref(table), max_workgroups, ctypes.byref(res),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return res


def _table(*terms):
    t = N.CbxAggregate()
    t.n_terms = len(terms)
    for i, (field, funcs) in enumerate(terms):
        t.terms[i].field, t.terms[i].funcs = field, funcs
    return t


def test_c_level_refusals(syn):
    rd = FixedLenNestedReader(OCCURS_COPYBOOK, ReaderParameters())
    fi = rd.plan.field_of_node[id(rd.copybook.get_field_by_name("ITEM-NO"))]
    data = torch.zeros(22, dtype=torch.uint8, device="cuda")
    with pytest.raises(N.CbxError) as e:
        _raw_call(rd, _table((fi, N.AGG_SUM)), data, 22, 2, 11)
    assert e.value.code == N.CBX_E_UNSUPPORTED and "OCCURS" in str(e.value)
    for table in (_table((99, N.AGG_COUNT)), _table((0, 0)), _table((0, 1), (0, 2))):
        with pytest.raises(N.CbxError) as e:
            _raw_call(rd, table, data, 22, 2, 11)
        assert e.value.code == N.CBX_E_ARGUMENT
    with pytest.raises(N.CbxError) as e:
        _raw_call(rd, _table((0, 15)), data, 22, 3, 11)       # three records of 11 bytes exceed 22
    assert e.value.code == N.CBX_E_ARGUMENT
    assert _raw_call(rd, _table((0, 15)), data, 22, 2, 11).n_rows == 2
    with pytest.raises(A.Unhandled, match="OCCURS"):
        rd.aggregate(bytes(22), [A.Sum("ITEM-NO")])
    rd.close()
    # SUM on COMP-2
    srd, recs, _ = syn
    fx = srd.plan.field_of_node[id(srd.copybook.get_field_by_name("FX-RATE"))]
    t = _device(recs[:2].numpy().tobytes())
    with pytest.raises(N.CbxError) as e:
        _raw_call(srd, _table((fx, N.AGG_SUM)), t, 400, 2, 200)
    assert e.value.code == N.CBX_E_UNSUPPORTED and "COMP-1 / COMP-2" in str(e.value)
    assert _raw_call(srd, _table((fx, N.AGG_COUNT)), t, 400, 2, 200).n_rows == 2
    # a record-walk plan
    wide = """
       01  REC.
           05  CNT           PIC 9(2).
           05  VALS  PIC 9(2) OCCURS 0 TO 4 TIMES DEPENDING ON CNT.
           05  NAME          PIC X(8).
"""
    wrd = FixedLenNestedReader(wide, ReaderParameters(variable_size_occurs=True))
    assert wrd.walk
    nm = wrd.plan.field_of_node[id(wrd.copybook.get_field_by_name("NAME"))]
    size = wrd.get_record_size()
    wt = torch.zeros(2 * size, dtype=torch.uint8, device="cuda")
    with pytest.raises(N.CbxError) as e:
        _raw_call(wrd, _table((nm, N.AGG_COUNT)), wt, 2 * size, 2, size)
    assert e.value.code == N.CBX_E_UNSUPPORTED and "record-walk" in str(e.value)
    with pytest.raises(A.Unhandled, match="data-dependent"):
        wrd.aggregate_device(wt, 2 * size, [A.Count("NAME")])
    wrd.close()


def test_hierarchical_reader_raises():
    opts = {"is_record_sequence": "true", "segment_field": "SEGMENT_ID",
            "redefine_segment_id_map:1": "STATIC-DETAILS => C", "redefine-segment-id-map:2": "CONTACTS => P",
            "segment-children:1": "STATIC-DETAILS => CONTACTS"}
    p, _ = parse_options(opts)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert rd.hierarchical
    raw = rdw_narrow(50, seed=4)[0].numpy().tobytes()
    with pytest.raises(N.CbxError) as e:
        rd.aggregate(raw, [A.CountStar()])
    assert e.value.code == N.CBX_E_UNSUPPORTED
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    with pytest.raises(N.CbxError) as e:
        rd.aggregate_device(t, vb, (off, ln), [A.CountStar()])
    assert e.value.code == N.CBX_E_UNSUPPORTED
    rd.close()


def test_projected_reader_aggregates_through_its_full_plan(syn):
    _, recs, rows = syn
    rd = FixedLenNestedReader(SYN200_COPYBOOK, SYN_PARAMS, columns=["REC-ID"])
    data = recs[:300].numpy().tobytes()
    f = [F.GreaterThan("AMT-01", 0)]
    n_rows, values, _ = expected_aggregates(rd.copybook, rd.plan, rows[:300], SYN_FILTER_AGGS, f)
    got = rd.aggregate(data, SYN_FILTER_AGGS, f)
    assert got.n_rows == n_rows and got.values == values and 0 < n_rows < 300
    rd.close()
