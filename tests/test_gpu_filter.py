"""Row filters on the GPU (cbx_filter_records -> cbx_decode_selected) against the contract: the filtered
read returns exactly the rows of the unfiltered ORACLE read that the filters keep under SQL three-valued
logic (test_filter.py py_keep over the oracle's rows -- never the code under test), in file order, every
value identical, generated ids included.
"""
from __future__ import annotations

import random
from decimal import Decimal

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.options import parse_options  # noqa: E402
from cobrix_amd.reader import (FixedLenNestedReader, ReaderParameters, VarLenNestedReader,  # noqa: E402
                               parse_copybook_for)
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, SYN200_COPYBOOK, rdw_file, rdw_narrow, syn200  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from parity import compare_batch  # noqa: E402
from test_decode_fuzz import ASCII_COPYBOOK, FUZZ_COPYBOOK  # noqa: E402
from test_filter import (FUZZ_N, LADDER_COPYBOOK, NARROW_SEGMENTS, ascii_records, check_field_filters,  # noqa: E402
                         expected_keep, field_filters, fuzz_records, ladder_file, ladder_params, narrow_file,
                         narrow_params, py_keep, row_value)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check(got, exp_all, cb, filters, unhandled=()):
    exp = [r for r in exp_all if py_keep(cb, r, filters)]
    assert list(unhandled) == []
    assert len(got) == len(exp), (filters, len(got), len(exp))
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if a != b]
    assert not bad, (filters, bad[:5], got[bad[0]], exp[bad[0]])
    return len(exp)


# ---------------------------------------------------------------------------------------------
# Fixed-length SYN200, a fifth of the numeric fields malformed
# ---------------------------------------------------------------------------------------------
SYN_N = 4097
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


def _decode(rd, data: bytes, filters):
    """decode_device over the records in HBM (decode() refuses an empty file, as the reference does)."""
    t = torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()
    return rd.decode_device(t, len(data), filters=filters)


def _valid(cb, rows, name, start=0):
    return next(v for v in (row_value(cb, r, name) for r in rows[start:]) if v is not None)


def syn_predicates(cb, rows):
    """One predicate per decoder kind (binary int32 / int64, COMP-3 decimal, zoned int / decimal, cp037
    string), null tests, an OR group and a conjunction; literals are decoded values of the data."""
    acct = sorted(v for v in (row_value(cb, r, "ACCT-NO") for r in rows) if v is not None)
    name = next(v for v in (row_value(cb, r, "NAME") for r in rows[3:]) if len(v) >= 2)
    return {
        "br_in": [F.In("BR-ID", [_valid(cb, rows, "BR-ID", k) for k in (0, 5, 70)])],
        "acct_range": [F.GreaterThanOrEqual("ACCT-NO", acct[len(acct) // 4]), F.LessThan("ACCT-NO", acct[len(acct) // 2])],
        "amt_gt": [F.GreaterThan("AMT-01", Decimal("1234567.89"))],
        "zn_eq": [F.EqualTo("ZN-01", _valid(cb, rows, "ZN-01", 2))],
        "zd_lt": [F.LessThan("ZD-01", Decimal("-100.5"))],
        "name_eq": [F.EqualTo("NAME", name)],
        "name_empty": [F.EqualTo("NAME", "")],
        "name_lt": [F.LessThan("NAME", "M")],
        "name_starts": [F.StringStartsWith("NAME", name[:1])],
        "name_not_starts": [F.Not(F.StringStartsWith("NAME", name[:1]))],
        "amt2_null": [F.IsNull("AMT-02")],
        "or_group": [F.Or(F.EqualTo("BR-ID", _valid(cb, rows, "BR-ID", 1)), F.IsNull("QTY-01"))],
        "three_terms": [F.GreaterThan("AMT-01", 0), F.LessThan("ZD-01", 0), F.IsNotNull("RATE-01")],
    }


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, SYN_N])
def test_syn200_predicates(syn, n):
    rd, recs, rows = syn
    data = recs[:n].numpy().tobytes()
    kept = {}
    for key, filters in syn_predicates(rd.copybook, rows).items():
        b = _decode(rd, data, filters)
        kept[key] = _check(b.to_rows(), rows[:n], rd.copybook, filters, b.unhandled_filters)
    if n == SYN_N:   # the predicates separate rows: each keeps some and drops some
        assert all(0 < k < n for k in kept.values()), kept


def test_syn200_unaligned_data_pointer(syn):
    """Records that start at an odd device address (a batch cut out of a larger buffer): the 8- and 16-byte
    loads of the SWAR decoders and of the string image take any alignment."""
    rd, recs, rows = syn
    t = torch.zeros(200 * 67 + 9, dtype=torch.uint8, device="cuda")
    t[9:] = recs[:67].reshape(-1).cuda()
    for filters in syn_predicates(rd.copybook, rows).values():
        b = rd.decode_device(t[9:], 200 * 67, filters=filters)
        _check(b.to_rows(), rows[:67], rd.copybook, filters, b.unhandled_filters)


@pytest.mark.parametrize("n", [1, 63, 64, 65, SYN_N])
def test_syn200_edge_selections(syn, n):
    """In(REC-ID, [...]): all rows, no rows, only record 0, only the last record, only record 64."""
    rd, recs, rows = syn
    cb = rd.copybook
    data = recs[:n].numpy().tobytes()
    ids = [row_value(cb, r, "REC-ID") for r in rows[:n]]
    absent = next(v for v in range(10 ** 9) if v not in set(ids))
    # In holds 64 literals: every record's id where they fit, else NOT In(an id no record has)
    cases = {"all": F.In("REC-ID", ids) if n <= N.CBX_FILTER_MAX_LITERALS else F.Not(F.In("REC-ID", [absent])),
             "none": F.In("REC-ID", [absent]), "first": F.In("REC-ID", [ids[0]]), "last": F.In("REC-ID", [ids[-1]])}
    if n > 64:
        cases["rec64"] = F.In("REC-ID", [ids[64]])
    for key, f in cases.items():
        b = rd.decode(data, filters=[f])
        k = _check(b.to_rows(), rows[:n], cb, [f], b.unhandled_filters)
        assert k == {"all": n, "none": 0}.get(key, k) and (key in ("all", "none") or k >= 1)
        assert b.n_rec == k


def test_syn200_past_the_scan_block():
    """A batch just past one block of the scan over the tile counts (131,072 records), kept rows on both sides
    of the boundary.  The oracle's rows of 131k records take ~20 s to build in Python, so here the keep flags
    come from the oracle's COLUMNS (numpy) and the expected rows from the oracle's decode of the kept records."""
    n = N.FILTER_SCAN_BLOCK_RECORDS + 65
    assert n <= 200_000
    rd = FixedLenNestedReader(SYN200_COPYBOOK, SYN_PARAMS)
    cb = rd.copybook
    recs = syn200(n, seed=12, malformed_rate=0.2)
    data = recs.numpy().tobytes()
    res = O.decode_fixed(cb, data)
    cols = O.columns(res)
    rec_id, br_id = (cols[res.ast.node_of(cb.get_field_by_name(nm))] for nm in ("REC-ID", "BR-ID"))
    assert rec_id["valid"].all() and len(rec_id["lo"]) == n
    edge = [int(rec_id["lo"][i]) for i in (0, 64, N.FILTER_SCAN_BLOCK_RECORDS - 1, N.FILTER_SCAN_BLOCK_RECORDS, n - 1)]
    brs = [int(v) for v in br_id["lo"][br_id["valid"]][[7, 70000, n // 2 + 3]]]
    f = F.Or(F.In("REC-ID", edge), F.In("BR-ID", brs))
    keep = np.isin(rec_id["lo"], edge) | (br_id["valid"] & np.isin(br_id["lo"], brs))
    idx = np.nonzero(keep)[0]
    assert {0, 64, N.FILTER_SCAN_BLOCK_RECORDS - 1, N.FILTER_SCAN_BLOCK_RECORDS, n - 1} <= set(idx.tolist()) and len(idx) < 200
    exp = RO.fixed_len_rows(cb, recs[torch.from_numpy(idx)].numpy().tobytes(), SYN_PARAMS)
    assert all(py_keep(cb, r, [f]) for r in exp)
    b = rd.decode(data, filters=[f])
    assert b.unhandled_filters == [] and b.to_rows() == exp
    rd.close()


def test_unhandled_filters_are_returned_not_applied(syn):
    rd, recs, rows = syn
    data = recs[:200].numpy().tobytes()
    fx = F.GreaterThan("FX-RATE", 1)           # a COMP-2 comparison stays with the caller
    b = rd.decode(data, filters=[fx])
    assert b.unhandled_filters == [fx] and b.to_rows() == rows[:200]
    f = F.IsNull("AMT-02")
    b = rd.decode(data, filters=[fx, f])
    assert b.unhandled_filters == [fx]
    _check(b.to_rows(), rows[:200], rd.copybook, [f])
    assert rd.decode(data).unhandled_filters == []


# ---------------------------------------------------------------------------------------------
# 128-bit decimals, a two-byte code page, trimming policies, an ASCII copy of the file
# ---------------------------------------------------------------------------------------------
WIDE_COPYBOOK = """
       01  R.
           05  ID            PIC 9(4) COMP.
           05  BIG           PIC S9(25)V9(5) COMP-3.
           05  TXT           PIC X(10).
"""
# cp037 bytes whose characters take two UTF-8 bytes (cent, not sign, pound, yen, AE), letters, blanks
_CP037_TWO = [0x4A, 0x5F, 0xB1, 0xB2, 0x9E]
_CP037_ONE = [0xC1, 0xC2, 0xC3, 0x81, 0x82, 0xF1]


def _wide_records(n: int, ascii_copy: bool) -> bytes:
    rng = np.random.default_rng(2026)
    out = bytearray()
    for i in range(n):
        k = int(rng.integers(0, 8))
        digits = [0] * 31 if k == 0 else [0] + [int(d) for d in rng.integers(0, 10, 30)]   # 30 digits of precision
        if k == 1:
            digits[:20] = [0] * 20                       # small magnitudes: the high word is a sign extension
        if k == 2:
            digits[int(rng.integers(0, 31))] = 0xB       # malformed -> null
        nib = digits + [0xD if rng.random() < 0.5 else 0xC]
        big = bytes((nib[2 * j] << 4) | nib[2 * j + 1] for j in range(16))
        ln = int(rng.integers(0, 7))
        lead = int(rng.integers(0, 3))
        if ascii_copy:
            body = [int(rng.choice([0x41, 0x42, 0x61, 0x7A, 0x31, 0x09, 0xE9])) for _ in range(ln)]
            txt = bytes([0x20] * lead + body + [0x20] * (10 - lead - ln))
        else:
            body = [int(rng.choice(_CP037_TWO + _CP037_ONE)) for _ in range(ln)]
            txt = bytes([0x40] * lead + body + [0x40] * (10 - lead - ln))
        out += int(i).to_bytes(2, "big") + big + txt
    return bytes(out)


@pytest.mark.parametrize("ascii_copy", [False, True])
@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
def test_dec128_and_two_byte_strings(trim, ascii_copy):
    p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=trim, ebcdic_code_page="cp037",
                         is_ebcdic=not ascii_copy)
    rd = FixedLenNestedReader(WIDE_COPYBOOK, p)
    cb = rd.copybook
    data = _wide_records(300, ascii_copy)
    rows = RO.fixed_len_rows(cb, data, p)
    assert len(rows) == 300
    bigs = sorted(r["BIG"] for r in rows if r["BIG"] is not None)
    txts = sorted({r["TXT"] for r in rows}, key=lambda s: s.encode("utf-8"))
    assert bigs[0] < -10 ** 20 and bigs[-1] > 10 ** 20 and any(r["BIG"] is None for r in rows)
    if not ascii_copy:
        assert any(len(t.encode("utf-8")) > len(t) for t in txts)          # two-byte characters are present
    wide = next(t for t in txts if len(t.encode("utf-8")) > len(t)) if not ascii_copy else txts[len(txts) // 2]
    neg = next(b for b in bigs if -10 ** 20 < b < 0)
    cases = [[F.GreaterThan("BIG", 0)], [F.LessThan("BIG", Decimal("-1e20"))], [F.LessThanOrEqual("BIG", neg)],
             [F.GreaterThanOrEqual("BIG", bigs[len(bigs) // 2])], [F.EqualTo("BIG", bigs[3])],
             [F.In("BIG", [bigs[0], bigs[-1], Decimal(0)])], [F.Not(F.In("BIG", [Decimal(0)]))],
             [F.IsNull("BIG")], [F.GreaterThan("BIG", Decimal("-0.00001")), F.LessThan("BIG", Decimal("1e10"))],
             [F.EqualTo("TXT", wide)], [F.LessThan("TXT", wide)], [F.GreaterThanOrEqual("TXT", wide)],
             [F.StringStartsWith("TXT", wide[:2])], [F.Not(F.StringStartsWith("TXT", wide[:1]))],
             [F.In("TXT", [txts[0], txts[-1], wide])], [F.EqualTo("TXT", "")], [F.GreaterThan("TXT", " ")]]
    kept = []
    for filters in cases:
        b = rd.decode(data, filters=filters)
        kept.append(_check(b.to_rows(), rows, cb, filters, b.unhandled_filters))
    assert any(0 < k < 300 for k in kept[:9]) and any(0 < k < 300 for k in kept[9:])
    rd.close()


# ---------------------------------------------------------------------------------------------
# RDW multisegment file: select -> filter -> decode_selected, ids carried over
# ---------------------------------------------------------------------------------------------
NARROW_OPTIONS = {"is_record_sequence": "true", "segment_field": "SEGMENT_ID", "segment_id_level0": "C",
                  "segment_id_level1": "P", "input_split_records": "300", "generate_record_id": "true",
                  "redefine_segment_id_map:0": "STATIC-DETAILS => C", "redefine-segment-id-map:1": "CONTACTS => P",
                  "schema_retention_policy": "collapse_root"}


@pytest.fixture(scope="module")
def narrow():
    d, hdr = rdw_narrow(1000, seed=9)
    raw = bytearray(d.numpy().tobytes())
    # TAXPAYER-NUM (PIC 9(8) COMP at payload offset 56 of a 'C' record): the generator's letters there have
    # the top bit set (null for an unsigned 4-byte value); give every second 'C' record a value
    c_recs = [int(h) for h in hdr.tolist() if raw[int(h) + 4] == 0xC3]
    for k, h in enumerate(c_recs[::2]):
        raw[h + 4 + 56:h + 4 + 60] = (1000 + 37 * k).to_bytes(4, "big")
    raw = bytes(raw)
    p, var_len = parse_options(NARROW_OPTIONS)
    assert var_len
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    rows = RO.var_len_rows(rd.copybook, raw, p)
    assert len(rows) > 900 and {"Record_Id", "Seg_Id0", "Seg_Id1"} <= set(rows[0])
    yield rd, p, raw, rows
    rd.close()


def narrow_cases(cb, rows):
    company = next(r["STATIC_DETAILS"]["COMPANY_NAME"] for r in rows if r["STATIC_DETAILS"] is not None)
    return {"segment_c": [F.EqualTo("SEGMENT-ID", "C")],
            "company_ge": [F.GreaterThanOrEqual("COMPANY-NAME", company)],      # P records: null, dropped
            "company_null": [F.IsNull("COMPANY-NAME")],                         # exactly the P records
            "taxpayer": [F.LessThan("TAXPAYER-NUM", 1000 + 37 * 40)],
            "taxpayer_null_c": [F.IsNull("TAXPAYER-NUM"), F.EqualTo("SEGMENT-ID", "C")],
            "phone_or_company": [F.Or(F.StringStartsWith("PHONE-NUMBER", "A"), F.StringStartsWith("COMPANY-NAME", "B"))]}


def test_rdw_narrow_read_with_filters(narrow):
    rd, p, raw, rows = narrow
    cb = rd.copybook
    for key, filters in narrow_cases(cb, rows).items():
        b = rd.read(raw, filters=filters)
        got = b.to_rows()
        k = _check(got, rows, cb, filters, b.unhandled_filters)
        assert 0 < k < len(rows), key
        # surviving records keep the ids of the unfiltered read
        by_id = {r["Record_Id"]: r for r in rows}
        assert all(by_id[g["Record_Id"]]["Seg_Id0"] == g["Seg_Id0"] and by_id[g["Record_Id"]]["Seg_Id1"] == g["Seg_Id1"]
                   for g in got)
        if key == "company_null":
            assert all(g["STATIC_DETAILS"] is None for g in got) and k == sum(r["STATIC_DETAILS"] is None for r in rows)


def test_rdw_narrow_select_filter_decode_chain(narrow):
    """The device-level chain, and filtering a filtered selection again."""
    rd, p, raw, rows = narrow
    cb = rd.copybook
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    entries = rd.generate_index(t, len(raw), off, ln, 0)
    assert len(entries) > 2
    sel = rd.select(t, vb, off, ln, entries, 0)
    f1, f2 = F.EqualTo("SEGMENT-ID", "C"), F.IsNotNull("TAXPAYER-NUM")
    s1 = rd.filter(t, vb, sel, [f1])
    s2 = rd.filter(t, vb, s1, [f2])
    assert s1["unhandled"] == [] and 0 < s2["n"] < s1["n"] < sel["n"]
    _check(rd.decode_selected(t, vb, s1).to_rows(), rows, cb, [f1])
    _check(rd.decode_selected(t, vb, s2).to_rows(), rows, cb, [f1, f2])
    # Seg_IdN state comes from select(): framed records are refused on a reader with segment id levels
    for call in (lambda: rd.filter(t, vb, (off, ln), [f1]), lambda: rd.decode(raw, filters=[f1])):
        with pytest.raises(N.CbxError) as e:
            call()
        assert e.value.code == N.CBX_E_ARGUMENT and "select" in str(e.value)
    # per sparse-index entry (read_entries): the same rows
    got = [r for b in rd.read_entries(t, len(raw), entries, 2, filters=[f1, f2]) for r in b.to_rows()]
    _check(got, rows, cb, [f1, f2])


# ---------------------------------------------------------------------------------------------
# Records cut short inside and in front of the predicate fields
# ---------------------------------------------------------------------------------------------
SHORT_COPYBOOK = """
       01  R.
           05  A             PIC X(4).
           05  NUM           PIC S9(5) COMP-3.
           05  TXT           PIC X(6).
"""


def _ebcdic(s: str) -> bytes:
    return s.encode("cp037")


def test_short_variable_length_records():
    """NUM occupies bytes 4-6, TXT bytes 7-12: records of 13 (whole), 10 (cut inside TXT: compares as the
    truncated value), 7 (TXT starts at the end), 6 and 5 (cut inside NUM: null), 3 (in front of both)."""
    full = [_ebcdic("AAAA") + bytes([0x12, 0x34, 0x5C]) + _ebcdic("abcdef"),
            _ebcdic("BBBB") + bytes([0x00, 0x07, 0x7D]) + _ebcdic("abc   "),
            _ebcdic("CCCC") + bytes([0x99, 0x99, 0x9C]) + _ebcdic("  zz  ")]
    recs = []
    for k, cut in enumerate([13, 10, 7, 6, 5, 3, 13, 10, 8, 7, 4, 13, 12, 9]):
        recs.append(full[k % 3][:cut])
    raw = rdw_file(recs)
    p = ReaderParameters(is_record_sequence=True, schema_policy="collapse_root", generate_record_id=True)
    rd = VarLenNestedReader(SHORT_COPYBOOK, p)
    cb = rd.copybook
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == len(recs)
    assert sum(r["NUM"] is None for r in rows) == 4 and any(r["TXT"] == "abc" for r in rows)
    cases = [[F.EqualTo("NUM", 12345)], [F.IsNull("NUM")], [F.IsNotNull("NUM")], [F.LessThan("NUM", 0)],
             [F.EqualTo("TXT", "abc")], [F.EqualTo("TXT", "abcdef")], [F.IsNull("TXT")], [F.EqualTo("TXT", "")],
             [F.LessThan("TXT", "b")], [F.StringStartsWith("TXT", "ab")], [F.Not(F.StringStartsWith("TXT", "ab"))],
             [F.Or(F.IsNull("NUM"), F.EqualTo("TXT", "zz"))], [F.Not(F.EqualTo("NUM", 12345)), F.IsNotNull("TXT")]]
    for filters in cases:
        for b in (rd.read(raw, filters=filters), rd.decode(raw, filters=filters)):
            _check(b.to_rows(), rows, cb, filters, b.unhandled_filters)
    rd.close()


# ---------------------------------------------------------------------------------------------
# Error paths
# ---------------------------------------------------------------------------------------------
OCCURS_COPYBOOK = """
       01  R.
           05  ID            PIC 9(4) COMP.
           05  ITEMS         OCCURS 3 TIMES.
              10  ITEM-NO    PIC 9(3).
"""


def test_c_call_reports_unsupported_occurs_field():
    rd = FixedLenNestedReader(OCCURS_COPYBOOK, ReaderParameters())
    fi = rd.plan.field_of_node[id(rd.copybook.get_field_by_name("ITEM-NO"))]
    table = N.CbxFilter()
    table.n_terms, table.n_literals = 1, 1
    table.terms[0].field, table.terms[0].op, table.terms[0].lit_count = fi, N.OP_EQ, 1
    data = torch.zeros(22, dtype=torch.uint8, device="cuda")
    with pytest.raises(N.CbxError) as e:
        rd._filter_records(table, data, 22, 2, torch.cuda.current_stream(), stride=11)
    assert e.value.code == N.CBX_E_UNSUPPORTED and "OCCURS" in str(e.value)
    table.terms[0].field = 99
    with pytest.raises(N.CbxError) as e:
        rd._filter_records(table, data, 22, 2, torch.cuda.current_stream(), stride=11)
    assert e.value.code == N.CBX_E_ARGUMENT
    # the reader hands the same filter back instead
    f = F.EqualTo("ITEM-NO", 1)
    assert rd.decode(bytes(22), filters=[f]).unhandled_filters == [f]
    rd.close()


def test_hierarchical_read_with_filters_raises():
    opts = {"is_record_sequence": "true", "segment_field": "SEGMENT_ID",
            "redefine_segment_id_map:1": "STATIC-DETAILS => C", "redefine-segment-id-map:2": "CONTACTS => P",
            "segment-children:1": "STATIC-DETAILS => CONTACTS"}
    p, _ = parse_options(opts)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert rd.hierarchical
    raw = rdw_narrow(50, seed=4)[0].numpy().tobytes()
    with pytest.raises(N.CbxError) as e:
        rd.read(raw, filters=[F.EqualTo("SEGMENT-ID", "C")])
    assert e.value.code == N.CBX_E_UNSUPPORTED
    assert len(rd.read(raw).to_rows()) > 0
    rd.close()


# ---------------------------------------------------------------------------------------------
# Every decoder kind and edge: test_filter.py's filter families (one per field of a copybook) on the GPU.
# The bulk of a family is compared as a selection (the kept records' indices against the contract over
# the oracle's rows); one filter per field goes through the whole filtered read and its rows are compared.
# ---------------------------------------------------------------------------------------------
def _flags(ids, n: int, what) -> np.ndarray:
    """Keep flags of n records from a selection's record indices, which must be in file order."""
    ids = np.asarray(ids, dtype=np.int64)
    assert ids.size == 0 or (ids[0] >= 0 and ids[-1] < n and (np.diff(ids) > 0).all()), (what, ids[:10], n)
    keep = np.zeros(n, dtype=bool)
    keep[ids] = True
    return keep


def _same(a, b) -> bool:
    """Row values equal; COMP-1 / COMP-2 values (numpy scalars, NaNs among them for random bytes) as bit patterns."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.floating) and isinstance(b, np.floating):   # bit for bit, a NaN's payload included
        return a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def _rows_match(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if not _same(a, b)]
    diff = {k: (got[bad[0]].get(k), exp[bad[0]].get(k)) for k in exp[bad[0]] if not _same(got[bad[0]].get(k), exp[bad[0]].get(k))} \
        if bad else {}
    assert not bad, (what, bad[:5], diff)


def _one_filter_per_field(family, expected):
    """Of every field's compiled filters one that keeps and drops rows (any, where none does): the one that
    keeps the fewest rows for every second field, for the others the one nearest a tenth of the rows (the
    rows of a batch are rebuilt in Python: a few dozen per field keep the test quick)."""
    by = {}
    for name, f in family:
        e = expected.get(id(f))
        if e is not None:
            by.setdefault(name, []).append((int(e.sum()), len(by.get(name, ())), f, len(e)))
    picks = []
    for k, lst in enumerate(by.values()):
        sep = [x for x in lst if 0 < x[0] < x[3]] or lst
        picks.append((min(sep) if k % 2 else min(sep, key=lambda x: (abs(x[0] - x[3] // 10), x[1])))[2])
    return picks


def _run_fixed(rd, t, n_bytes, cb, rows, family, expected, first_record_id=0, **kw):
    """A family over fixed-length records in HBM: selections through cbx_filter_records, then one filtered
    decode_device per field."""
    stride = rd.get_record_size()
    n = n_bytes // stride
    assert n == len(rows)
    st = torch.cuda.current_stream()

    def keep_fn(table, f):
        sel = rd._filter_records(table, t, n_bytes, n, st, stride=stride, first_record_id=first_record_id)
        return _flags(sel["record_id"][:sel["n"]].cpu().numpy() - first_record_id, n, f)
    count = check_field_filters(cb, rd.plan, rows, family, keep_fn, expected=expected, **kw)
    for f in _one_filter_per_field(family, expected):
        b = rd.decode_device(t, n_bytes, first_record_id, filters=[f])
        assert b.unhandled_filters == []
        _rows_match(b.to_rows(), [r for r, k in zip(rows, expected[id(f)]) if k], f)
    return count


def _run_framed(rd, raw, cb, rows, family, expected, path, **kw):
    """A family over a variable-length file: `read` (select -> filter -> decode_selected) or `decode` (the framed
    records straight into the filter stage, the active segment from the plan's segment map)."""
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    n = int(off.numel())
    assert n == len(rows)
    src = rd.select(t, vb, off, ln, None, 0) if path == "read" else (off, ln)
    assert path != "read" or src["n"] == n
    host_off = off.cpu().numpy()

    def keep_fn(table, f):
        sel = rd.filter(t, vb, src, [f])
        assert sel["unhandled"] == []
        k = sel["n"]
        ids = np.searchsorted(host_off, sel["rec_off"][:k].cpu().numpy())
        assert np.array_equal(host_off[ids], sel["rec_off"][:k].cpu().numpy())
        assert np.array_equal(sel["rec_len"][:k].cpu().numpy(), ln.cpu().numpy()[ids])
        assert np.array_equal(sel["record_id"][:k].cpu().numpy(), ids), f     # Record_Id = index in the file
        return _flags(ids, n, f)
    count = check_field_filters(cb, rd.plan, rows, family, keep_fn, expected=expected, **kw)
    for f in _one_filter_per_field(family, expected):
        b = rd.read(raw, filters=[f]) if path == "read" else rd.decode(raw, filters=[f])
        assert b.unhandled_filters == []
        _rows_match(b.to_rows(), [r for r, k in zip(rows, expected[id(f)]) if k], f)
    return count


_CASES: dict = {}   # inputs, oracle rows, families and their expected flags: computed once, shared, never changed


def _case(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _device(data: bytes, odd: bool = False):
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    if not odd:
        return t.cuda()
    buf = torch.zeros(len(data) + 9, dtype=torch.uint8, device="cuda")   # a batch cut out of a larger buffer
    buf[9:] = t.cuda()
    return buf[9:]


# the option sets of test_gpu_parity.test_fuzz_copybook_vs_oracle
FUZZ_GPU_OPTIONS = [("common", "both", "IBM"), ("cp037", "left", "IEEE754"), ("cp875", "none", "IBM_LE")]
FUZZ_UNHANDLED = dict(unhandled_names=("F01", "F02"), reason="COMP-1 / COMP-2")


def _fuzz_case(code_page, trim, fmt, start, end):
    def make():
        p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim,
                             floating_point_format=fmt, start_offset=start, end_offset=end)
        cb = parse_copybook_for(FUZZ_COPYBOOK, p)
        data = fuzz_records(cb, FUZZ_N, 31, start, end)
        rows = RO.fixed_len_rows(cb, data, p)
        assert len(rows) == FUZZ_N
        return p, cb, data, rows, list(field_filters(cb, rows, random.Random(17))), {}
    return _case(("fuzz", code_page, trim, fmt, start, end), make)


@pytest.mark.parametrize("mode", ["plain", "offsets", "odd_pointer"])
@pytest.mark.parametrize("code_page,trim,fmt", FUZZ_GPU_OPTIONS)
def test_fuzz_copybook_field_filters(code_page, trim, fmt, mode):
    """Every zoned / binary / COMP-3 shape of the decode fuzz, three strings and null tests on two floats, 321
    records (two workgroups, the second with one record): plain, with record_start_offset 3 and
    record_end_offset 2 (random bytes there), and at an odd device address."""
    start, end = (3, 2) if mode == "offsets" else (0, 0)
    p, cb, data, rows, family, expected = _fuzz_case(code_page, trim, fmt, start, end)
    rd = FixedLenNestedReader(FUZZ_COPYBOOK, p)
    n = _run_fixed(rd, _device(data, odd=mode == "odd_pointer"), len(data), cb, rows, family, expected, **FUZZ_UNHANDLED)
    assert n > 1000
    rd.close()


@pytest.mark.parametrize("code_page,trim,fmt", FUZZ_GPU_OPTIONS)
def test_fuzz_copybook_single_record(code_page, trim, fmt):
    """One record at the start of the data: a field that ends before byte 16 has no 16 bytes in front of its
    end, so the SWAR forms hand it to the byte loop.  The literals are those of the 321-record family."""
    p, cb, data, rows, family, _ = _fuzz_case(code_page, trim, fmt, 0, 0)
    rd = FixedLenNestedReader(FUZZ_COPYBOOK, p)
    one = data[:cb.record_size]
    n = _run_fixed(rd, _device(one), len(one), cb, rows[:1], family, {}, separation=0, **FUZZ_UNHANDLED)
    assert n > 1000
    rd.close()


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_ascii_copybook_field_filters(charset):
    """ASCII data: every CBX_K_ASCII_NUM shape, the ASCII string through ascii_lut or the charset's table."""
    def make():
        p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
        cb = parse_copybook_for(ASCII_COPYBOOK, p)
        data = ascii_records(cb, FUZZ_N, 32)
        rows = RO.fixed_len_rows(cb, data, p)
        return p, cb, data, rows, list(field_filters(cb, rows, random.Random(18))), {}
    p, cb, data, rows, family, expected = _case(("ascii", charset), make)
    rd = FixedLenNestedReader(ASCII_COPYBOOK, p)
    n = _run_fixed(rd, _device(data), len(data), cb, rows, family, expected, unhandled_names=("N1", "N2", "N3"),
                   reason="UTF-16", null_tests_compile=False)
    assert n > 300
    rd.close()


@pytest.mark.parametrize("path", ["read", "decode"])
@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
def test_width_ladder_on_cut_records(trim, path):
    """Strings of 1-47 bytes (in registers up to 32 bytes, through the pointer beyond), COMP-3 and zoned of 1-16
    bytes on 500 RDW records cut at random lengths, under the four trimming policies."""
    def make():
        p = ladder_params(trim)
        cb = parse_copybook_for(LADDER_COPYBOOK, p)
        raw, _, _ = ladder_file()
        rows = RO.var_len_rows(cb, raw, p)
        return p, cb, raw, rows, list(field_filters(cb, rows, random.Random(19))), {}
    p, cb, raw, rows, family, expected = _case(("ladder", trim), make)
    rd = VarLenNestedReader(LADDER_COPYBOOK, p)
    n = _run_framed(rd, raw, cb, rows, family, expected, path)
    assert n > 950
    rd.close()


@pytest.mark.parametrize("trim", ["none", "both"])
def test_width_ladder_cut_at_every_length(trim):
    """One ladder record per length 1..L (framed source): every field cut after each of its bytes."""
    def make():
        p = ladder_params(trim)
        cb = parse_copybook_for(LADDER_COPYBOOK, p)
        raw, _, ln = ladder_file(seed=34, every_length=True)
        assert ln.tolist() == list(range(1, cb.record_size + 1))
        rows = RO.var_len_rows(cb, raw, p)
        return p, cb, raw, rows, list(field_filters(cb, rows, random.Random(26))), {}
    p, cb, raw, rows, family, expected = _case(("ladder_every", trim), make)
    rd = VarLenNestedReader(LADDER_COPYBOOK, p)
    assert _run_framed(rd, raw, cb, rows, family, expected, "decode") > 950
    rd.close()


@pytest.mark.parametrize("start,delta", [(0, 17 - 517), (0, -150), (5, 98)])
def test_record_length_shorter_and_longer_than_the_copybook(start, delta):
    """record_length (the pattern of test_gpu_parity.test_record_offsets_and_length) on FUZZ_COPYBOOK: 17 bytes
    (S1 and S2 whole, A1 cut after two bytes, every numeric past the record: null), 150 bytes short (the
    COMP-3 fields and the floats past the record), 98 bytes long behind a start offset of 5."""
    p0 = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037")
    size = parse_copybook_for(FUZZ_COPYBOOK, p0).record_size
    assert size == 517
    rl = size + delta
    n_rec = 130

    def make():
        p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", start_offset=start, record_length=rl)
        cb = parse_copybook_for(FUZZ_COPYBOOK, p)
        base = fuzz_records(cb, n_rec, 41)
        rng = np.random.default_rng(1)
        data = bytearray()
        for i in range(n_rec):
            r = base[i * size:(i + 1) * size] + bytes(rng.integers(0, 256, max(0, rl - size), dtype=np.uint8))
            data += bytes(rng.integers(0, 256, start, dtype=np.uint8)) + r[:rl]
        rows = RO.fixed_len_rows(cb, bytes(data), p)
        assert len(rows) == n_rec
        return p, cb, bytes(data), rows, list(field_filters(cb, rows, random.Random(23))), {}
    p, cb, data, rows, family, expected = _case(("record_length", start, delta), make)
    if delta < 0:
        assert all(r["P17"] is None and r["F02"] is None for r in rows) and any(r["S1"] for r in rows)
    if rl == 17:
        assert all(r["Z01"] is None and len(r["A1"]) <= 2 for r in rows) and any(len(r["A1"]) == 2 for r in rows)
    rd = FixedLenNestedReader(FUZZ_COPYBOOK, p)
    assert rd.get_record_size() == rl + start
    # fields past a short record are null in every row: their null tests cannot keep and drop rows
    n = _run_fixed(rd, _device(data), len(data), cb, rows, family, expected,
                   **({"separation": 0} if delta < 0 else {}), **FUZZ_UNHANDLED)
    assert n > (1000 if delta > 0 else 50)
    rd.close()


def test_segment_map_without_levels_fixed():
    """Fixed-length records of the test5 layout (test_gpu_parity.test_segment_redefines_fixed) with the
    redefine map and no Seg_Id levels: the filter stage takes each record's active segment from the plan's
    segment map and hands it to the decode.  Some records carry an id the map does not name."""
    p = ReaderParameters(schema_policy="collapse_root", segment_field="SEGMENT-ID",
                         segment_id_redefine_map=dict(NARROW_SEGMENTS))
    cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(FUZZ_N, 22)
    off, ln = O.frame_rdw(raw)
    L = cb.record_size
    data = b"".join((raw[o:o + l] + b"\x40" * L)[:L] for o, l in zip(off, ln))
    rows = RO.fixed_len_rows(cb, data, p)
    assert len(rows) == FUZZ_N
    assert all(any(r[g] is not None for r in rows) for g in ("STATIC_DETAILS", "CONTACTS"))
    assert any(r["STATIC_DETAILS"] is None and r["CONTACTS"] is None for r in rows)
    rd = FixedLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert rd.plan.options.has_segments and not rd.plan.seg_id_columns
    family = list(field_filters(cb, rows, random.Random(24)))
    assert _run_fixed(rd, _device(data), len(data), cb, rows, family, {}) > 150
    rd.close()


def test_segment_map_without_levels_framed():
    """RDW_NARROW through decode(raw, filters=...): framed records, segment_field and the redefine map but no
    segment_id_level*, so no select() stage gives the segments."""
    p = narrow_params()
    cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(FUZZ_N, 21)
    rows = RO.var_len_rows(cb, raw, p)
    assert all(any(r[g] is not None for r in rows) for g in ("STATIC_DETAILS", "CONTACTS"))
    assert any(r["STATIC_DETAILS"] is None and r["CONTACTS"] is None for r in rows)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert rd.plan.options.has_segments and not rd.plan.seg_id_columns
    family = list(field_filters(cb, rows, random.Random(25)))
    assert _run_framed(rd, raw, cb, rows, family, {}, "decode") > 150
    rd.close()


def test_first_record_id_carried_into_a_fixed_selection(syn):
    rd, recs, rows = syn
    n = 130
    data = recs[:n].numpy().tobytes()
    t = _device(data)
    for key, filters in syn_predicates(rd.copybook, rows).items():
        exp = np.nonzero(expected_keep(rd.copybook, rows[:n], filters))[0]
        table, un = F.compile_filters(rd.plan, filters)
        assert not un
        sel = rd._filter_records(table, t, len(data), n, torch.cuda.current_stream(), stride=200, first_record_id=1000)
        assert sel["n"] == len(exp), key
        assert np.array_equal(sel["record_id"][:sel["n"]].cpu().numpy(), 1000 + exp), key
        assert np.array_equal(sel["rec_off"][:sel["n"]].cpu().numpy(), 200 * exp), key
        b = rd.decode_device(t, len(data), 1000, filters=filters)
        _check(b.to_rows(), rows[:n], rd.copybook, filters, b.unhandled_filters)


# ---------------------------------------------------------------------------------------------
# Filtered reads in the three string layouts, on the table-driven and the specialised kernel
# ---------------------------------------------------------------------------------------------
def _share_filters(cb, rows, name):
    """Five filters on `name` that keep none, one, about a tenth, about half and all of the rows; the literals
    are the oracle's values."""
    vals = sorted(v for v in (row_value(cb, r, name) for r in rows) if v is not None)
    once = next(v for v in vals if vals.count(v) == 1)
    return {"none": F.LessThan(name, vals[0]), "one": F.EqualTo(name, once),
            "tenth": F.LessThan(name, vals[len(vals) // 10]), "half": F.LessThan(name, vals[len(vals) // 2]),
            "all": F.Or(F.IsNull(name), F.GreaterThanOrEqual(name, vals[0]))}


def _layout_case(which):
    def make():
        if which == "syn200":
            text, kw, name = SYN200_COPYBOOK, {}, "ACCT-NO"
            cb = parse_copybook_for(text, ReaderParameters(schema_policy="collapse_root"))
            data = syn200(SYN_N, seed=11, malformed_rate=0.2).numpy().tobytes()
        else:
            text, kw, name = FUZZ_COPYBOOK, dict(ebcdic_code_page="cp037", string_trimming_policy="left"), "B07"
            cb = parse_copybook_for(text, ReaderParameters(schema_policy="collapse_root", **kw))
            data = fuzz_records(cb, FUZZ_N, 31)
        rows = RO.fixed_len_rows(cb, data, ReaderParameters(schema_policy="collapse_root", **kw))
        filters = _share_filters(cb, rows, name)
        kept = {k: np.nonzero(expected_keep(cb, rows, [f]))[0] for k, f in filters.items()}
        n = len(rows)
        assert len(kept["none"]) == 0 and len(kept["one"]) == 1 and len(kept["all"]) == n
        assert n // 20 < len(kept["tenth"]) < n // 5 and n // 3 < len(kept["half"]) < 2 * n // 3
        return text, kw, cb, data, filters, kept
    return _case(("layout", which), make)


@pytest.mark.parametrize("jit", [1, -1])
@pytest.mark.parametrize("layout", ["large", "views", "utf8"])
@pytest.mark.parametrize("which", ["syn200", "fuzz"])
def test_filtered_read_layouts_and_kernels(which, layout, jit):
    """A filtered fixed-length read decodes the kept records through the offset / length path: in the large,
    string-view and Utf8 layouts, with the specialised kernel allowed from one record on and switched off,
    every column equals the oracle's decode of exactly the kept records' bytes."""
    text, kw, cb, data, filters, kept = _layout_case(which)
    rd = FixedLenNestedReader(text, ReaderParameters(schema_policy="collapse_root", jit_min_records=jit,
                                                     string_views=layout == "views", string_utf8=layout == "utf8", **kw))
    size = rd.get_record_size()
    t = _device(data)
    for key, f in filters.items():
        idx = kept[key]
        b = rd.decode_device(t, len(data), filters=[f])
        assert b.unhandled_filters == [] and b.n_rec == len(idx), (key, b.n_rec, len(idx))
        if len(idx) == 0:
            continue
        sub = b"".join(data[i * size:(i + 1) * size] for i in idx)
        errs = compare_batch(b, O.decode_fixed(rd.copybook, sub))
        assert not errs, (key, errs)
        if layout == "utf8":
            pitch = 64 * ((b.n_rec + 63) // 64)
            for ci, info in enumerate(rd.plan.columns):
                c = b.cols[ci]
                if "offsets32" not in c:
                    continue
                o = c["offsets32"].cpu().numpy().reshape(info.n_slots, pitch + 1)[:, :b.n_rec + 1].astype(np.int64)
                assert (o[:, 0] == 0).all() and (np.diff(o, axis=1) >= 0).all(), (key, ci)
                assert np.array_equal(o[:, -1], c["sizes"].cpu().numpy()), (key, ci)
    rd.close()
