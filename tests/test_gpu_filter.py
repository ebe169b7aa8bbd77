"""Row filters on the GPU (cbx_filter_records -> cbx_decode_selected) against the contract: the filtered
read returns exactly the rows of the unfiltered ORACLE read that the filters keep under SQL three-valued
logic (test_filter.py py_keep over the oracle's rows -- never the code under test), in file order, every
value identical, generated ids included.
"""
from __future__ import annotations

from decimal import Decimal

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.options import parse_options  # noqa: E402
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader  # noqa: E402
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, SYN200_COPYBOOK, rdw_file, rdw_narrow, syn200  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_filter import py_keep, row_value  # noqa: E402


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
