"""Suffix / substring filters, null-safe equality and constant filters on the GPU: the kept rows of the test
pass (cbx_filter_records), of the filtered reads and of the stages that inline filter_keep (aggregate, grouped
aggregate, Top-N, the keyed filter) against test_filter_strings.py's evaluator over the ORACLE's rows -- never
the code under test.  Literals are cut from the data (data_literals), so that the reference alone shows every
matching filter to keep some rows and drop others.
"""
from __future__ import annotations

import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from cobrix_amd import aggregate as A  # noqa: E402
from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.reader import (FixedLenNestedReader, ReaderParameters, VarLenNestedReader,  # noqa: E402
                               parse_copybook_for)
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, SYN200_COPYBOOK, rdw_file, syn200  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_aggregate import ALL_FUNCS, expected_aggregates  # noqa: E402
from test_filter import narrow_file, narrow_params, row_value  # noqa: E402
from test_filter_strings import (STRING_OPS, check_string_family, family_filter, py_keep_s, raw_table,  # noqa: E402
                                 string_family, string_fields)
from test_group import check_groups, expected_groups  # noqa: E402
from topn_cases import S, expected_indices  # noqa: E402


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


def _flags(ids, n: int) -> np.ndarray:
    ids = np.asarray(ids, dtype=np.int64)
    assert ids.size == 0 or (ids[0] >= 0 and ids[-1] < n and (np.diff(ids) > 0).all()), (ids[:10], n)
    keep = np.zeros(n, dtype=bool)
    keep[ids] = True
    return keep


def _fixed_keep_fn(rd, t, n_bytes, n):
    st = torch.cuda.current_stream()
    stride = rd.get_record_size()

    def fn(table):
        sel = rd._filter_records(table, t, n_bytes, n, st, stride=stride)
        return _flags(sel["record_id"][:sel["n"]].cpu().numpy(), n)
    return fn


def _framed_keep_fn(rd, t, n_bytes, off, ln):
    st = torch.cuda.current_stream()
    n = int(off.numel())

    def fn(table):
        sel = rd._filter_records(table, t, n_bytes, n, st, rec_off=off, rec_len=ln)
        return _flags(sel["record_id"][:sel["n"]].cpu().numpy(), n)   # Record_Id = index in the file
    return fn


def _kept(cb, rows, filters):
    return [r for r in rows if py_keep_s(cb, r, filters)]


def _check_rows(batch, cb, rows, filters):
    """The filtered read's rows are the oracle's rows the evaluator keeps; returns their number."""
    assert batch.unhandled_filters == []
    got, exp = batch.to_rows(), _kept(cb, rows, filters)
    assert len(got) == len(exp), (filters, len(got), len(exp))
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if a != b]
    assert not bad, (filters, bad[:5], got[bad[0]], exp[bad[0]])
    return len(exp)


# ---------------------------------------------------------------------------------------------
# A ladder of string widths: the word boundaries of FltBytes and both sides of kFltRegBytes
# ---------------------------------------------------------------------------------------------
WIDTHS = [1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40, 64]
WIDTH_COPYBOOK = "       01  R.\n" + "".join(f"           05  X{s:02d}   PIC X({s}).\n" for s in WIDTHS)
WIDTH_N = 130   # two tiles and two lanes
# blank (weighted), letters and digits, cent / not sign / pound in cp037 (two UTF-8 bytes each), NUL
EBCDIC_ALPHABET = [0x40] * 10 + [0xC1, 0xC2, 0x81, 0x82, 0xF0, 0xF1] + [0x4A, 0x5F, 0xB1] + [0x00]
ASCII_ALPHABET = [0x20] * 10 + list(b"ABab01") + list(b"#~_") + [0x09]
ENCODINGS = {"cp037": dict(ebcdic_code_page="cp037"), "cp875": dict(ebcdic_code_page="cp875"), "ascii": dict(is_ebcdic=False)}


def width_records(alphabet, filler: int, n: int = WIDTH_N, seed: int = 51) -> bytes:
    """n records of random alphabet bytes; every sixteenth record holds `filler` (a byte outside the alphabet) in
    every position, so that no literal cut from another record matches every record."""
    rng = random.Random(seed)
    size = sum(WIDTHS)
    return b"".join(bytes([filler]) * size if i % 16 == 5 else bytes(rng.choice(alphabet) for _ in range(size))
                    for i in range(n))


_CASES: dict = {}   # inputs, oracle rows, families and their expected flags: computed once, shared, never changed


def _case(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _width_case(enc, trim):
    def make():
        p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=trim, **ENCODINGS[enc])
        cb = parse_copybook_for(WIDTH_COPYBOOK, p)
        data = width_records(ASCII_ALPHABET, ord("Z")) if enc == "ascii" else width_records(EBCDIC_ALPHABET, 0xE9)
        rows = RO.fixed_len_rows(cb, data, p)
        assert len(rows) == WIDTH_N
        return p, cb, data, rows, {}
    return _case(("width", enc, trim), make)


@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
@pytest.mark.parametrize("enc", list(ENCODINGS))
def test_width_ladder(enc, trim):
    """PIC X(n) for n at the word boundaries of the register image and on both sides of its 32-byte limit, 130
    records: every field crossed with the four ops.  X01 of record 0 lies at offset 0 of the data: nothing is
    readable in front of it."""
    p, cb, data, rows, expected = _width_case(enc, trim)
    rd = FixedLenNestedReader(WIDTH_COPYBOOK, p)
    assert string_fields(cb, rd.plan) == [f"X{s:02d}" for s in WIDTHS]
    family = string_family(cb, rd.plan, rows, random.Random(52), per_field=2)
    t = _device(data)
    n, raw = check_string_family(cb, rd.plan, rows, family, _fixed_keep_fn(rd, t, len(data), WIDTH_N), expected)
    assert n > 1200 and (raw > 0 or enc == "ascii")   # (raw: literals cut inside a two-byte character)
    # filtered reads: the rows, not only the selection
    v = next(x for x in (row_value(cb, r, "X33") for r in rows[1:]) if len(x.strip()) > 4).strip()
    for f in (F.StringContains("X33", v[1:3]), F.Not(F.StringContains("X33", v[1:3]))):
        assert 0 < _check_rows(rd.decode_device(t, len(data), filters=[f]), cb, rows, [f]) < WIDTH_N
    for f in (F.StringEndsWith("X33", v[-2:]), F.Not(F.StringEndsWith("X16", v[-1:]))):
        _check_rows(rd.decode_device(t, len(data), filters=[f]), cb, rows, [f])
    rd.close()


EDGE_COPYBOOK = """
       01  R.
           05  E07           PIC X(7).
           05  E03           PIC X(3).
           05  E13           PIC X(13).
           05  E05           PIC X(5).
"""


@pytest.mark.parametrize("odd", [False, True])
def test_load_path_edges(odd):
    """The first field of record 0 at offset 0 of the data with fewer than 8 bytes: flt_load_bytes has nothing to
    load in front of it (its `back` path); the next fields' last words end at bytes 10, 23 and 28.  Plain and at an
    odd device address."""
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", string_trimming_policy="both")

    def make():
        cb = parse_copybook_for(EDGE_COPYBOOK, p)
        rng = random.Random(53)
        data = b"".join(bytes([0xE9]) * 28 if i % 16 == 5 else bytes(rng.choice(EBCDIC_ALPHABET) for _ in range(28))
                        for i in range(WIDTH_N))
        rows = RO.fixed_len_rows(cb, data, p)
        return cb, data, rows, {}
    cb, data, rows, expected = _case("edges", make)
    rd = FixedLenNestedReader(EDGE_COPYBOOK, p)
    family = string_family(cb, rd.plan, rows, random.Random(54), per_field=4)
    t = _device(data, odd)
    check_string_family(cb, rd.plan, rows, family, _fixed_keep_fn(rd, t, len(data), WIDTH_N), expected)
    # record 0 alone: its first field has no byte in front of it and none behind the record
    one = _device(data[:28], odd)
    fam0 = [m for m in family if m[0] == "E07"]
    check_string_family(cb, rd.plan, rows[:1], fam0, _fixed_keep_fn(rd, one, 28, 1), from_data=False)
    rd.close()


# ---------------------------------------------------------------------------------------------
# Variable-length records cut inside the strings; segment redefines
# ---------------------------------------------------------------------------------------------
CUT_COPYBOOK = """
       01  R.
           05  ID            PIC X(2).
           05  S12           PIC X(12).
           05  S33           PIC X(33).
"""


def test_rdw_records_cut_inside_the_strings_at_every_length():
    """Three records per length 1..47: S12 (registers) and S33 (the pointer path) cut after each of their bytes
    compare as the cut value; a string that starts past the record's end is null and kept by no op."""
    p = ReaderParameters(is_record_sequence=True, schema_policy="collapse_root", ebcdic_code_page="cp037",
                         string_trimming_policy="both")

    def make():
        cb = parse_copybook_for(CUT_COPYBOOK, p)
        rng = random.Random(55)
        recs = [bytes(rng.choice(EBCDIC_ALPHABET) for _ in range(47))[:ln] for ln in range(1, 48) for _ in range(3)]
        raw = rdw_file(recs)
        rows = RO.var_len_rows(cb, raw, p)
        assert len(rows) == 141
        return cb, raw, rows, {}
    cb, raw, rows, expected = _case("cut", make)
    rd = VarLenNestedReader(CUT_COPYBOOK, p)
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    assert int(off.numel()) == 141
    family = string_family(cb, rd.plan, rows, random.Random(56), per_field=6, names=["S12", "S33"])
    check_string_family(cb, rd.plan, rows, family, _framed_keep_fn(rd, t, vb, off, ln), expected)
    nulls = np.array([r["S33"] is None for r in rows])
    assert nulls.sum() == 3 * 13   # records of 1..13 bytes end in front of S33 (a record of 14 holds its empty start)
    for (name, op, lit), exp in expected.items():
        assert name != "S33" or not exp[nulls].any()
    v = next(r["S33"] for r in rows[100:] if r["S33"] and len(r["S33"]) > 3)
    for f in (F.StringContains("S33", v[1:3]), F.Not(F.StringEndsWith("S12", v[-1:]))):
        for b in (rd.read(raw, filters=[f]), rd.decode(raw, filters=[f])):
            assert 0 < _check_rows(b, cb, rows, [f]) < 141
    rd.close()


def test_rdw_multisegment_inactive_segment_is_null():
    """RDW_NARROW with its redefine map, the active segment from the plan's segment map: a field of the other
    redefine is kept by neither an op nor its negation."""
    p = narrow_params()

    def make():
        cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
        raw = narrow_file(300, 21)
        rows = RO.var_len_rows(cb, raw, p)
        assert len(rows) == 300
        return cb, raw, rows, {}
    cb, raw, rows, expected = _case("narrow", make)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    family = string_family(cb, rd.plan, rows, random.Random(57), per_field=3)
    n, _ = check_string_family(cb, rd.plan, rows, family, _framed_keep_fn(rd, t, vb, off, ln), expected)
    assert n > 150
    nulls = np.array([row_value(cb, r, "COMPANY-NAME") is None for r in rows])
    assert nulls.any() and not nulls.all()
    seen = 0
    for (name, op, lit), exp in expected.items():
        if name.replace("_", "-") == "COMPANY-NAME":   # (leaf names are the transformed identifiers)
            assert not exp[nulls].any()
            seen += 1
    assert seen >= 4 * 8
    company = next(v for v in (row_value(cb, r, "COMPANY-NAME") for r in rows) if v)
    for f in (F.StringContains("COMPANY-NAME", company[1:3]), F.Not(F.StringContains("COMPANY-NAME", company[1:3]))):
        assert 0 < _check_rows(rd.read(raw, filters=[f]), cb, rows, [f]) < 300
    rd.close()


# ---------------------------------------------------------------------------------------------
# SYN200: tile edges, null-safe equality, constants
# ---------------------------------------------------------------------------------------------
SYN_PARAMS = ReaderParameters(schema_policy="collapse_root")


@pytest.fixture(scope="module")
def syn():
    """(reader, data of 1,000 records, oracle rows) -- computed once, shared, never changed."""
    rd = FixedLenNestedReader(SYN200_COPYBOOK, SYN_PARAMS)
    data = syn200(1000, seed=11, malformed_rate=0.2).numpy().tobytes()
    rows = RO.fixed_len_rows(rd.copybook, data, SYN_PARAMS)
    assert len(rows) == 1000
    _name.cb = rd.copybook
    yield rd, data, rows
    rd.close()


def _name(row):
    return row_value(_name.cb, row, "NAME")


def _name_literal(rows):
    """Two characters from the middle of the first NAME of four characters or more (among the first 63 records)."""
    return next(_name(r) for r in rows[:63] if len(_name(r)) >= 4)[1:3]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_syn200_name_contains_at_tile_edges(syn, n):
    rd, data, rows = syn
    lit = _name_literal(rows)
    one = _name(rows[0])[:1] or "A"
    t = _device(data[:200 * n])
    kept = []
    for f in (F.StringContains("NAME", lit), F.Not(F.StringContains("NAME", lit)), F.StringContains("NAME", one),
              F.StringEndsWith("NAME", one), F.StringContains("NAME", ""), F.Not(F.StringEndsWith("NAME", ""))):
        kept.append(_check_rows(rd.decode_device(t, 200 * n, filters=[f]), rd.copybook, rows[:n], [f]))
    assert kept[0] + kept[1] == n == kept[4] and kept[5] == 0
    if n >= 63:
        assert 0 < kept[0] < n and 0 < kept[2] < n


def test_null_safe_equality_and_constants_through_the_reads(syn):
    rd, data, rows = syn
    cb = rd.copybook
    amt = next(v for v in (row_value(cb, r, "AMT-01") for r in rows) if v is not None)
    nulls = sum(row_value(cb, r, "AMT-01") is None for r in rows)
    assert 0 < nulls < 1000
    x = F.StringContains("NAME", _name_literal(rows))
    t = _device(data)
    want = {"eq": ([F.EqualNullSafe("AMT-01", amt)], None), "ne": ([F.Not(F.EqualNullSafe("AMT-01", amt))], None),
            "null": ([F.EqualNullSafe("AMT-01", None)], nulls), "not_null": ([F.Not(F.EqualNullSafe("AMT-01", None))], 1000 - nulls),
            "name": ([F.Not(F.EqualNullSafe("NAME", _name(rows[0])))], None),
            "or_false": ([F.Or(F.AlwaysFalse(), x)], None), "not_true": ([F.Not(F.AlwaysTrue())], 0),
            "true": ([F.AlwaysTrue()], 1000), "and_true": ([F.And(F.AlwaysTrue(), x), F.Not(F.AlwaysFalse())], None)}
    kept = {}
    for key, (filters, k) in want.items():
        kept[key] = _check_rows(rd.decode_device(t, len(data), filters=filters), cb, rows, filters)
        assert k is None or kept[key] == k, key
    assert kept["eq"] >= 1 and kept["eq"] + kept["ne"] == 1000        # NOT (a <=> v) keeps the nulls
    assert kept["or_false"] == kept["and_true"] and 0 < kept["or_false"] < 1000
    assert _check_rows(rd.decode(data, filters=want["ne"][0]), cb, rows, want["ne"][0]) == kept["ne"]
    # the variable-length reader's read(filters=)
    p = narrow_params()
    rdn = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(300, 21)
    nrows = RO.var_len_rows(rdn.copybook, raw, p)
    company = next(v for v in (row_value(rdn.copybook, r, "COMPANY-NAME") for r in nrows) if v)
    y = F.StringEndsWith("COMPANY-NAME", company[-1:])
    for filters, k in (([F.Or(F.AlwaysFalse(), y)], None), ([F.Not(F.AlwaysTrue())], 0),
                       ([F.Not(F.EqualNullSafe("COMPANY-NAME", company))], None), ([F.EqualNullSafe("COMPANY-NAME", None)], None)):
        got = _check_rows(rdn.read(raw, filters=filters), rdn.copybook, nrows, filters)
        assert (got == k) if k is not None else 0 < got < 300, filters
    rdn.close()


# ---------------------------------------------------------------------------------------------
# The stages that inline filter_keep
# ---------------------------------------------------------------------------------------------
def test_aggregate_with_a_contains_filter(syn):
    rd, data, rows = syn
    f = [F.StringContains("NAME", _name_literal(rows))]
    aggs = [A.CountStar()] + [fn(c) for c in ("AMT-01", "BR-ID") for fn in ALL_FUNCS] + [A.Count("NAME")]
    kept = _kept(rd.copybook, rows, f)
    assert 0 < len(kept) < 1000
    got = rd.aggregate_device(_device(data), len(data), aggs, f)
    n_rows, values, _ = expected_aggregates(rd.copybook, rd.plan, kept, aggs)
    assert got.n_rows == n_rows == len(kept) and got.values == values


def test_aggregate_by_with_a_contains_filter(syn):
    rd, data, rows = syn
    f = [F.Not(F.StringContains("NAME", _name_literal(rows)[:1]))]
    aggs = [A.CountStar(), A.Sum("AMT-01"), A.Min("BR-ID"), A.Count("NAME")]
    kept = _kept(rd.copybook, rows, f)
    assert 0 < len(kept) < 1000
    got = rd.aggregate_by_device(_device(data), len(data), ["ZD-01", "NAME"], aggs, f, max_groups=2048)
    check_groups(got, expected_groups(rd.copybook, rd.plan, kept, ["ZD-01", "NAME"], aggs), aggs)
    assert got.n_rows == len(kept)


def test_top_n_with_a_contains_filter(syn):
    rd, data, rows = syn
    f = [F.StringContains("NAME", _name_literal(rows)[:1])]
    kept = _kept(rd.copybook, rows, f)
    assert 10 < len(kept) < 1000
    orders = [S("AMT-01", True), S("NAME")]
    _, chosen = expected_indices(rd.copybook, kept, orders, 10)
    b = rd.top_n_device(_device(data), len(data), orders, 10, f)
    assert b.to_rows() == [kept[i] for i in chosen] and len(chosen) == 10


def test_keyed_filter_with_a_contains_filter(syn):
    rd, data, rows = syn
    cb = rd.copybook
    x = F.StringContains("NAME", _name_literal(rows)[:1])
    ids = sorted({v for v in (row_value(cb, r, "BR-ID") for r in rows) if v is not None})
    half = ids[::2]
    exp = [r for r in _kept(cb, rows, [x]) if row_value(cb, r, "BR-ID") in set(half)]
    assert 0 < len(exp) < len(_kept(cb, rows, [x]))
    with rd.key_set(["BR-ID"], half) as ks:
        b = rd.decode_device(_device(data), len(data), filters=[F.InSet(ks), x])
        assert b.unhandled_filters == [] and b.to_rows() == exp


# ---------------------------------------------------------------------------------------------
# The raw C call
# ---------------------------------------------------------------------------------------------
def test_raw_c_call_rejections(syn):
    rd, data, rows = syn
    t = _device(data[:200 * 64])
    st = torch.cuda.current_stream()
    name, amt = (rd.plan.field_of_node[id(rd.copybook.get_field_by_name(c))] for c in ("NAME", "AMT-01"))

    def call(table):
        return rd._filter_records(table, t, 200 * 64, 64, st, stride=200)

    assert N.load().cbx_filter_max_op() == 16
    for table, word in ((raw_table(name, 17, [b"A"]), "unknown op"), (raw_table(amt, N.OP_ENDS_WITH, [b"1"]), "ENDS_WITH on a numeric field"),
                        (raw_table(amt, N.OP_NOT_CONTAINS, [b"1"]), "CONTAINS on a numeric field"),
                        (raw_table(name, N.OP_CONTAINS, [b"A", b"B"]), "literal"), (raw_table(name, N.OP_ENDS_WITH, []), "literal")):
        with pytest.raises(N.CbxError) as e:
            call(table)
        assert e.value.code == N.CBX_E_ARGUMENT and word in str(e.value), (word, str(e.value))
    for op in STRING_OPS:   # a literal cut inside a character, as only a C caller can pass it
        sel = call(raw_table(name, op, [b"\xc2"]))
        exp = [py_keep_s(rd.copybook, r, [family_filter("NAME", op, b"\xc2")]) for r in rows[:64]]
        assert sel["n"] == sum(exp)
