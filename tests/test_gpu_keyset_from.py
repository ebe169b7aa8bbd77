"""Key sets built on the GPU from a second file's records (cbx_key_set_create_from_records through
`key_set_of` / `key_set_of_device`) against the contract: the distinct non-null source keys of the ORACLE's source rows
that the source filters keep, without the ones the probe columns can never hold (test_keyset_from.py model_of), and the
probe rows expected_set_keep keeps with those values -- never the code under test.  Every test calls the new entry
point: none of them passes without the feature.
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
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader  # noqa: E402
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, SYN200_COPYBOOK  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_aggregate import ALL_FUNCS, expected_aggregates  # noqa: E402
from test_filter import row_value  # noqa: E402
from test_gpu_filter import _flags  # noqa: E402
from test_gpu_filter import narrow  # noqa: E402,F401  (fixture)
from test_group import check_groups, expected_groups  # noqa: E402
from test_keyset import expected_set_keep  # noqa: E402
from test_keyset_from import (DIM_COPYBOOK, DIM_SIZE, _bcd, _zoned, counts_of, dim_records, model_of,  # noqa: E402
                              probe_records)
from topn_cases import S, expected_indices  # noqa: E402

PARAMS = ReaderParameters(schema_policy="collapse_root")
COUNTS = [1, 63, 64, 65, 321]
PAIRS = [(["D-BR"], ["BR-ID"]), (["D-ACCT"], ["ACCT-NO"]), (["D-AMT"], ["AMT-01"]), (["D-NAME"], ["NAME"]), (["D-BIG"], ["ACCT-NO"])]
COMPOSITE = (["D-BR", "D-NAME", "D-AMT", "D-BIG"], ["BR-ID", "NAME", "AMT-01", "ACCT-NO"])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _device(data: bytes):
    return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()


def _cap(n: int) -> int:
    cap = 2
    while cap < 2 * n:
        cap <<= 1
    return cap


class Side:
    """A fixed-length file: reader, bytes, the oracle's rows, the bytes on the device."""

    def __init__(self, copybook: str, data: bytes, params: ReaderParameters = PARAMS):
        self.rd = FixedLenNestedReader(copybook, params)
        self.cb, self.plan, self.data = self.rd.copybook, self.rd.plan, data
        self.size = self.rd.get_record_size()
        self.rows = RO.fixed_len_rows(self.cb, data, params)
        self.t = _device(data)

    def first(self, n: int) -> "Side":
        part = object.__new__(Side)
        part.__dict__.update(self.__dict__)
        part.data, part.rows = self.data[:self.size * n], self.rows[:n]
        return part

    def flags(self, ks, neg: int) -> np.ndarray:
        n = len(self.rows)
        sel = self.rd._filter_records(None, self.t, len(self.data), n, torch.cuda.current_stream(), stride=self.size, sets=[ks],
                                      negate=[neg])
        return _flags(sel["record_id"][:sel["n"]].cpu().numpy(), n, (ks, neg))


@pytest.fixture(scope="module")
def probe():
    """321 SYN200 records, a fifth of the numeric fields malformed -- computed once, shared, never changed."""
    s = Side(SYN200_COPYBOOK, probe_records())
    assert len(s.rows) == 321
    yield s
    s.rd.close()


@pytest.fixture(scope="module")
def dim(probe):
    """321 DIM records (keys encoded differently from SYN200's), half of them drawn from the probe's rows, a fifth of
    the numeric fields malformed."""
    s = Side(DIM_COPYBOOK, dim_records(321, 7, probe.cb, probe.rows))
    assert len(s.rows) == 321 and s.size == DIM_SIZE
    yield s
    s.rd.close()


def check_set(probe: Side, names, source: Side, snames, filters=(), model=None, **kw):
    """Build the set on the device; its counts, sizes and keep flags (IN, NOT IN for one column) equal the model's, and
    the flags equal those of a host-built set over the model's values.  Returns (model, IN flags)."""
    m = model if model is not None else model_of(source.cb, source.rows, snames, probe.plan, names, filters)
    first = None
    with source.rd.key_set_of_device(source.t, len(source.data), snames, probe.rd, names, filters=list(filters) or None, **kw) as ks:
        assert counts_of(ks.source_info) == m.counts(), (snames, counts_of(ks.source_info), m.counts())
        info = ks.info()
        assert (info.n_values, info.n_distinct, info.n_keys) == (len(m.values), len(m.values), len(names))
        assert info.capacity == _cap(len(m.values))   # what cbx_key_set_create over the same tuples chooses
        assert (ks.n_values, ks.dropped, ks.has_null) == (len(m.values), m.n_dropped, m.n_null_rows > 0)
        assert not ks.source_info.overflow and ks.source_info.source_capacity == _cap(kw.get("max_values", 65536))
        with probe.rd.key_set(names, m.values) as host:
            assert host.dropped == 0 and host.n_values == len(m.values)
            for neg in ((0, 1) if len(names) == 1 else (0,)):
                exp = expected_set_keep(probe.cb, probe.rows, [], [(names, m.values, neg)])
                got = probe.flags(ks, neg)
                assert np.array_equal(got, exp), (snames, neg, np.flatnonzero(got != exp)[:8])
                assert np.array_equal(probe.flags(host, neg), exp)
                first = exp if first is None else first
    assert ks.closed
    return m, first


# ---------------------------------------------------------------------------------------------
# Record counts x key pairs; the counts do not depend on max_workgroups
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_source_record_counts(probe, dim, n):
    part = dim.first(n)
    for snames, names in PAIRS:
        m, exp = check_set(probe, names, part, snames)
        if n == 321:
            assert 0 < exp.sum() < 321, snames
            assert m.n_null_rows > 0 or snames == ["D-NAME"]
            check_set(probe, names, part, snames, model=m, max_workgroups=1)
    if n == 321:   # the out-of-range values are dropped and counted
        assert model_of(dim.cb, dim.rows, ["D-NAME"], probe.plan, ["NAME"]).n_dropped > 0
        assert model_of(dim.cb, dim.rows, ["D-BIG"], probe.plan, ["ACCT-NO"]).n_dropped > 0


def test_composite_of_four_keys_and_a_source_filter(probe, dim):
    snames, names = COMPOSITE
    for filters in ([], [F.IsNotNull("D-RATE")], [F.GreaterThan("D-BR", 0), F.LessThan("D-AMT", Decimal("5000000.00"))]):
        m, exp = check_set(probe, names, dim, snames, filters)
        assert 0 < exp.sum() < 321 and m.n_null_rows > 0 and 0 < m.n_rows <= 321


def test_heavy_duplication(probe, dim):
    """321 rows with 3 distinct keys."""
    three = [r for r in range(321) if all(row_value(dim.cb, dim.rows[r], c) is not None for c in ("D-BR", "D-NAME"))
             and row_value(probe.cb, probe.rows[0], "BR-ID") is not None][:3]
    recs = [dim.data[DIM_SIZE * r:DIM_SIZE * (r + 1)] for r in three]
    recs[0] = _bcd(row_value(probe.cb, probe.rows[0], "BR-ID"), 3) + recs[0][3:]
    dup = Side(DIM_COPYBOOK, b"".join(recs[i % 3] for i in range(321)))
    for snames, names in ((["D-BR"], ["BR-ID"]), (["D-BR", "D-NAME"], ["BR-ID", "NAME"])):
        m, exp = check_set(probe, names, dup, snames)
        assert m.counts() == (321, 0, 3, 0)
    m, exp = check_set(probe, ["BR-ID"], dup, ["D-BR"], max_workgroups=1)
    assert 0 < exp.sum() < 321
    dup.rd.close()


def test_all_source_keys_null_no_records_and_a_filter_that_keeps_none(probe, dim):
    null = Side(DIM_COPYBOOK, b"".join(b"\xAB\xAB\xAB" + dim.data[DIM_SIZE * i + 3:DIM_SIZE * (i + 1)] for i in range(100)))
    m, exp = check_set(probe, ["BR-ID"], null, ["D-BR"])
    assert m.counts() == (100, 100, 0, 0) and not exp.any()
    null.rd.close()
    m, exp = check_set(probe, ["BR-ID"], dim.first(0), ["D-BR"])
    assert m.counts() == (0, 0, 0, 0) and not exp.any()
    m, exp = check_set(probe, ["BR-ID"], dim, ["D-BR"], [F.GreaterThan("D-BR", 10 ** 6)])
    assert m.counts() == (0, 0, 0, 0) and not exp.any()


def test_max_values_exact_and_one_less(probe, dim):
    m = model_of(dim.cb, dim.rows, ["D-ACCT"], probe.plan, ["ACCT-NO"])
    assert m.n_source_keys > 100
    check_set(probe, ["ACCT-NO"], dim, ["D-ACCT"], model=m, max_values=m.n_source_keys)
    with pytest.raises(A.GroupOverflow):
        dim.rd.key_set_of_device(dim.t, len(dim.data), ["D-ACCT"], probe.rd, ["ACCT-NO"], max_values=m.n_source_keys - 1)
    # nothing was left behind: the next call on the same plans succeeds
    check_set(probe, ["ACCT-NO"], dim, ["D-ACCT"], model=m, max_values=m.n_source_keys)
    # the C level: the status, the flag, no handle
    L = N.load()
    pt, st = N.CbxGroupBy(), N.CbxGroupBy()
    pt.n_keys = st.n_keys = 1
    pt.fields[0] = probe.plan.field_of_node[id(probe.cb.get_field_by_name("ACCT-NO"))]
    st.fields[0] = dim.plan.field_of_node[id(dim.cb.get_field_by_name("D-ACCT"))]
    h, info = ctypes.c_void_p(), N.CbxKeysetSourceInfo()
    rc = L.cbx_key_set_create_from_records(probe.rd.native.handle, ctypes.byref(pt), dim.rd.native.handle, ctypes.byref(st),
                                           dim.t.data_ptr(), len(dim.data), None, None, None, 321, DIM_SIZE, 0, None,
                                           m.n_source_keys - 1, 0, None, ctypes.byref(h), ctypes.byref(info))
    assert rc == N.CBX_E_CAPACITY and info.overflow == 1 and not h.value and "max_values" in L.cbx_last_error().decode()
    for bad, word in ((0, "at least 1"), (1 << 40, "workspace")):
        rc = L.cbx_key_set_create_from_records(probe.rd.native.handle, ctypes.byref(pt), dim.rd.native.handle, ctypes.byref(st),
                                               dim.t.data_ptr(), len(dim.data), None, None, None, 321, DIM_SIZE, 0, None, bad, 0,
                                               None, ctypes.byref(h), None)
        assert rc == N.CBX_E_ARGUMENT and word in L.cbx_last_error().decode() and not h.value
    rc = L.cbx_key_set_create_from_records(probe.rd.native.handle, ctypes.byref(pt), dim.rd.native.handle, ctypes.byref(st),
                                           dim.t.data_ptr(), len(dim.data), None, None, None, 400, DIM_SIZE, 0, None, 65536, 0,
                                           None, ctypes.byref(h), None)
    assert rc == N.CBX_E_ARGUMENT and "exceed n_bytes" in L.cbx_last_error().decode()


def test_seventy_thousand_distinct_source_keys(probe):
    """More than one workgroup in every pass (1,094 source tiles, a distinct table of 2^18 slots, 70,000 values)."""
    have = sorted({v for v in (row_value(probe.cb, r, "ACCT-NO") for r in probe.rows) if v is not None and abs(v) < 10 ** 18})
    assert len(have) >= 10
    keys = have[::2] + list(range(-35000, 35000))
    keys = keys[:70000]
    filler = _bcd(0, 3), _bcd(0, 5) + b"\x40" * 24 + _bcd(0, 11) + _bcd(0, 5)
    big = Side(DIM_COPYBOOK, b"".join(filler[0] + _zoned(v, 18) + filler[1] for v in keys))
    m, exp = check_set(probe, ["ACCT-NO"], big, ["D-ACCT"], max_values=70000)
    assert m.counts() == (70000, 0, 70000, 0) and 0 < exp.sum() < 321
    with pytest.raises(A.GroupOverflow):
        big.rd.key_set_of_device(big.t, len(big.data), ["D-ACCT"], probe.rd, ["ACCT-NO"])   # 65,536 by default
    big.rd.close()


# ---------------------------------------------------------------------------------------------
# Text: code pages and trimming policies differ between the two sides
# ---------------------------------------------------------------------------------------------
TEXT_COPYBOOK = "       01  R.\n           05  T    PIC X(10).\n           05  N    PIC S9(3) COMP-3.\n"
TEXT_WORDS = ["A¢", "£B¬", "¬¬", "plain", "", "¢", "x£y", "Zz", "££££££££££", "¢ ¢"]


def _text_records(words, encoding: str, pad: bytes, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out = bytearray()
    for i, w in enumerate(words):
        raw = w.encode(encoding)
        lead = int(rng.integers(0, 10 - len(raw) + 1)) if i % 3 == 2 else 0
        out += pad * lead + raw + pad * (10 - lead - len(raw)) + _bcd(i % 7, 2)
    return bytes(out)


def test_cp037_source_against_an_ascii_probe(probe):
    """An EBCDIC master joins an ASCII fact file on the decoded text, two-byte UTF-8 characters included."""
    rng = np.random.default_rng(5)
    swords = [TEXT_WORDS[int(k)] for k in rng.integers(0, 7, 130)]
    pwords = [TEXT_WORDS[int(k)] for k in rng.integers(3, 10, 321)]
    source = Side(TEXT_COPYBOOK, _text_records(swords, "cp037", b"\x40", 1),
                  ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", string_trimming_policy="both"))
    fact = Side(TEXT_COPYBOOK, _text_records(pwords, "cp1252", b" ", 2),
                ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset="windows-1252",
                                 string_trimming_policy="both"))
    assert any(len(r["T"].encode()) > len(r["T"]) for r in source.rows) and any(len(r["T"].encode()) > len(r["T"]) for r in fact.rows)
    m, exp = check_set(fact, ["T"], source, ["T"])
    assert 0 < exp.sum() < 321 and m.n_source_keys >= 5
    source.rd.close()
    fact.rd.close()


@pytest.mark.parametrize("strim,ptrim", [("none", "both"), ("both", "none"), ("left", "right")])
def test_trimming_policies_differ(strim, ptrim):
    """Each side trims as its own plan says; the model (the oracle's rows of each side) says which rows match."""
    rng = np.random.default_rng(6)
    swords = [TEXT_WORDS[int(k)] for k in rng.integers(0, 10, 130)]
    pwords = [TEXT_WORDS[int(k)] for k in rng.integers(0, 10, 321)]
    source = Side(TEXT_COPYBOOK, _text_records(swords, "cp037", b"\x40", 3),
                  ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", string_trimming_policy=strim))
    fact = Side(TEXT_COPYBOOK, _text_records(pwords, "cp037", b"\x40", 4),
                ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", string_trimming_policy=ptrim))
    m, exp = check_set(fact, ["T"], source, ["T"])
    both = check_set(fact, ["T", "N"], source, ["T", "N"])[1]
    assert 0 < exp.sum() < 321 and both.sum() <= exp.sum()
    source.rd.close()
    fact.rd.close()


# ---------------------------------------------------------------------------------------------
# A variable-length source with segment redefines, through the reader's selection
# ---------------------------------------------------------------------------------------------
NUM_COPYBOOK = "       01  R.\n           05  K    PIC S9(9) COMP.\n           05  C    PIC X(5).\n"


def test_variable_length_source_with_segment_redefines(narrow):  # noqa: F811
    """RDW_NARROW (Seg_Id levels, record ids, a sparse index) as the source: TAXPAYER-NUM lies inside the STATIC-DETAILS
    redefine, so it is null in every CONTACTS record."""
    rd, p, raw, rows = narrow
    ks_vals = [1000 + 37 * k for k in range(0, 400, 3)] + [5, 6, 7]
    fact = Side(NUM_COPYBOOK, b"".join(int(v).to_bytes(4, "big", signed=True) + ("C" if i % 2 else "P").ljust(5).encode("cp037")
                                       for i, v in enumerate(ks_vals)))
    for snames, names, filters in ((["TAXPAYER-NUM"], ["K"], []), (["TAXPAYER-NUM", "SEGMENT-ID"], ["K", "C"], []),
                                   (["TAXPAYER-NUM"], ["K"], [F.LessThan("TAXPAYER-NUM", 1000 + 37 * 40)])):
        m = model_of(rd.copybook, rows, snames, fact.plan, names, filters)
        with rd.key_set_of(raw, snames, fact.rd, names, filters=filters or None) as ks:
            assert counts_of(ks.source_info) == m.counts() and m.n_source_keys > 10
            # (a comparison with a null is not true: the filtered case has no null key left)
            assert (m.n_null_rows == 0 and not ks.has_null) if filters else (m.n_null_rows > 300 and ks.has_null)
            assert ks.info().n_distinct == len(m.values)
            exp = expected_set_keep(fact.cb, fact.rows, [], [(names, m.values, 0)])
            assert np.array_equal(fact.flags(ks, 0), exp) and 0 < exp.sum() < len(exp)
    fact.rd.close()


def test_hierarchical_source_and_unpushed_filters_refuse(probe, dim):
    opts = {"is_record_sequence": "true", "segment_field": "SEGMENT_ID",
            "redefine_segment_id_map:1": "STATIC-DETAILS => C", "redefine-segment-id-map:2": "CONTACTS => P",
            "segment-children:1": "STATIC-DETAILS => CONTACTS"}
    p, _ = parse_options(opts)
    hier = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert hier.hierarchical
    from cobrix_amd.synth import rdw_narrow
    raw = rdw_narrow(50, seed=4)[0].numpy().tobytes()
    with pytest.raises(N.CbxError) as e:
        hier.key_set_of(raw, ["SEGMENT-ID"], probe.rd, ["NAME"])
    assert e.value.code == N.CBX_E_UNSUPPORTED
    hier.close()
    # a filter that is not pushed down: a set over unfiltered rows would be wrong
    with pytest.raises(A.Unhandled, match="table limits"):
        dim.rd.key_set_of_device(dim.t, len(dim.data), ["D-BR"], probe.rd, ["BR-ID"], filters=[F.In("D-BR", list(range(65)))])
    # columns that do not pair
    for snames, names, word in ((["D-RATE"], ["AMT-01"], "scales 2 and 3 differ"), (["D-NAME"], ["BR-ID"], "string column against"),
                                (["D-BR", "D-ACCT"], ["BR-ID"], "1 probe key columns against 2"), (["D-BR"], ["FX-RATE"], "probe: ")):
        with pytest.raises(F.Unhandled, match=word):
            dim.rd.key_set_of_device(dim.t, len(dim.data), snames, probe.rd, names)
    # and the C level says the same
    L = N.load()
    pt, st = N.CbxGroupBy(), N.CbxGroupBy()
    pt.n_keys = st.n_keys = 1
    h = ctypes.c_void_p()
    for pcol, scol, rc_want, word in (("AMT-01", "D-RATE", N.CBX_E_UNSUPPORTED, "key 0: scales 2 and 3 differ"),
                                      ("BR-ID", "D-NAME", N.CBX_E_ARGUMENT, "key 0: a string column against a numeric one"),
                                      ("FX-RATE", "D-BR", N.CBX_E_UNSUPPORTED, "probe: cbx_group_by: key 0: COMP-1 / COMP-2 key")):
        pt.fields[0] = probe.plan.field_of_node[id(probe.cb.get_field_by_name(pcol))]
        st.fields[0] = dim.plan.field_of_node[id(dim.cb.get_field_by_name(scol))]
        rc = L.cbx_key_set_create_from_records(probe.rd.native.handle, ctypes.byref(pt), dim.rd.native.handle, ctypes.byref(st),
                                               dim.t.data_ptr(), len(dim.data), None, None, None, 321, DIM_SIZE, 0, None, 65536, 0,
                                               None, ctypes.byref(h), None)
        assert rc == rc_want and word in L.cbx_last_error().decode() and not h.value


# ---------------------------------------------------------------------------------------------
# Chained semi joins; the probe side's stages with a device-built set
# ---------------------------------------------------------------------------------------------
def test_source_filter_with_an_in_set_of_its_own(probe, dim):
    br = sorted({v for v in (row_value(dim.cb, r, "D-BR") for r in dim.rows) if v is not None})
    first = br[::2]
    kept_rows = [r for r, k in zip(dim.rows, expected_set_keep(dim.cb, dim.rows, [F.IsNotNull("D-RATE")], [(["D-BR"], first, 0)])) if k]
    assert 0 < len(kept_rows) < 321
    m = model_of(dim.cb, kept_rows, ["D-NAME"], probe.plan, ["NAME"])
    with dim.rd.key_set(["D-BR"], first) as inner:
        check_set(probe, ["NAME"], dim, ["D-NAME"], [F.IsNotNull("D-RATE"), F.InSet(inner)], model=m)
        assert 0 < expected_set_keep(probe.cb, probe.rows, [], [(["NAME"], m.values, 0)]).sum() < 321


AGGS = [A.CountStar()] + [fn(c) for c in ("AMT-01", "ACCT-NO", "ZD-01") for fn in ALL_FUNCS] + [A.Count("NAME")]


def test_probe_stages_take_a_device_built_set(probe, dim):
    rd, cb, rows, t, data = probe.rd, probe.cb, probe.rows, probe.t, probe.data
    snames, names = ["D-BR", "D-NAME"], ["BR-ID", "NAME"]
    m = model_of(dim.cb, dim.rows, snames, probe.plan, names)
    with pytest.raises(F.Unhandled, match="probe: "):   # names default to source_names: SYN200 has no such columns
        dim.rd.key_set_of(dim.data, snames, rd)
    with dim.rd.key_set_of(dim.data, snames, dim.rd) as own:
        assert own.names == snames and own.plan is dim.plan and own.n_values == model_of(dim.cb, dim.rows, snames, dim.plan, snames).n_source_keys
    with dim.rd.key_set_of(dim.data, snames, rd, names) as ks:
        for plain in ([], [F.LessThan("ZD-01", 0)]):
            filters = plain + [F.InSet(ks)]
            keep = expected_set_keep(cb, rows, plain, [(names, m.values, 0)])
            kept = [r for r, k in zip(rows, keep) if k]
            kept_at = np.flatnonzero(keep)
            assert 0 < len(kept) < len(rows)
            b = rd.decode_device(t, len(data), filters=filters)
            assert b.unhandled_filters == [] and b.to_rows() == kept
            got = rd.aggregate_device(t, len(data), AGGS, filters)
            n_rows, values, _ = expected_aggregates(cb, rd.plan, kept, AGGS)
            assert got.n_rows == n_rows == len(kept) and got.values == values
            grouped = rd.aggregate_by_device(t, len(data), ["BR-ID"], AGGS, filters)
            check_groups(grouped, expected_groups(cb, rd.plan, kept, ["BR-ID"], AGGS), AGGS)
            orders = [S("AMT-01", True), S("NAME")]
            for limit in (1, 10, len(kept) + 1):
                _, chosen = expected_indices(cb, kept, orders, limit)
                b = rd.top_n_device(t, len(data), orders, limit, filters, first_record_id=100)
                assert b.to_rows() == [kept[i] for i in chosen], (plain, limit)
                sel = rd._top_n_records(orders, limit, filters, t, len(data), 321, torch.cuda.current_stream(), stride=200,
                                        first_record_id=100)
                assert sel["record_id"][:sel["n"]].cpu().tolist() == [100 + int(kept_at[i]) for i in chosen]
    # a closed set is refused
    assert ks.closed
    with pytest.raises(ValueError, match="closed"):
        rd.decode_device(t, len(data), filters=[F.InSet(ks)])
    with pytest.raises(ValueError):
        ks.info()
    # a set of another reader's plan is handed back
    other = FixedLenNestedReader(SYN200_COPYBOOK, PARAMS)
    with dim.rd.key_set_of(dim.data, ["D-BR"], other, ["BR-ID"]) as foreign:
        flt = F.InSet(foreign)
        b = rd.decode_device(t, len(data), filters=[flt])
        assert b.unhandled_filters == [flt] and b.n_rec == 321
    other.close()


def test_not_in_over_a_source_with_null_keys_stays_unhandled(probe, dim):
    """SQL's NOT IN over a subquery with a NULL: unknown for every row, so the filter is handed back."""
    with dim.rd.key_set_of(dim.data, ["D-BR"], probe.rd, ["BR-ID"]) as ks:
        assert ks.has_null and ks.source_info.n_null_rows > 0
        flt = F.NotInSet(ks)
        b = probe.rd.decode_device(probe.t, len(probe.data), filters=[flt])
        assert b.unhandled_filters == [flt] and b.n_rec == 321
        with pytest.raises(A.Unhandled, match="null"):
            probe.rd.aggregate_device(probe.t, len(probe.data), [A.CountStar()], [flt])
    # without null keys in the source the negated set is pushed down
    m = model_of(dim.cb, dim.rows, ["D-BR"], probe.plan, ["BR-ID"], [F.IsNotNull("D-BR")])
    with dim.rd.key_set_of(dim.data, ["D-BR"], probe.rd, ["BR-ID"], filters=[F.IsNotNull("D-BR")]) as ks:
        assert not ks.has_null
        b = probe.rd.decode_device(probe.t, len(probe.data), filters=[F.NotInSet(ks)])
        exp = expected_set_keep(probe.cb, probe.rows, [], [(["BR-ID"], m.values, 1)])
        assert b.unhandled_filters == [] and b.to_rows() == [r for r, k in zip(probe.rows, exp) if k] and 0 < exp.sum() < 321


def test_pass_times_with_profiling(probe, dim):
    L = N.load()
    with dim.rd.key_set_of(dim.data, ["D-ACCT"], probe.rd, ["ACCT-NO"]) as ks:
        assert ks.source_info.distinct_ms == 0.0 and ks.source_info.convert_ms == 0.0 and ks.info().build_ms == 0.0
        assert ks.source_info.workspace_bytes >= 8 * ks.source_info.source_capacity
    N.check(L.cbx_plan_set_profiling(dim.rd.native.handle, 1))
    try:
        with dim.rd.key_set_of(dim.data, ["D-ACCT"], probe.rd, ["ACCT-NO"]) as ks:
            assert ks.source_info.distinct_ms > 0 and ks.source_info.convert_ms > 0 and ks.info().build_ms > 0
    finally:
        N.check(L.cbx_plan_set_profiling(dim.rd.native.handle, 0))
