"""Lookup joins on the GPU (cbx_key_map_create_from_records, cbx_join_records, cbx_select_ordinals through the
readers' `key_map_of` / `join` and through the C ABI) against the contract: `map_model` and `expected_join` of
test_keymap.py over the ORACLE's rows of both files -- never the code under test.  Every test calls a new entry point:
none of them passes without the feature.
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
from cobrix_amd import keyset as K  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader, parse_copybook_for  # noqa: E402
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, SYN200_COPYBOOK  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_filter import FUZZ_N, NARROW_SEGMENTS, narrow_file, narrow_params, row_value  # noqa: E402
from test_gpu_filter import narrow  # noqa: E402,F401  (fixture)
from test_gpu_keyset_from import (NUM_COPYBOOK, TEXT_COPYBOOK, TEXT_WORDS, Side, _device, _text_records, dim,  # noqa: E402,F401
                                  probe)
from test_keymap import duplicates_of, expected_join, map_model  # noqa: E402
from test_keyset import distinct_keys, expected_set_keep  # noqa: E402
from test_keyset_from import DIM_COPYBOOK, DIM_SIZE, _bcd, _zoned, counts_of  # noqa: E402

COUNTS = [1, 63, 64, 65, 321]
SEL_KEYS = ("rec_off", "rec_len", "record_id", "segment")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cur():
    return torch.cuda.current_stream()


def _sel_arrays(sel):
    return [sel[k][:sel["n"]].cpu().numpy() for k in SEL_KEYS]


def check_result(res, fact: Side, names, mp, how, keep_k=None, first_record_id=0):
    """A JoinResult against expected_join; returns (kept indices, match)."""
    keep_k = np.ones(len(fact.rows), bool) if keep_k is None else keep_k
    idx, match, mrows = expected_join(fact.cb, fact.rows, keep_k, names, mp, how)
    assert res.selection["n"] == len(idx) == res.batch.n_rec
    assert np.array_equal(res.selection["record_id"][:len(idx)].cpu().numpy(), first_record_id + idx), (names, how)
    assert np.array_equal(res.match.cpu().numpy(), match) and np.array_equal(res.match_rows.cpu().numpy(), mrows), (names, how)
    assert np.array_equal(res.matched.cpu().numpy(), match >= 0)
    assert res.batch.to_rows() == [fact.rows[i] for i in idx]
    return idx, match


def check_map_and_join(fact: Side, names, source: Side, snames, filters=(), **kw):
    """Build the map on the device; counts, duplicate numbers and both joins over the fact file equal the model's, and
    INNER's selection is bit-identical to the keyed filter's with the map's set.  Returns (map model, INNER indices)."""
    m, mp = map_model(source.cb, source.rows, snames, fact.plan, names, filters)
    n = len(fact.rows)
    inner = None
    with source.rd.key_map_of_device(source.t, len(source.data), snames, fact.rd, names, filters=list(filters) or None, **kw) as km:
        assert counts_of(km.source_info) == m.counts(), (snames, counts_of(km.source_info), m.counts())
        assert (km.n_values, km.dropped, km.has_null) == (len(m.values), m.n_dropped, m.n_null_rows > 0)
        assert (km.n_duplicate_keys, km.max_rows_per_key) == duplicates_of(mp), snames
        assert km.key_set.info().n_distinct == len(m.values) and not km.source_info.overflow
        for how in ("inner", "left"):
            res = fact.rd.join_device(fact.t, len(fact.data), km, how, duplicates="first")
            idx, match = check_result(res, fact, names, mp, how)
            if how == "inner":
                inner = idx
                ref = fact.rd._filter_records(None, fact.t, len(fact.data), n, _cur(), stride=fact.size, sets=[km.key_set], negate=[0])
                assert ref["n"] == res.selection["n"]
                for a, b in zip(_sel_arrays(ref), _sel_arrays(res.selection)):
                    assert a.tobytes() == b.tobytes()
            else:
                assert len(idx) == n
    assert km.closed and km.key_set.closed
    return mp, inner


# ---------------------------------------------------------------------------------------------
# Record counts on both sides, empty inputs, nulls, no match
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_source_and_probe_record_counts(probe, dim, n):  # noqa: F811
    for snames, names in ((["D-BR"], ["BR-ID"]), (["D-NAME"], ["NAME"])):
        mp, inner = check_map_and_join(probe, names, dim.first(n), snames)
        check_map_and_join(probe.first(n), names, dim, snames)
        if n == 321:
            assert 0 < len(inner) < 321


def test_empty_source_empty_probe_null_keys_and_no_match(probe, dim):  # noqa: F811
    for source in (dim.first(0),
                   Side(DIM_COPYBOOK, b"".join(b"\xAB\xAB\xAB" + dim.data[DIM_SIZE * i + 3:DIM_SIZE * (i + 1)] for i in range(100)))):
        mp, inner = check_map_and_join(probe, ["BR-ID"], source, ["D-BR"])
        assert mp == {} and len(inner) == 0
        if source.rd is not dim.rd:
            source.rd.close()
    mp, inner = check_map_and_join(probe, ["BR-ID"], dim, ["D-BR"], [F.GreaterThan("D-BR", 10 ** 6)])
    assert mp == {} and len(inner) == 0
    mp, inner = check_map_and_join(probe.first(0), ["BR-ID"], dim, ["D-BR"])
    assert len(mp) > 0 and len(inner) == 0
    # a dimension whose keys no fact row has
    far = Side(DIM_COPYBOOK, b"".join(_bcd(-90000 - i, 3) + dim.data[3:DIM_SIZE] for i in range(65)))
    assert not {k[0] for k in distinct_keys(probe.cb, probe.rows, ["BR-ID"])} & set(range(-90064, -89999))
    mp, inner = check_map_and_join(probe, ["BR-ID"], far, ["D-BR"])
    assert len(mp) == 65 and len(inner) == 0
    far.rd.close()


# ---------------------------------------------------------------------------------------------
# Determinism: first_row is a minimum, n_rows a count
# ---------------------------------------------------------------------------------------------
def test_first_row_and_n_rows_do_not_depend_on_the_grid(dim):  # noqa: F811
    """321 rows over 7 keys, joined with the dimension itself (its own columns), so every member is looked at."""
    seen = {}
    for i in range(321):
        v = row_value(dim.cb, dim.rows[i], "D-BR")
        if v is not None:
            seen.setdefault(v, i)
    recs = [dim.data[DIM_SIZE * i:DIM_SIZE * (i + 1)] for i in list(seen.values())[:7]]
    dup = Side(DIM_COPYBOOK, b"".join(recs[(5 * i + i // 7) % 7] for i in range(321)))
    m, mp = map_model(dup.cb, dup.rows, ["D-BR"], dup.plan, ["D-BR"])
    assert len(mp) == 7 and sum(c for _, c in mp.values()) == 321
    for kw in (dict(max_workgroups=1), dict()):
        with dup.rd.key_map_of_device(dup.t, len(dup.data), ["D-BR"], dup.rd, **kw) as km:
            assert (km.n_duplicate_keys, km.max_rows_per_key) == duplicates_of(mp) == (len(mp), max(c for _, c in mp.values()))
            with pytest.raises(K.DuplicateKeys) as e:
                dup.rd.join_device(dup.t, len(dup.data), km)
            assert (e.value.n_duplicate_keys, e.value.max_rows_per_key) == duplicates_of(mp)
            res = dup.rd.join_device(dup.t, len(dup.data), km, "left", duplicates="first")
            idx, match = check_result(res, dup, ["D-BR"], mp, "left")
            assert sorted(set(match.tolist())) == sorted(f for f, _ in mp.values())   # the lowest ordinal of each key
            assert (match <= idx).all()
    dup.rd.close()


# ---------------------------------------------------------------------------------------------
# INNER / LEFT, filters and other sets, the C ABI
# ---------------------------------------------------------------------------------------------
def test_join_with_a_filter_and_a_negated_set_of_another_column(probe, dim):  # noqa: F811
    m, mp = map_model(dim.cb, dim.rows, ["D-BR"], probe.plan, ["BR-ID"])
    zd = distinct_keys(probe.cb, probe.rows, ["ZD-01"])[::2]
    plain = [F.IsNotNull("AMT-01")]
    keep_k = expected_set_keep(probe.cb, probe.rows, plain, [(["ZD-01"], zd, 1)])
    with dim.rd.key_map_of(dim.data, ["D-BR"], probe.rd, ["BR-ID"]) as km, probe.rd.key_set(["ZD-01"], zd) as other:
        for how in ("inner", "left"):
            res = probe.rd.join_device(probe.t, len(probe.data), km, how, filters=plain + [F.NotInSet(other)], duplicates="first",
                                       first_record_id=100)
            idx, match = check_result(res, probe, ["BR-ID"], mp, how, keep_k, first_record_id=100)
            assert 0 < len(idx) < 321
            if how == "left":
                assert (match == -1).any() and (match >= 0).any()   # null keys and non-members stay, with -1
        # the map's set is a set like any other
        b = probe.rd.decode_device(probe.t, len(probe.data), filters=[F.InSet(km.key_set)])
        exp = expected_set_keep(probe.cb, probe.rows, [], [(["BR-ID"], m.values, 0)])
        assert b.unhandled_filters == [] and b.to_rows() == [r for r, k in zip(probe.rows, exp) if k]
        with pytest.raises(A.Unhandled, match="table limits"):
            probe.rd.join_device(probe.t, len(probe.data), km, filters=[F.In("BR-ID", list(range(65)))], duplicates="first")
    with pytest.raises(ValueError, match="closed"):
        probe.rd.join_device(probe.t, len(probe.data), km)


def test_c_abi_no_sets_null_filter_and_every_refusal(probe, dim):  # noqa: F811
    L = N.load()
    m, mp = map_model(dim.cb, dim.rows, ["D-ACCT"], probe.plan, ["ACCT-NO"])
    other = FixedLenNestedReader(SYN200_COPYBOOK, ReaderParameters(schema_policy="collapse_root"))
    with dim.rd.key_map_of(dim.data, ["D-ACCT"], probe.rd, ["ACCT-NO"]) as km:
        info = N.CbxKeymapInfo()
        N.check(L.cbx_key_map_info(km.handle, ctypes.byref(info)))
        assert counts_of(info) == m.counts() and (info.n_duplicate_keys, info.max_rows_per_key) == duplicates_of(mp)
        assert info.fill_ms == 0.0
        n = 321
        out, cs = probe.rd._empty_selection(n, probe.t.device)
        match = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        ns = ctypes.c_int64(-1)

        def call(plan=probe.rd.native.handle, maph=km.handle, jt=N.JOIN_INNER, dm=match.data_ptr(), n_sets=0, sets=None, n_rec=n):
            return L.cbx_join_records(plan, probe.t.data_ptr(), len(probe.data), None, None, None, n_rec, 200, 0, 0, None, sets, None,
                                      n_sets, maph, jt, ctypes.byref(cs), ctypes.byref(ns), dm, None, None)

        assert call() == 0   # n_sets == 0, a NULL filter, no d_match_rows
        torch.cuda.synchronize()
        idx, want, _ = expected_join(probe.cb, probe.rows, np.ones(n, bool), ["ACCT-NO"], mp, "inner")
        assert ns.value == len(idx) > 0 and np.array_equal(match[:ns.value].cpu().numpy(), want)
        assert np.array_equal(out["record_id"][:ns.value].cpu().numpy(), idx)
        assert (match[ns.value:] == -7).all()   # nothing is written past the kept rows
        five, one = (ctypes.c_void_p * 5)(), (ctypes.c_void_p * 1)()
        for kw, word in ((dict(maph=None), "map: null"), (dict(plan=other.native.handle), "built for another probe plan"),
                         (dict(jt=2), "join_type 2 is neither"), (dict(dm=None), "d_match must not be NULL"),
                         (dict(n_sets=5, sets=ctypes.addressof(five)), "0 to 4 key sets"),
                         (dict(n_sets=1, sets=ctypes.addressof(one)), "set 0: null"),
                         (dict(n_rec=400), "exceed n_bytes")):
            assert call(**kw) == N.CBX_E_ARGUMENT and word in L.cbx_last_error().decode(), kw
        assert L.cbx_key_map_set(km.handle) == km.key_set.handle.value and L.cbx_key_map_set(None) is None
    L.cbx_key_map_destroy(None)   # NULL is allowed
    other.close()


# ---------------------------------------------------------------------------------------------
# Composite keys, dropped values, many keys, text
# ---------------------------------------------------------------------------------------------
def test_composite_of_four_keys_and_dropped_values(probe, dim):  # noqa: F811
    snames, names = ["D-BR", "D-NAME", "D-AMT", "D-BIG"], ["BR-ID", "NAME", "AMT-01", "ACCT-NO"]
    for filters in ([], [F.GreaterThan("D-BR", 0), F.LessThan("D-AMT", Decimal("5000000.00"))]):
        mp, inner = check_map_and_join(probe, names, dim, snames, filters)
        assert 0 < len(inner) < 321
    # source keys the probe column cannot hold (names past 18 characters, values past 63 bits) match nothing
    for snames, names in ((["D-NAME"], ["NAME"]), (["D-BIG"], ["ACCT-NO"])):
        m, _ = map_model(dim.cb, dim.rows, snames, probe.plan, names)
        assert m.n_dropped > 0
        check_map_and_join(probe, names, dim, snames)


def test_seventy_thousand_distinct_keys(probe):  # noqa: F811
    """Past 65,536: several grid rounds of the fill pass under max_workgroups, 1,094 source tiles."""
    have = sorted({v for v in (row_value(probe.cb, r, "ACCT-NO") for r in probe.rows) if v is not None and abs(v) < 10 ** 18})
    keys = (have[::2] + list(range(-35000, 35000)))[:70000]
    filler = _bcd(0, 3), _bcd(0, 5) + b"\x40" * 24 + _bcd(0, 11) + _bcd(0, 5)
    big = Side(DIM_COPYBOOK, b"".join(filler[0] + _zoned(v, 18) + filler[1] for v in keys))
    mp, inner = check_map_and_join(probe, ["ACCT-NO"], big, ["D-ACCT"], max_values=70000, max_workgroups=8)
    assert len(mp) == 70000 and duplicates_of(mp) == (0, 1) and 0 < len(inner) < 321
    with pytest.raises(A.GroupOverflow):
        big.rd.key_map_of_device(big.t, len(big.data), ["D-ACCT"], probe.rd, ["ACCT-NO"])   # 65,536 by default
    big.rd.close()


@pytest.mark.parametrize("strim,ptrim,pascii", [("both", "both", True), ("none", "both", False), ("left", "right", False)])
def test_code_pages_and_trimming_policies_differ(strim, ptrim, pascii):
    rng = np.random.default_rng(5)
    # (where both sides trim alike every shared word matches: the two files then share only some of the words)
    swords = [TEXT_WORDS[int(k)] for k in rng.integers(0, 7 if pascii else 10, 130)]
    pwords = [TEXT_WORDS[int(k)] for k in rng.integers(3 if pascii else 0, 10, 321)]
    source = Side(TEXT_COPYBOOK, _text_records(swords, "cp037", b"\x40", 1),
                  ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", string_trimming_policy=strim))
    if pascii:
        fact = Side(TEXT_COPYBOOK, _text_records(pwords, "cp1252", b" ", 2),
                    ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset="windows-1252",
                                     string_trimming_policy=ptrim))
    else:
        fact = Side(TEXT_COPYBOOK, _text_records(pwords, "cp037", b"\x40", 4),
                    ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", string_trimming_policy=ptrim))
    mp, inner = check_map_and_join(fact, ["T"], source, ["T"])
    assert 0 < len(inner) < 321 and duplicates_of(mp)[0] > 0
    check_map_and_join(fact, ["T", "N"], source, ["T", "N"])
    source.rd.close()
    fact.rd.close()


# ---------------------------------------------------------------------------------------------
# dimension() and rows(); sources that are selections
# ---------------------------------------------------------------------------------------------
def _joined_rows(fact_rows, idx, match, dim_rows, prefix=""):
    out = []
    for i, m in zip(idx.tolist(), match.tolist()):
        row = dict(fact_rows[i])
        for k, v in dim_rows[0].items():
            row[prefix + k] = dim_rows[m][k] if m >= 0 else None
        out.append(row)
    return out


def test_dimension_and_rows_against_both_oracles(probe, dim):  # noqa: F811
    m, mp = map_model(dim.cb, dim.rows, ["D-BR"], probe.plan, ["BR-ID"])
    with dim.rd.key_map_of_device(dim.t, len(dim.data), ["D-BR"], probe.rd, ["BR-ID"]) as km:
        for how in ("inner", "left"):
            res = probe.rd.join(probe.data, km, how, duplicates="first")
            idx, match = check_result(res, probe, ["BR-ID"], mp, how)
            assert res.dimension().to_rows() == [dim.rows[j] for j in match if j >= 0]
            assert res.rows() == _joined_rows(probe.rows, idx, match, dim.rows)
            assert res.rows(prefix="d.") == _joined_rows(probe.rows, idx, match, dim.rows, "d.")
        assert (match == -1).any()
    # colliding names need a prefix
    with dim.rd.key_map_of_device(dim.t, len(dim.data), ["D-BR"], dim.rd) as own:
        res = dim.rd.join_device(dim.t, len(dim.data), own, duplicates="first")
        with pytest.raises(ValueError, match="collides"):
            res.rows()
        k0 = next(iter(dim.rows[0]))   # the key column: the first dimension row with the same key has the same value
        first = res.rows(prefix="R-")[0]
        assert first["R-" + k0] == first[k0] is not None
    with pytest.raises(ValueError, match="closed"):
        res.dimension()


def test_variable_length_source_through_the_readers_selection(narrow):  # noqa: F811
    """RDW_NARROW (Seg_Id levels, record ids, a sparse index) as the dimension: the ordinals index select()'s rows, and
    dimension() carries record ids, segments and Seg_Id state over."""
    rd, p, raw, rows = narrow
    ks_vals = [1000 + 37 * k for k in range(0, 400, 3)] + [5, 6, 7]
    fact = Side(NUM_COPYBOOK, b"".join(int(v).to_bytes(4, "big", signed=True) + ("C" if i % 2 else "P").ljust(5).encode("cp037")
                                       for i, v in enumerate(ks_vals)))
    for snames, names, filters in ((["TAXPAYER-NUM"], ["K"], []), (["TAXPAYER-NUM", "SEGMENT-ID"], ["K", "C"], []),
                                   (["TAXPAYER-NUM"], ["K"], [F.LessThan("TAXPAYER-NUM", 1000 + 37 * 40)])):
        m, mp = map_model(rd.copybook, rows, snames, fact.plan, names, filters)
        with rd.key_map_of(raw, snames, fact.rd, names, filters=filters or None) as km:
            assert counts_of(km.source_info) == m.counts() and (km.n_duplicate_keys, km.max_rows_per_key) == duplicates_of(mp)
            res = fact.rd.join_device(fact.t, len(fact.data), km, "left", duplicates="first")
            idx, match = check_result(res, fact, names, mp, "left")
            assert 0 < (match >= 0).sum() < len(match)
            assert res.dimension().to_rows() == [rows[j] for j in match if j >= 0]
    fact.rd.close()


def test_source_filter_with_an_in_set_of_its_own(probe, dim):  # noqa: F811
    """The keyed filter runs first: the ordinals index its selection, and dimension() still returns the right rows."""
    br = sorted({v for v in (row_value(dim.cb, r, "D-BR") for r in dim.rows) if v is not None})[::2]
    plain = [F.IsNotNull("D-RATE")]
    keep = expected_set_keep(dim.cb, dim.rows, plain, [(["D-BR"], br, 0)])
    kept_rows = [r for r, k in zip(dim.rows, keep) if k]
    assert 0 < len(kept_rows) < 321
    m, mp = map_model(dim.cb, kept_rows, ["D-NAME"], probe.plan, ["NAME"])   # ordinals among the kept rows
    with dim.rd.key_set(["D-BR"], br) as inner_set:
        with dim.rd.key_map_of_device(dim.t, len(dim.data), ["D-NAME"], probe.rd, ["NAME"], filters=plain + [F.InSet(inner_set)]) as km:
            assert counts_of(km.source_info) == m.counts() and km.source["sel"] is not None and km.source["n_rec"] == len(kept_rows)
            res = probe.rd.join_device(probe.t, len(probe.data), km, duplicates="first")
            idx, match = check_result(res, probe, ["NAME"], mp, "inner")
            assert len(idx) > 0 and res.dimension().to_rows() == [kept_rows[j] for j in match]


def _fixed_segment_side():
    p = ReaderParameters(schema_policy="collapse_root", segment_field="SEGMENT-ID", segment_id_redefine_map=dict(NARROW_SEGMENTS))
    cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(FUZZ_N, 22)
    off, ln = O.frame_rdw(raw)
    size = cb.record_size
    return Side(RDW_NARROW_COPYBOOK, b"".join((raw[o:o + l] + b"\x40" * size)[:size] for o, l in zip(off, ln)), p)


def test_fixed_length_source_with_a_segment_map():
    """The dimension's active segments come from the plan's segment map inside cbx_select_ordinals."""
    source = _fixed_segment_side()
    assert source.rd.plan.options.has_segments and not source.rd.plan.seg_id_columns
    fact = Side(NUM_COPYBOOK, b"".join(b"\x00\x00\x00\x01" + c.ljust(5).encode("cp037") for c in "CPXCPCCP" * 9))
    m, mp = map_model(source.cb, source.rows, ["SEGMENT-ID"], fact.plan, ["C"])
    with source.rd.key_map_of_device(source.t, len(source.data), ["SEGMENT-ID"], fact.rd, ["C"]) as km:
        assert len(mp) >= 2 and km.n_duplicate_keys >= 2
        res = fact.rd.join_device(fact.t, len(fact.data), km, "left", duplicates="first")
        idx, match = check_result(res, fact, ["C"], mp, "left")
        got = res.dimension().to_rows()
        assert got == [source.rows[j] for j in match if j >= 0]
        assert any(r["STATIC_DETAILS"] is not None for r in got) and any(r["CONTACTS"] is not None for r in got)
    source.rd.close()
    fact.rd.close()


# ---------------------------------------------------------------------------------------------
# cbx_select_ordinals alone
# ---------------------------------------------------------------------------------------------
def _ordinals(n):
    return [n - 1, n - 1, n // 2, 1, 0, n + 5, 3, 2]   # repeated, descending, one out of range


def test_select_ordinals_on_all_three_record_sources(dim, narrow):  # noqa: F811
    # fixed-length records with a segment map
    source = _fixed_segment_side()
    n = len(source.rows)
    ords = _ordinals(n)
    sel = source.rd._select_ordinals(torch.tensor(ords, device="cuda"), source.t, len(source.data), _cur(), n_rec=n, stride=source.size,
                                     first_record_id=50)
    ref = source.rd._filter_records(N.CbxFilter(), source.t, len(source.data), n, _cur(), stride=source.size, first_record_id=50)
    want = [np.array([a[o] if o < n else z for o in ords], dtype=a.dtype) for a, z in zip(_sel_arrays(ref), (0, 0, -1, -1))]
    for a, b in zip(_sel_arrays(sel), want):
        assert np.array_equal(a, b)
    assert len(set(want[3].tolist())) >= 2   # more than one segment came from the map
    rows = source.rd._decode_rows(source.t, len(source.data), sel, _cur()).to_rows()
    assert [r for r, o in zip(rows, ords) if o < n] == [source.rows[o] for o in ords if o < n]
    source.rd.close()
    # framed records and a selection of a variable-length reader with Seg_Id levels
    rd, p, raw, vrows = narrow
    t, vb, whole = rd._whole_file_selection(raw, 0)
    n = whole["n"]
    ords = _ordinals(n)
    sel = rd._select_ordinals(torch.tensor(ords, device="cuda"), t, vb, _cur(), n_rec=n, sel=whole)
    nl = 1 + rd.plan.options.segments.n_levels
    state = whole["seg_state"][:n * nl].cpu().numpy().reshape(n, nl)
    got_state = sel["seg_state"][:len(ords) * nl].cpu().numpy().reshape(len(ords), nl)
    for j, o in enumerate(ords):
        if o < n:
            assert [int(sel[k][j]) for k in SEL_KEYS] == [int(whole[k][o]) for k in SEL_KEYS]
            assert np.array_equal(got_state[j], state[o])
        else:
            assert [int(sel[k][j]) for k in SEL_KEYS] == [0, 0, -1, -1]
    got = rd.decode_selected(t, vb, sel).to_rows()
    assert [r for r, o in zip(got, ords) if o < n] == [vrows[o] for o in ords if o < n]
    # framed records of a reader without levels
    p2 = narrow_params()
    rd2 = VarLenNestedReader(RDW_NARROW_COPYBOOK, p2)
    raw2 = narrow_file(FUZZ_N, 21)
    rows2 = RO.var_len_rows(rd2.copybook, raw2, p2)
    t2 = rd2._device_file(raw2)
    off2, ln2, vb2 = rd2.frame_file(t2, len(raw2))
    n = int(off2.numel())
    ords = _ordinals(n)
    sel = rd2._select_ordinals(torch.tensor(ords, device="cuda"), t2, vb2, _cur(), n_rec=n, rec_off=off2, rec_len=ln2, first_record_id=7)
    o_h, l_h = off2.cpu().numpy(), ln2.cpu().numpy()
    for j, o in enumerate(ords):
        want = [int(o_h[o]), int(l_h[o]), 7 + o] if o < n else [0, 0, -1]
        assert [int(sel[k][j]) for k in SEL_KEYS[:3]] == want
    got = rd2.decode_selected(t2, vb2, sel).to_rows()
    assert len(rows2) == n and [r for r, o in zip(got, ords) if o < n] == [rows2[o] for o in ords if o < n]
    rd2.close()
    # no ordinals: nothing is launched
    assert dim.rd._select_ordinals(torch.zeros(0, dtype=torch.int64, device="cuda"), dim.t, len(dim.data), _cur(), n_rec=321,
                                   stride=DIM_SIZE)["n"] == 0
    L = N.load()
    out, cs = dim.rd._empty_selection(4, dim.t.device)
    rc = L.cbx_select_ordinals(dim.rd.native.handle, dim.t.data_ptr(), len(dim.data), None, None, None, 321, DIM_SIZE, 0, 0, None, 4,
                               ctypes.byref(cs), None)
    assert rc == N.CBX_E_ARGUMENT and "ordinals and selection arrays required" in L.cbx_last_error().decode()


# ---------------------------------------------------------------------------------------------
# Overflow, pass times
# ---------------------------------------------------------------------------------------------
def test_overflow_leaves_nothing_behind(probe, dim):  # noqa: F811
    m, mp = map_model(dim.cb, dim.rows, ["D-ACCT"], probe.plan, ["ACCT-NO"])
    with pytest.raises(A.GroupOverflow):
        dim.rd.key_map_of_device(dim.t, len(dim.data), ["D-ACCT"], probe.rd, ["ACCT-NO"], max_values=m.n_source_keys - 1)
    L = N.load()
    pt, st = N.CbxGroupBy(), N.CbxGroupBy()
    pt.n_keys = st.n_keys = 1
    pt.fields[0] = probe.plan.field_of_node[id(probe.cb.get_field_by_name("ACCT-NO"))]
    st.fields[0] = dim.plan.field_of_node[id(dim.cb.get_field_by_name("D-ACCT"))]
    h, info = ctypes.c_void_p(), N.CbxKeymapInfo()
    rc = L.cbx_key_map_create_from_records(probe.rd.native.handle, ctypes.byref(pt), dim.rd.native.handle, ctypes.byref(st),
                                           dim.t.data_ptr(), len(dim.data), None, None, None, 321, DIM_SIZE, 0, None,
                                           m.n_source_keys - 1, 0, None, ctypes.byref(h), ctypes.byref(info))
    assert rc == N.CBX_E_CAPACITY and info.overflow == 1 and not h.value and "max_values" in L.cbx_last_error().decode()
    check_map_and_join(probe, ["ACCT-NO"], dim, ["D-ACCT"], max_values=m.n_source_keys)   # the exact bound works


def test_pass_times_with_profiling(probe, dim):  # noqa: F811
    L = N.load()
    with dim.rd.key_map_of(dim.data, ["D-ACCT"], probe.rd, ["ACCT-NO"]) as km:
        assert km.source_info.fill_ms == 0.0
        probe.rd.join_device(probe.t, len(probe.data), km, duplicates="first")
        assert probe.rd.join_pass_times() == (0.0, 0.0, 0.0)
    for rd in (dim.rd, probe.rd):
        N.check(L.cbx_plan_set_profiling(rd.native.handle, 1))
    try:
        with dim.rd.key_map_of(dim.data, ["D-ACCT"], probe.rd, ["ACCT-NO"]) as km:
            assert km.source_info.fill_ms > 0 and km.source_info.distinct_ms > 0
            probe.rd.join_device(probe.t, len(probe.data), km, duplicates="first")
            assert all(x > 0 for x in probe.rd.join_pass_times())
    finally:
        for rd in (dim.rd, probe.rd):
            N.check(L.cbx_plan_set_profiling(rd.native.handle, 0))
