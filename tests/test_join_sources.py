"""The join stages over every kind of fact source (variable-length records behind a selection, framed records, records
cut short, fixed-length records with a segment map), the parts that need no GPU: the fixture files of
test_gpu_join_sources.py, a third expected-value model written as a plain nested loop, its agreement pair for pair with
the two models the join suites already use (`map_model` / `expected_join` of test_keymap.py, `rows_model` /
`expected_expand` of test_fanout.py), and the conditions that keep the GPU tests from passing vacuously.

Everything here comes from the ORACLE's rows and framing of the fixture files; none of it runs the code under test.
"""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np
import pytest

from cobrix_amd import filter as F
from cobrix_amd.options import parse_options
from cobrix_amd.reader import ReaderParameters, parse_copybook_for
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, rdw_file, rdw_narrow
from oracle import oracle as O
from oracle import reader_oracle as RO
from test_fanout import expected_expand, rows_model
from test_filter import FUZZ_N, NARROW_SEGMENTS, narrow_file, narrow_params, py_keep, reader_plan, row_value
# (the issue asks for num_data, interleaved and the copybooks of the GPU suites to be reused: those modules need torch
# to import, as cobrix_amd.synth does, and touch no GPU until a test of theirs runs)
from test_gpu_fanout import interleaved, num_data
from test_gpu_filter import NARROW_OPTIONS, SHORT_COPYBOOK
from test_gpu_keyset_from import NUM_COPYBOOK, PARAMS
from test_keymap import expected_join, map_model


# ---------------------------------------------------------------------------------------------
# The model: a nested loop over the rows of both files
# ---------------------------------------------------------------------------------------------
def expected_join_rows(fact_rows, fact_keep, fact_names, dim_rows, dim_keep, dim_names, how, duplicates, *, fact_cb, dim_cb):
    """[(fact row index, dimension row index or -1)] of SQL's inner / left join of the kept fact rows with the kept
    dimension rows on fact_names == dim_names: in fact order, then ascending dimension ordinal; a key with a null column
    equals nothing; duplicates="first" keeps only the first dimension row of every fact row.  (`row_value` needs the
    copybooks: they are keyword arguments.)"""
    assert how in ("inner", "left") and duplicates in ("first", "all")
    fkeys = [tuple(row_value(fact_cb, r, c) for c in fact_names) for r in fact_rows]
    dkeys = [tuple(row_value(dim_cb, r, c) for c in dim_names) for r in dim_rows]
    pairs = []
    for i, fk in enumerate(fkeys):
        if not fact_keep[i]:
            continue
        hits = 0
        for j, dk in enumerate(dkeys):
            if not dim_keep[j] or None in fk or None in dk or fk != dk:
                continue
            hits += 1
            if hits == 1 or duplicates == "all":
                pairs.append((i, j))
        if not hits and how == "left":
            pairs.append((i, -1))
    return pairs


def joined_model_rows(fact_rows, dim_rows, pairs, prefix=""):
    """The row dicts `JoinResult.rows` returns for `pairs`."""
    out = []
    for i, j in pairs:
        row = dict(fact_rows[i])
        for k in dim_rows[0]:
            row[prefix + k] = dim_rows[j][k] if j >= 0 else None
        out.append(row)
    return out


# ---------------------------------------------------------------------------------------------
# The fixture files (each at most about 1000 records)
# ---------------------------------------------------------------------------------------------
class Source:
    """One file: copybook text, reader parameters, copybook, plan, bytes, the oracle's rows; for RDW files the oracle's
    framing (off, ln)."""

    def __init__(self, text, p, data, var):
        self.text, self.p, self.data, self.var = text, p, data, var
        self.cb, self.plan = reader_plan(text, p)
        if var:
            self.rows = RO.var_len_rows(self.cb, data, p)
            self.off, self.ln = O.frame_rdw(data)
            assert len(self.off) == len(self.rows)   # (no fixture drops records in select())
        else:
            self.rows = RO.fixed_len_rows(self.cb, data, p)


class Case:
    """fact, dim, the key choices [(fact names, dimension names)]; waived: {fact key names: the non-vacuity conditions
    the files cannot meet for that key}, each with its reason where the case is defined."""

    def __init__(self, fact: Source, dim: Source, keys, waived=None):
        self.fact, self.dim, self.keys = fact, dim, keys
        self.waived = {tuple(k[0]): set() for k in keys}
        self.waived.update(waived or {})


# a few taxpayer numbers of the narrow files (1000 + 37 k) with fan-outs 1, 2, 65 and 321; 5 and 6 are in no fact file
# (all but 1111 are in every narrow fact file; the composite key with SEGMENT-ID keeps about half of a list, hence 200)
NUM_FANOUTS = {1000: 1, 1037: 2, 1074: 65, 1185: 321, 1259: 200, 1333: 1, 1370: 1, 1407: 1, 1111: 3, 5: 3, 6: 1}
NARROW_KEYS = [(["TAXPAYER-NUM"], ["K"]), (["TAXPAYER-NUM", "SEGMENT-ID"], ["K", "C"])]
SHORT_KEYS = [(["NUM"], ["NUM"]), (["TXT"], ["TXT"])]
SHORT_GIVEN = [13, 10, 7, 6, 5, 3, 13, 10, 8, 7, 4, 13, 12, 9]   # the cuts of test_gpu_filter's file, in its order
SHORT_REPEATS = 66                                               # then as many records cut at 10 inside TXT, and one at 9
SHORT_CUTS = SHORT_GIVEN + [10] * SHORT_REPEATS + [9]


@functools.lru_cache(maxsize=None)
def num_dim() -> Source:
    return Source(NUM_COPYBOOK, PARAMS, num_data(interleaved(NUM_FANOUTS, seed=3)), False)


def narrow_raw() -> bytes:
    """The bytes of test_gpu_filter's `narrow` fixture: every second 'C' record has a TAXPAYER-NUM, 1000 + 37 k."""
    d, hdr = rdw_narrow(1000, seed=9)
    raw = bytearray(d.numpy().tobytes())
    c_recs = [int(h) for h in hdr.tolist() if raw[int(h) + 4] == 0xC3]
    for k, h in enumerate(c_recs[::2]):
        raw[h + 4 + 56:h + 4 + 60] = (1000 + 37 * k).to_bytes(4, "big")
    return bytes(raw)


def plain_params() -> ReaderParameters:
    """RDW_NARROW without a segment field: no redefine is ever null."""
    return ReaderParameters(is_record_sequence=True, schema_policy="collapse_root")


def fixed_segment_params() -> ReaderParameters:
    return ReaderParameters(schema_policy="collapse_root", segment_field="SEGMENT-ID", segment_id_redefine_map=dict(NARROW_SEGMENTS))


def fixed_segment_data() -> bytes:
    """The bytes of test_gpu_keymap's `_fixed_segment_side()`: narrow_file(FUZZ_N, 22), every record padded to the size."""
    raw = narrow_file(FUZZ_N, 22)
    size = parse_copybook_for(RDW_NARROW_COPYBOOK, fixed_segment_params()).record_size
    off, ln = O.frame_rdw(raw)
    return b"".join((raw[o:o + l] + b"\x40" * size)[:size] for o, l in zip(off, ln))


def _ebcdic(s: str) -> bytes:
    return s.encode("cp037")


def short_params() -> ReaderParameters:
    return ReaderParameters(is_record_sequence=True, schema_policy="collapse_root", generate_record_id=True)


def short_raw() -> bytes:
    """The 14 records of test_gpu_filter.test_short_variable_length_records (NUM occupies bytes 4-6, TXT bytes 7-12), then
    66 records with one NUM and one TXT cut inside TXT (as the dimension: a list of more than 64 truncated keys) and
    one record whose NUM and TXT no other cut record has (a list of exactly one row)."""
    full = [_ebcdic("AAAA") + bytes([0x12, 0x34, 0x5C]) + _ebcdic("abcdef"),
            _ebcdic("BBBB") + bytes([0x00, 0x07, 0x7D]) + _ebcdic("abc   "),
            _ebcdic("CCCC") + bytes([0x99, 0x99, 0x9C]) + _ebcdic("  zz  ")]
    once = _ebcdic("HHHH") + bytes([0x00, 0x42, 0x4C]) + _ebcdic("r     ")
    recs = [full[k % 3][:cut] for k, cut in enumerate(SHORT_GIVEN)] + [full[1][:10]] * SHORT_REPEATS + [once[:9]]
    assert [len(r) for r in recs] == SHORT_CUTS
    return rdw_file(recs)


def whole_data() -> bytes:
    """Whole SHORT_COPYBOOK records: a TXT equal to a value a cut leaves ("abc", 66 times), duplicated ones, the empty
    string, a NUM no cut record has, and one malformed NUM (a null key)."""
    recs = {_ebcdic("AAAA") + bytes([0x12, 0x34, 0x5C]) + _ebcdic("abcdef"): 1,
            _ebcdic("BBBB") + bytes([0x00, 0x07, 0x7D]) + _ebcdic("abc   "): 66,
            _ebcdic("DDDD") + bytes([0x00, 0x00, 0x5C]) + _ebcdic("  zz  "): 2,
            _ebcdic("EEEE") + bytes([0x00, 0x42, 0x4C]) + _ebcdic("      "): 2,
            _ebcdic("FFFF") + bytes([0xFF, 0xFF, 0xFF]) + _ebcdic("ab    "): 1,
            _ebcdic("GGGG") + bytes([0x00, 0x00, 0x9C]) + _ebcdic("q     "): 1}
    return b"".join(interleaved(recs, seed=5))


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    if name == "narrow":        # (a) (b) (c) (g) (h) (i): Seg_Id levels, record ids, a sparse index; through select()
        p, var = parse_options(NARROW_OPTIONS)
        assert var
        return Case(Source(RDW_NARROW_COPYBOOK, p, narrow_raw(), True), num_dim(), NARROW_KEYS)
    if name == "framed_map":    # (d) framed records, the active segment from the plan's segment map
        return Case(Source(RDW_NARROW_COPYBOOK, narrow_params(), narrow_file(FUZZ_N, 21), True), num_dim(), NARROW_KEYS)
    if name == "framed_plain":  # (d) framed records, no segment map
        return Case(Source(RDW_NARROW_COPYBOOK, plain_params(), narrow_file(FUZZ_N, 21), True), num_dim(), NARROW_KEYS)
    if name == "fixed_segment":  # (e) fixed-length records with a segment map
        return Case(Source(RDW_NARROW_COPYBOOK, fixed_segment_params(), fixed_segment_data(), False), num_dim(), NARROW_KEYS)
    if name == "short":         # (f) records cut short as the fact
        return Case(Source(SHORT_COPYBOOK, short_params(), short_raw(), True), Source(SHORT_COPYBOOK, PARAMS, whole_data(), False),
                    SHORT_KEYS)
    if name == "short_swapped":
        # (f) records cut short as the dimension.  The one condition this case cannot meet: the whole fixed-length
        # records of the fact side cannot hold a null string (the null TXT keys are the dimension's, which is what this
        # case is for; that the dimension has them is asserted instead).
        return Case(Source(SHORT_COPYBOOK, PARAMS, whole_data(), False), Source(SHORT_COPYBOOK, short_params(), short_raw(), True),
                    SHORT_KEYS, waived={("TXT",): {"fact_null"}})
    raise KeyError(name)


CASES = ["narrow", "framed_map", "framed_plain", "fixed_segment", "short", "short_swapped"]
SEGMENT_C = [F.EqualTo("SEGMENT-ID", "C")]   # the fact filter of (b)


def fact_filters_of(name: str):
    return [[], SEGMENT_C] if name == "narrow" else [[]]


def keep_of(src: Source, filters) -> np.ndarray:
    return np.array([py_keep(src.cb, r, filters) for r in src.rows], dtype=bool)


def model_pairs(c: Case, fnames, dnames, how, duplicates, fact_keep=None):
    keep = np.ones(len(c.fact.rows), bool) if fact_keep is None else fact_keep
    return expected_join_rows(c.fact.rows, keep, fnames, c.dim.rows, np.ones(len(c.dim.rows), bool), dnames, how, duplicates,
                              fact_cb=c.fact.cb, dim_cb=c.dim.cb)


# ---------------------------------------------------------------------------------------------
# The model itself
# ---------------------------------------------------------------------------------------------
def test_the_nested_loop_on_rows_written_by_hand():
    fact = Source(NUM_COPYBOOK, PARAMS, num_data([3, 2, 9, 2]), False)
    dim = Source(NUM_COPYBOOK, PARAMS, num_data([2, 2, 3, 7, 2]), False)
    all_f, all_d = [True] * 4, [True] * 5
    run = lambda how, dup, fk=all_f, dk=all_d: expected_join_rows(fact.rows, fk, ["K"], dim.rows, dk, ["K"], how, dup,   # noqa: E731
                                                                  fact_cb=fact.cb, dim_cb=dim.cb)
    assert run("inner", "all") == [(0, 2), (1, 0), (1, 1), (1, 4), (3, 0), (3, 1), (3, 4)]
    assert run("left", "all") == [(0, 2), (1, 0), (1, 1), (1, 4), (2, -1), (3, 0), (3, 1), (3, 4)]
    assert run("inner", "first") == [(0, 2), (1, 0), (3, 0)]
    assert run("left", "first") == [(0, 2), (1, 0), (2, -1), (3, 0)]
    assert run("left", "all", [True, False, True, True], [False, True, True, True, True]) == [(0, 2), (2, -1), (3, 1), (3, 4)]
    # (K, C): C is "P" on even and "C" on odd records of num_data
    both = expected_join_rows(fact.rows, all_f, ["K", "C"], dim.rows, all_d, ["K", "C"], "inner", "all", fact_cb=fact.cb, dim_cb=dim.cb)
    assert both == [(0, 2), (1, 1), (3, 1)]
    assert joined_model_rows(fact.rows, dim.rows, [(2, -1)], "d.") == [dict(fact.rows[2], **{"d." + k: None for k in dim.rows[0]})]


@pytest.mark.parametrize("name", CASES)
def test_three_models_agree_pair_for_pair(name):
    """expected_join_rows against rows_model + expected_expand (duplicates="all") and map_model + expected_join
    ("first"), for every fixture, key choice, fact filter and join type."""
    c = case(name)
    for fnames, dnames in c.keys:
        m, mp, lists = rows_model(c.dim.cb, c.dim.rows, dnames, c.fact.plan, fnames)
        m2, mp2 = map_model(c.dim.cb, c.dim.rows, dnames, c.fact.plan, fnames)
        assert mp == mp2
        for filters in fact_filters_of(name):
            keep = keep_of(c.fact, filters)
            for how in ("inner", "left"):
                wf, wm = expected_expand(c.fact.cb, c.fact.rows, keep, fnames, lists, how)
                assert model_pairs(c, fnames, dnames, how, "all", keep) == list(zip(wf.tolist(), wm.tolist())), (fnames, how)
                idx, match, _ = expected_join(c.fact.cb, c.fact.rows, keep, fnames, mp, how)
                assert model_pairs(c, fnames, dnames, how, "first", keep) == list(zip(idx.tolist(), match.tolist())), (fnames, how)


# ---------------------------------------------------------------------------------------------
# The fixtures: no GPU test over them can pass vacuously
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_has_matched_unmatched_and_null_rows_and_fans_out(name):
    c = case(name)
    assert 0 < len(c.fact.rows) <= 1000 and 0 < len(c.dim.rows) <= 1000
    for fnames, dnames in c.keys:
        for filters in fact_filters_of(name):
            keep = keep_of(c.fact, filters)
            assert 0 < keep.sum() and (not filters or keep.sum() < len(keep))
            left = model_pairs(c, fnames, dnames, "left", "all", keep)
            fkeys = [tuple(row_value(c.fact.cb, r, k) for k in fnames) for r in c.fact.rows]
            assert any(j >= 0 for _, j in left) and any(j < 0 and None not in fkeys[i] for i, j in left), (name, fnames)
            waived = c.waived[tuple(fnames)]
            if "fact_null" not in waived:
                assert any(None in fkeys[i] for i, _ in left), (name, fnames)
            else:
                assert any(row_value(c.dim.cb, r, dnames[0]) is None for r in c.dim.rows), (name, fnames)
            fan = Counter(i for i, j in left if j >= 0)      # dimension list length per matched fact row
            assert min(fan.values()) == 1 and max(fan.values()) > 64, (name, fnames)
            # more outputs than fact rows: the emit writes rows (and Seg_Id state) past the input row count
            assert len(left) > (keep.sum() if filters else len(c.fact.rows)), (name, fnames)
            inner = model_pairs(c, fnames, dnames, "inner", "all", keep)
            assert len(inner) > len({i for i, _ in inner}) > 0, (name, fnames)
            first = model_pairs(c, fnames, dnames, "left", "first", keep)
            assert len(first) == keep.sum() < len(left)


def test_narrow_fixture_ids_levels_and_the_segment_filter():
    """Both Seg_Id levels vary, the key is null on every P record and on every second C record."""
    c = case("narrow")
    rows = c.fact.rows
    ids = [r["Record_Id"] for r in rows]
    assert len(set(ids)) == len(ids)
    kept_ids = [i for i, k in zip(ids, keep_of(c.fact, SEGMENT_C)) if k]
    assert kept_ids != list(range(len(kept_ids)))   # behind the filtered selection of (b) a record id is no ordinal
    assert len({r["Seg_Id0"] for r in rows}) > 100 and len({r["Seg_Id1"] for r in rows}) > 100
    tn = [row_value(c.fact.cb, r, "TAXPAYER-NUM") for r in rows]
    assert all(v is None for v, r in zip(tn, rows) if r["STATIC_DETAILS"] is None)
    on_c = [v for v, r in zip(tn, rows) if r["STATIC_DETAILS"] is not None]
    assert all(v is not None for v in on_c[::2]) and all(v is None for v in on_c[1::2])
    assert {1, 2, 65, 321} <= set(NUM_FANOUTS.values())
    assert set(NUM_FANOUTS) - set(on_c) == {5, 6} and len(set(on_c) - set(NUM_FANOUTS)) > 100


def test_framed_fixture_differs_with_and_without_the_segment_map():
    """Records with the id 'X' have no active segment: their key is null with the map and a value without it."""
    a, b = case("framed_map").fact, case("framed_plain").fact
    assert a.data == b.data and len(a.rows) == len(b.rows) == FUZZ_N
    ka = [row_value(a.cb, r, "TAXPAYER-NUM") for r in a.rows]
    kb = [row_value(b.cb, r, "TAXPAYER-NUM") for r in b.rows]
    assert any(x is None and y is not None for x, y in zip(ka, kb)) and any(x is not None for x in ka)
    assert any(r["STATIC_DETAILS"] is None and r["CONTACTS"] is None for r in a.rows)
    assert all(r["STATIC_DETAILS"] is not None for r in b.rows)


def test_short_fixture_cuts_inside_and_in_front_of_both_keys():
    """NUM occupies bytes 4-6, TXT bytes 7-12."""
    c = case("short")
    assert c.fact.ln.tolist() == SHORT_CUTS and len(c.fact.rows) == len(SHORT_CUTS) == 14 + SHORT_REPEATS + 1
    for name, first, size in (("NUM", 4, 3), ("TXT", 7, 6)):
        assert any(first < n < first + size for n in SHORT_CUTS), name     # cut inside the key field
        assert any(n < first for n in SHORT_CUTS), name                    # cut in front of it
    num = [r["NUM"] for r in c.fact.rows]
    txt = [r["TXT"] for r in c.fact.rows]
    assert all((v is None) == (n < 7) for v, n in zip(num, SHORT_CUTS))    # cut anywhere inside NUM: null
    assert all((v is None) == (n < 7) for v, n in zip(txt, SHORT_CUTS))    # TXT that starts at the end is "", not null
    assert txt[1] == "abc" and txt[2] == "" and txt[12] == "abcde"          # cut inside TXT: the truncated value
    dim_txt = Counter(r["TXT"] for r in c.dim.rows)
    assert dim_txt["abc"] == 66 and dim_txt["abcdef"] == 1 and dim_txt["ab"] == 1 and dim_txt[""] == 2 and "abcde" not in dim_txt
    # the truncated value finds the dimension's whole "abc" rows
    pairs = model_pairs(c, ["TXT"], ["TXT"], "inner", "all")
    assert sum(i == 1 for i, _ in pairs) == 66 and not any(i == 12 for i, _ in pairs)
    # as the dimension: truncated keys in lists of more than 64 rows and of exactly one, for both keys
    cut_txt, cut_num = Counter(txt), Counter(num)
    assert cut_txt["abc"] == 2 + SHORT_REPEATS and cut_txt["zz"] == 1 and cut_txt["r"] == 1 and txt[-1] == "r" and "q" not in cut_txt
    assert cut_num[-77] == 3 + SHORT_REPEATS and cut_num[424] == 1 and cut_num[12345] == 4
    swapped = case("short_swapped")
    assert swapped.dim.data == c.fact.data and swapped.fact.data == c.dim.data
    assert swapped.waived == {("NUM",): set(), ("TXT",): {"fact_null"}}   # whole records hold no null string
