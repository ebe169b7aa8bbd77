"""The lookup join (cbx_join_records) and the fan-out join (cbx_join_records_expand) over every kind of FACT source: a
selection of a variable-length reader with Seg_Id levels (the emit's `has_in` branch with n_state > 0), framed records
with and without a segment map (the `rec_off` branch, `segment` from the test pass's seg_out or -1), fixed-length records
with a segment map (the stride branch with seg_out), records cut short inside and in front of the key, and the whole-file
and C ABI entry points above them.

Every expectation is `expected_join_rows` of test_join_sources.py over the ORACLE's rows and framing of the fixture files
defined there -- never the code under test.  Everything is integers, bytes and decoded rows: all comparisons are exact.
"""
from __future__ import annotations

import ctypes
from collections import Counter

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from cobrix_amd import aggregate as A  # noqa: E402
from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.options import parse_options  # noqa: E402
from cobrix_amd.reader import VarLenNestedReader  # noqa: E402
from cobrix_amd.synth import RDW_NARROW_COPYBOOK  # noqa: E402
from cobrix_amd.topn import SortOrder as S  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_fanout import rows_model  # noqa: E402
from test_filter import py_keep, row_value  # noqa: E402
from test_gpu_fanout import check_lists  # noqa: E402
from test_gpu_filter import NARROW_OPTIONS, SHORT_COPYBOOK, narrow  # noqa: E402,F401  (fixture)
from test_gpu_keymap import SEL_KEYS, _cur, _fixed_segment_side, _sel_arrays  # noqa: E402
from test_gpu_keyset_from import NUM_COPYBOOK, Side  # noqa: E402
from test_join_sources import (NARROW_KEYS, SEGMENT_C, SHORT_KEYS, case, expected_join_rows, joined_model_rows, keep_of,  # noqa: E402
                               model_pairs)
from topn_cases import expected_indices  # noqa: E402

HOW = {"inner": N.JOIN_INNER, "left": N.JOIN_LEFT}
MODES = [(how, dup) for dup in ("first", "all") for how in ("inner", "left")]
ALL_KEYS = SEL_KEYS + ("seg_state",)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------------------------
# Sources on the device
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def numdim():
    """The NUM_COPYBOOK dimension of the narrow cases (fan-outs 1, 2, 3, 65, 200 and 321)."""
    src = case("narrow").dim
    side = Side(NUM_COPYBOOK, src.data)
    assert side.rows == src.rows
    yield side
    side.rd.close()


@pytest.fixture(scope="module")
def selected(narrow):  # noqa: F811
    """The `narrow` fixture's file behind select(): (reader, device bytes, valid bytes, selection, Case)."""
    rd, p, raw, rows = narrow
    c = case("narrow")
    assert raw == c.fact.data and rows == c.fact.rows
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    entries = rd.generate_index(t, len(raw), off, ln, 0)
    assert len(entries) > 2   # input_split_records = 300
    sel = rd.select(t, vb, off, ln, entries, 0)
    assert sel["n"] == len(rows)
    return rd, t, vb, sel, c


def key_map(dim: Side, dnames, fact_rd, fnames, **kw):
    return dim.rd.key_map_of_device(dim.t, len(dim.data), dnames, fact_rd, fnames, **kw)


def arrays(pairs):
    return (np.array([i for i, _ in pairs], dtype=np.int64), np.array([j for _, j in pairs], dtype=np.int64))


def check_join(res, pairs, all_pairs, dup, fact_rows, off, ln, ids, position=None):
    """A JoinResult against the model's pairs.  off / ln / ids: the oracle's framing and record id of every fact row;
    position[i]: the ordinal of fact row i in the input handed to the join (None: i itself)."""
    wf, wm = arrays(pairs)
    T = len(pairs)
    assert res.selection["n"] == T == res.batch.n_rec
    assert np.array_equal(res.match.cpu().numpy(), wm)
    assert np.array_equal(res.matched.cpu().numpy(), wm >= 0)
    if dup == "all":
        at = wf if position is None else position[wf]
        assert np.array_equal(res.fact_row.cpu().numpy(), at) and res.match_rows is None
        assert res.n_kept == len(set(wf.tolist()))
    else:
        fan = Counter(i for i, j in all_pairs if j >= 0)
        assert res.fact_row is None and res.n_kept == T == len(set(wf.tolist()))
        assert np.array_equal(res.match_rows.cpu().numpy(), np.array([fan[i] for i in wf.tolist()], dtype=np.int64))
    got = _sel_arrays(res.selection)
    assert np.array_equal(got[0], np.asarray(off, dtype=np.int64)[wf])
    assert np.array_equal(got[1], np.asarray(ln, dtype=np.int32)[wf])
    assert np.array_equal(got[2], np.asarray(ids, dtype=np.int64)[wf])
    assert res.batch.to_rows() == [fact_rows[i] for i in wf]
    return wf, wm


def check_every_mode(join, count, c, fnames, dnames, off, ln, ids, keep=None, position=None, dim_rows=None):
    """Lookup and fan-out, inner and left, and the count-only form: `join(how, dup)`, `count(how)`."""
    out = {}
    for how, dup in MODES:
        pairs = model_pairs(c, fnames, dnames, how, dup, keep)
        all_pairs = model_pairs(c, fnames, dnames, how, "all", keep)
        wf = [i for i, _ in all_pairs]
        assert count(how) == (len(all_pairs), len(set(wf))), (how, fnames)
        res = join(how, dup)
        check_join(res, pairs, all_pairs, dup, c.fact.rows, off, ln, ids, position)
        if dim_rows is not None:
            assert res.rows(prefix="d.") == joined_model_rows(c.fact.rows, dim_rows, pairs, "d."), (how, dup)
        out[how, dup] = res
    return out


def oracle_segments(rd, data, p) -> np.ndarray:
    """The segment-redefine index of every record from the oracle's active segment (-1: none)."""
    groups = [g.name.upper() for g in rd.plan.segment_groups]
    recs = RO.var_len_records(rd.copybook, data, p)
    return np.array([groups.index(r.active_segment.upper()) if r.active_segment is not None else -1 for r in recs], dtype=np.int32)


def state_of(sel, n_state):
    return sel["seg_state"][:sel["n"] * n_state].cpu().numpy().reshape(sel["n"], n_state)


# ---------------------------------------------------------------------------------------------
# (a) A selection of a reader with Seg_Id levels: the emit's has_in branch with n_state = 3
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fnames,dnames", NARROW_KEYS)
def test_selection_of_a_reader_with_seg_id_levels(selected, numdim, fnames, dnames):
    rd, t, vb, sel, c = selected
    ids = [r["Record_Id"] for r in c.fact.rows]
    n_state = 1 + rd.plan.options.segments.n_levels
    assert n_state == 3
    m, mp, lists = rows_model(c.dim.cb, c.dim.rows, dnames, c.fact.plan, fnames)
    with key_map(numdim, dnames, rd, fnames) as km:
        check_lists(km, lists)
        got = check_every_mode(lambda how, dup: rd.join_device(t, vb, sel, km, how, duplicates=dup),
                               lambda how: rd.join_count_device(t, vb, sel, km, how),
                               c, fnames, dnames, c.fact.off, c.fact.ln, ids, dim_rows=c.dim.rows)
        # every word of the Seg_Id state follows its fact row, on outputs past the input row count too
        whole = state_of(sel, n_state)
        seg = oracle_segments(rd, c.fact.data, c.fact.p)
        assert len(seg) == sel["n"] and set(seg.tolist()) == {0, 1}
        for (how, dup), res in got.items():
            wf, _ = arrays(model_pairs(c, fnames, dnames, how, dup))
            assert np.array_equal(state_of(res.selection, n_state), whole[wf]), (how, dup)
            assert np.array_equal(res.selection["segment"][:len(wf)].cpu().numpy(), seg[wf]), (how, dup)
        assert got["left", "all"].selection["n"] > sel["n"]
        assert len({tuple(r) for r in whole.tolist()}) > 100   # (the state differs from row to row)


# ---------------------------------------------------------------------------------------------
# (b) A filtered selection as the input: record ids are no ordinals
# ---------------------------------------------------------------------------------------------
def test_a_filtered_selection_equals_the_filter_inside_the_join(selected, numdim):
    rd, t, vb, sel, c = selected
    fnames, dnames = NARROW_KEYS[0]
    keep = keep_of(c.fact, SEGMENT_C)
    position = np.cumsum(keep) - 1   # ordinal of fact row i in the filtered selection
    ids = [r["Record_Id"] for r in c.fact.rows]
    s1 = rd.filter(t, vb, sel, SEGMENT_C)
    assert s1["unhandled"] == [] and s1["n"] == keep.sum() < sel["n"]
    with key_map(numdim, dnames, rd, fnames) as km:
        for how, dup in MODES:
            pairs = model_pairs(c, fnames, dnames, how, dup, keep)
            all_pairs = model_pairs(c, fnames, dnames, how, "all", keep)
            a = rd.join_device(t, vb, s1, km, how, duplicates=dup)
            b = rd.join_device(t, vb, sel, km, how, filters=SEGMENT_C, duplicates=dup)
            wf, wm = check_join(a, pairs, all_pairs, dup, c.fact.rows, c.fact.off, c.fact.ln, ids, position)
            check_join(b, pairs, all_pairs, dup, c.fact.rows, c.fact.off, c.fact.ln, ids)
            for x, y in zip(_sel_arrays(a.selection), _sel_arrays(b.selection)):
                assert x.tobytes() == y.tobytes()
            assert state_of(a.selection, 3).tobytes() == state_of(b.selection, 3).tobytes()
            assert a.match.cpu().numpy().tobytes() == b.match.cpu().numpy().tobytes()
            assert not np.array_equal(np.asarray(ids)[wf], position[wf])   # a record id is not the input ordinal
            n_all = (len(all_pairs), len({i for i, _ in all_pairs}))
            assert rd.join_count_device(t, vb, s1, km, how) == rd.join_count_device(t, vb, sel, km, how, filters=SEGMENT_C) == n_all


# ---------------------------------------------------------------------------------------------
# (c) The join's output as the next stage's input
# ---------------------------------------------------------------------------------------------
def test_a_fanned_out_selection_feeds_every_next_stage(selected, numdim):
    rd, t, vb, sel, c = selected
    fnames, dnames = NARROW_KEYS[0]
    cb = c.fact.cb
    pairs = model_pairs(c, fnames, dnames, "left", "all")
    wf, wm = arrays(pairs)
    out_rows = [c.fact.rows[i] for i in wf]          # repeated rows count as many times as they appear
    assert len(out_rows) > sel["n"] and max(Counter(wf.tolist()).values()) == 321
    with key_map(numdim, dnames, rd, fnames) as km:
        res = rd.join_device(t, vb, sel, km, "left", duplicates="all")
        fanned = res.selection
        assert fanned["n"] == len(out_rows)
        # filter
        for filters in ([F.IsNotNull("TAXPAYER-NUM")], [F.LessThan("TAXPAYER-NUM", 1200)], SEGMENT_C):
            s2 = rd.filter(t, vb, fanned, filters)
            assert s2["unhandled"] == []
            assert rd.decode_selected(t, vb, s2).to_rows() == [r for r in out_rows if py_keep(cb, r, filters)], filters
        # Top-N: the plain LIMIT and one order key (ties by position: a fact row's copies are exact ties)
        for orders, limit in (([], 100), ([], len(out_rows) + 5), ([S("TAXPAYER-NUM", False, False)], 70), ([S("TAXPAYER-NUM", True)], 400)):
            _, chosen = expected_indices(cb, out_rows, orders, limit)
            assert rd.top_n_device(t, vb, fanned, orders, limit).to_rows() == [out_rows[i] for i in chosen], (orders, limit)
        # aggregates
        vals = [row_value(cb, r, "TAXPAYER-NUM") for r in out_rows]
        agg = rd.aggregate_device(t, vb, fanned, [A.CountStar(), A.Count("TAXPAYER-NUM"), A.Sum("TAXPAYER-NUM")])
        assert agg.values == [len(out_rows), sum(v is not None for v in vals), sum(v for v in vals if v is not None)]
        # a second join over the fanned-out rows
        keep1 = np.ones(len(out_rows), bool)
        for how in ("inner", "left"):
            first = expected_join_rows(out_rows, keep1, fnames, c.dim.rows, np.ones(len(c.dim.rows), bool), dnames, how, "first",
                                       fact_cb=cb, dim_cb=c.dim.cb)
            f2, m2 = arrays(first)
            again = rd.join_device(t, vb, fanned, km, how, duplicates="first")
            assert again.selection["n"] == len(first) and np.array_equal(again.match.cpu().numpy(), m2)
            assert again.batch.to_rows() == [out_rows[i] for i in f2]
            assert np.array_equal(state_of(again.selection, 3), state_of(sel, 3)[wf[f2]])
            # fanned out once more, counted only: each of a fact row's c copies finds its c dimension rows again
            fan = Counter(i for i, j in pairs if j >= 0)
            unmatched = sum(j < 0 for _, j in pairs) if how == "left" else 0
            want = (sum(v * v for v in fan.values()) + unmatched, sum(fan.values()) + unmatched)
            assert want[0] > 100000 and rd.join_count_device(t, vb, fanned, km, how) == want


# ---------------------------------------------------------------------------------------------
# (d) Framed records without levels: the rec_off branch, with and without a segment map
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["framed_map", "framed_plain"])
def test_framed_records_with_and_without_a_segment_map(numdim, name):
    c = case(name)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, c.fact.p)
    assert rd.plan.options.has_segments == (name == "framed_map") and not rd.plan.seg_id_columns
    t = rd._device_file(c.fact.data)
    off, ln, vb = rd.frame_file(t, len(c.fact.data))
    assert np.array_equal(off.cpu().numpy(), c.fact.off) and np.array_equal(ln.cpu().numpy(), c.fact.ln)
    ids = 7 + np.arange(len(c.fact.rows))
    for fnames, dnames in c.keys:
        with key_map(numdim, dnames, rd, fnames) as km:
            got = check_every_mode(lambda how, dup: rd.join_device(t, vb, (off, ln), km, how, duplicates=dup, first_record_id=7),
                                   lambda how: rd.join_count_device(t, vb, (off, ln), km, how),
                                   c, fnames, dnames, c.fact.off, c.fact.ln, ids)
            seg = got["left", "all"].selection["segment"][:got["left", "all"].selection["n"]].cpu().numpy()
            if name == "framed_map":   # C, P and the unnamed 'X': the decoded rows above hold the redefine nulls
                assert set(seg.tolist()) == {-1, 0, 1}
            else:
                assert set(seg.tolist()) == {-1}
    rd.close()


def test_a_framing_on_a_reader_with_levels_is_refused(selected, numdim):
    rd, t, vb, sel, c = selected
    off, ln, _ = rd.frame_file(t, len(c.fact.data))
    with key_map(numdim, ["K"], rd, ["TAXPAYER-NUM"]) as km:
        for call in (lambda: rd.join_device(t, vb, (off, ln), km, duplicates="first"),
                     lambda: rd.join_device(t, vb, (off, ln), km, duplicates="all"),
                     lambda: rd.join_count_device(t, vb, (off, ln), km)):
            with pytest.raises(N.CbxError) as e:
                call()
            assert e.value.code == N.CBX_E_ARGUMENT and "select" in str(e.value)


# ---------------------------------------------------------------------------------------------
# (e) Fixed-length fact records with a segment map: the stride branch with seg_out
# ---------------------------------------------------------------------------------------------
def test_fixed_length_fact_with_a_segment_map(numdim):
    c = case("fixed_segment")
    fact = _fixed_segment_side()
    assert fact.data == c.fact.data and fact.rows == c.fact.rows
    assert fact.rd.plan.options.has_segments and not fact.rd.plan.seg_id_columns
    n = len(fact.rows)
    off, ln, ids = fact.size * np.arange(n), np.full(n, fact.size), 11 + np.arange(n)
    for fnames, dnames in c.keys:
        with key_map(numdim, dnames, fact.rd, fnames) as km:
            got = check_every_mode(lambda how, dup: fact.rd.join_device(fact.t, len(fact.data), km, how, duplicates=dup, first_record_id=11),
                                   lambda how: fact.rd.join_count_device(fact.t, len(fact.data), km, how),
                                   c, fnames, dnames, off, ln, ids)
            res = got["left", "all"]
            assert set(res.selection["segment"][:res.selection["n"]].cpu().tolist()) == {-1, 0, 1}
            rows = res.batch.to_rows()
            assert any(r["STATIC_DETAILS"] is not None for r in rows) and any(r["CONTACTS"] is not None for r in rows)
            assert any(r["STATIC_DETAILS"] is None and r["CONTACTS"] is None for r in rows)
    fact.rd.close()


# ---------------------------------------------------------------------------------------------
# (f) Records cut short, as the fact and as the dimension
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short():
    """(variable-length reader over the cut records, its device bytes / valid bytes / whole-file selection, the fixed
    side of whole records)."""
    c = case("short")
    rd = VarLenNestedReader(SHORT_COPYBOOK, c.fact.p)
    t, vb, sel = rd._whole_file_selection(c.fact.data, 0)
    whole = Side(SHORT_COPYBOOK, c.dim.data)
    assert whole.rows == c.dim.rows and sel["n"] == len(c.fact.rows)
    yield rd, t, vb, sel, whole
    rd.close()
    whole.rd.close()


@pytest.mark.parametrize("fnames,dnames", SHORT_KEYS)
def test_cut_records_as_the_fact(short, fnames, dnames):
    """NUM is null when the record ends inside or in front of it; TXT compares as the truncated value."""
    rd, t, vb, sel, whole = short
    c = case("short")
    ids = [r["Record_Id"] for r in c.fact.rows]
    with key_map(whole, dnames, rd, fnames) as km:
        check_every_mode(lambda how, dup: rd.join_device(t, vb, sel, km, how, duplicates=dup),
                         lambda how: rd.join_count_device(t, vb, sel, km, how),
                         c, fnames, dnames, c.fact.off, c.fact.ln, ids, dim_rows=c.dim.rows)
        off, ln = rd.frame_file(t, len(c.fact.data))[:2]   # the same records as a framing
        check_every_mode(lambda how, dup: rd.join_device(t, vb, (off, ln), km, how, duplicates=dup),
                         lambda how: rd.join_count_device(t, vb, (off, ln), km, how),
                         c, fnames, dnames, c.fact.off, c.fact.ln, ids)


@pytest.mark.parametrize("fnames,dnames", SHORT_KEYS)
def test_cut_records_as_the_dimension(short, fnames, dnames):
    rd, t, vb, sel, whole = short
    c = case("short_swapped")
    n = len(whole.rows)
    m, mp, lists = rows_model(c.dim.cb, c.dim.rows, dnames, c.fact.plan, fnames)
    with rd.key_map_of(c.dim.data, dnames, whole.rd, fnames) as km:
        assert km.source_info.n_null_rows == sum(r[dnames[0]] is None for r in c.dim.rows) > 0
        check_lists(km, lists)
        got = check_every_mode(lambda how, dup: whole.rd.join_device(whole.t, len(whole.data), km, how, duplicates=dup),
                               lambda how: whole.rd.join_count_device(whole.t, len(whole.data), km, how),
                               c, fnames, dnames, whole.size * np.arange(n), np.full(n, whole.size), np.arange(n),
                               dim_rows=c.dim.rows)
        wm = arrays(model_pairs(c, fnames, dnames, "inner", "all"))[1]
        assert got["inner", "all"].dimension().to_rows() == [c.dim.rows[j] for j in wm]


# ---------------------------------------------------------------------------------------------
# (g) Whole-file entry points
# ---------------------------------------------------------------------------------------------
def test_whole_file_join_and_join_count(selected, numdim):
    rd, t, vb, sel, c = selected
    fnames, dnames = NARROW_KEYS[0]
    raw = c.fact.data
    with key_map(numdim, dnames, rd, fnames) as km:
        for how, dup in MODES:
            for filters in (None, SEGMENT_C):
                a = rd.join(raw, km, how, filters=filters, duplicates=dup)
                b = rd.join_device(t, vb, sel, km, how, filters=filters, duplicates=dup)
                assert a.selection["n"] == b.selection["n"] > 0
                for x, y in zip(_sel_arrays(a.selection), _sel_arrays(b.selection)):
                    assert x.tobytes() == y.tobytes()
                assert state_of(a.selection, 3).tobytes() == state_of(b.selection, 3).tobytes()
                assert a.match.cpu().numpy().tobytes() == b.match.cpu().numpy().tobytes()
                assert a.batch.to_rows() == b.batch.to_rows()
                keep = keep_of(c.fact, filters or [])
                all_pairs = model_pairs(c, fnames, dnames, how, "all", keep)
                assert rd.join_count(raw, km, how, filters=filters) == (len(all_pairs), len({i for i, _ in all_pairs}))


def test_whole_file_join_honours_the_segment_filter(numdim):
    """segment_filter drops records in select(): the join runs over the rows of read(raw), whose record ids keep the
    numbering of the whole file."""
    fnames, dnames = NARROW_KEYS[0]
    p, _ = parse_options(dict(NARROW_OPTIONS, segment_filter="C"))
    raw = case("narrow").fact.data
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    rows = RO.var_len_rows(rd.copybook, raw, p)
    assert 0 < len(rows) < 1000 and all(r["STATIC_DETAILS"] is not None for r in rows)
    assert [r["Record_Id"] for r in rows] != list(range(len(rows)))
    assert rd.read(raw).to_rows() == rows
    dim = case("narrow").dim
    keep_f, keep_d = np.ones(len(rows), bool), np.ones(len(dim.rows), bool)
    with key_map(numdim, dnames, rd, fnames) as km:
        for how, dup in MODES:
            pairs = expected_join_rows(rows, keep_f, fnames, dim.rows, keep_d, dnames, how, dup, fact_cb=rd.copybook, dim_cb=dim.cb)
            all_pairs = expected_join_rows(rows, keep_f, fnames, dim.rows, keep_d, dnames, how, "all", fact_cb=rd.copybook,
                                           dim_cb=dim.cb)
            wf, wm = arrays(pairs)
            res = rd.join(raw, km, how, duplicates=dup)
            assert np.array_equal(res.match.cpu().numpy(), wm) and res.batch.to_rows() == [rows[i] for i in wf]
            assert np.array_equal(res.selection["record_id"][:len(wf)].cpu().numpy(), np.array([rows[i]["Record_Id"] for i in wf]))
            assert res.rows(prefix="d.") == joined_model_rows(rows, dim.rows, pairs, "d.")
            assert rd.join_count(raw, km, how) == (len(all_pairs), len({i for i, _ in all_pairs}))
    rd.close()


# ---------------------------------------------------------------------------------------------
# (h) The C ABI over a selection and over framing pointers
# ---------------------------------------------------------------------------------------------
PAD = 8   # entries past the capacity handed to the library: they keep their sentinels


def raw_join(rd, t, vb, km, how, dup, capacity, *, sel=None, framing=None, first_record_id=0, count_only=False):
    """cbx_join_records / cbx_join_records_expand through ctypes into sentinel-filled buffers of capacity + PAD rows:
    (rc, n_out, n_kept, out arrays, match, fact_row or match_rows)."""
    L = N.load()
    n_rec = sel["n"] if sel is not None else int(framing[0].numel())
    out, cs = rd._empty_selection(capacity + PAD, t.device)
    for k in ALL_KEYS:
        out[k].fill_(-9)
    match = torch.full((capacity + PAD,), -7, dtype=torch.int64, device="cuda")
    extra = torch.full((capacity + PAD,), -7, dtype=torch.int64, device="cuda")
    head = (rd.native.handle, t.data_ptr(), vb, ctypes.byref(sel["struct"]) if sel is not None else None,
            framing[0].data_ptr() if framing else None, framing[1].data_ptr() if framing else None, n_rec, 0, 0, first_record_id,
            None, None, None, 0, km.handle, HOW[how])
    no, nk = ctypes.c_int64(-1), ctypes.c_int64(-1)
    if dup == "all":
        if count_only:
            rc = L.cbx_join_records_expand(*head, None, 0, ctypes.byref(no), ctypes.byref(nk), None, None, None)
        else:
            rc = L.cbx_join_records_expand(*head, ctypes.byref(cs), capacity, ctypes.byref(no), ctypes.byref(nk), match.data_ptr(),
                                           extra.data_ptr(), None)
    else:
        rc = L.cbx_join_records(*head, ctypes.byref(cs), ctypes.byref(no), match.data_ptr(), extra.data_ptr(), None)
        nk.value = no.value
    torch.cuda.synchronize()
    return rc, no.value, nk.value, out, match, extra


def check_raw(got, pairs, all_pairs, dup, n_state, want):
    """Every word of the first n_out entries of all five arrays, and the sentinels past them.  want: the expected
    (rec_off, rec_len, record_id, segment, seg_state rows or None) of every fact row."""
    rc, no, nk, out, match, extra = got
    wf, wm = arrays(pairs)
    T = len(pairs)
    assert rc == 0 and (no, nk) == (T, len(set(wf.tolist())))
    for k, w in zip(SEL_KEYS, want[:4]):
        a = out[k].cpu().numpy()
        assert np.array_equal(a[:T], np.asarray(w)[wf].astype(a.dtype)), k
        assert (a[T:] == -9).all(), k
    st = out["seg_state"].cpu().numpy()
    if n_state:
        assert np.array_equal(st[:T * n_state].reshape(T, n_state), want[4][wf])
    assert (st[T * n_state:] == -9).all()
    m, x = match.cpu().numpy(), extra.cpu().numpy()
    assert np.array_equal(m[:T], wm) and (m[T:] == -7).all() and (x[T:] == -7).all()
    if dup == "all":
        assert np.array_equal(x[:T], wf)
    else:
        fan = Counter(i for i, j in all_pairs if j >= 0)
        assert np.array_equal(x[:T], np.array([fan[i] for i in wf.tolist()], dtype=np.int64))


def untouched(got):
    rc, no, nk, out, match, extra = got
    return all(bool((out[k] == -9).all()) for k in ALL_KEYS) and bool((match == -7).all()) and bool((extra == -7).all())


def test_c_abi_over_a_selection(selected, numdim):
    rd, t, vb, sel, c = selected
    fnames, dnames = NARROW_KEYS[0]
    n = sel["n"]
    want = [a for a in _sel_arrays(sel)] + [state_of(sel, 3)]
    assert np.array_equal(want[0], c.fact.off) and np.array_equal(want[2], [r["Record_Id"] for r in c.fact.rows])
    with key_map(numdim, dnames, rd, fnames) as km:
        km.index_rows()
        for how, dup in MODES:
            pairs = model_pairs(c, fnames, dnames, how, dup)
            all_pairs = model_pairs(c, fnames, dnames, how, "all")
            T = len(pairs)
            check_raw(raw_join(rd, t, vb, km, how, dup, max(T, n), sel=sel), pairs, all_pairs, dup, 3, want)
            if dup == "all":
                check_raw(raw_join(rd, t, vb, km, how, dup, T, sel=sel), pairs, all_pairs, dup, 3, want)   # the exact capacity
                got = raw_join(rd, t, vb, km, how, dup, T - 1, sel=sel)
                assert got[0] == N.CBX_E_CAPACITY and got[1:3] == (T, len({i for i, _ in pairs})) and untouched(got)
                got = raw_join(rd, t, vb, km, how, dup, 0, sel=sel, count_only=True)
                assert got[0] == 0 and got[1:3] == (T, len({i for i, _ in pairs})) and untouched(got)
        # out must not share arrays with in
        L = N.load()
        ns = ctypes.c_int64(-1)
        match = torch.empty(n, dtype=torch.int64, device="cuda")
        rc = L.cbx_join_records(rd.native.handle, t.data_ptr(), vb, ctypes.byref(sel["struct"]), None, None, n, 0, 0, 0, None, None, None,
                                0, km.handle, N.JOIN_LEFT, ctypes.byref(sel["struct"]), ctypes.byref(ns), match.data_ptr(), None, None)
        assert rc == N.CBX_E_ARGUMENT and "out must not share arrays with in" in L.cbx_last_error().decode()


def test_c_abi_over_framing_pointers(numdim):
    c = case("framed_map")
    fnames, dnames = NARROW_KEYS[0]
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, c.fact.p)
    t = rd._device_file(c.fact.data)
    off, ln, vb = rd.frame_file(t, len(c.fact.data))
    n = len(c.fact.rows)
    seg = oracle_segments(rd, c.fact.data, c.fact.p)
    assert set(seg.tolist()) == {-1, 0, 1}
    want = [c.fact.off, c.fact.ln, 7 + np.arange(n), seg, None]
    with key_map(numdim, dnames, rd, fnames) as km:
        km.index_rows()
        for how, dup in MODES:
            pairs = model_pairs(c, fnames, dnames, how, dup)
            all_pairs = model_pairs(c, fnames, dnames, how, "all")
            T = len(pairs)
            check_raw(raw_join(rd, t, vb, km, how, dup, max(T, n), framing=(off, ln), first_record_id=7), pairs, all_pairs, dup, 0, want)
            if dup == "all":
                got = raw_join(rd, t, vb, km, how, dup, T - 1, framing=(off, ln), first_record_id=7)
                assert got[0] == N.CBX_E_CAPACITY and got[1] == T and untouched(got)
    rd.close()


# ---------------------------------------------------------------------------------------------
# (i) Grid independence and the emit's window edges on a selection input
# ---------------------------------------------------------------------------------------------
def test_grid_independence_and_window_edges_on_a_selection(selected, numdim):
    rd, t, vb, sel, c = selected
    fnames, dnames = NARROW_KEYS[0]
    m, mp, lists = rows_model(c.dim.cb, c.dim.rows, dnames, c.fact.plan, fnames)
    left = model_pairs(c, fnames, dnames, "left", "all")
    per_row = Counter(i for i, _ in left)
    totals = np.cumsum([per_row[i] for i in range(sel["n"])])          # outputs of the first n + 1 fact rows
    limits = {}
    for target in (63, 0, 1):   # the smallest prefix past the first 321-row list whose outputs end there
        limits[target] = 1 + next(k for k, v in enumerate(totals.tolist()) if v > 400 and v % 64 == target)
    ids = [r["Record_Id"] for r in c.fact.rows]
    got = []
    for kw in (dict(max_workgroups=1), dict()):
        with key_map(numdim, dnames, rd, fnames, **kw) as km:
            info, rs, rows = check_lists(km, lists, **kw)
            segs = sorted((rows[a:b] for a, b in zip(rs[:-1], rs[1:])), key=lambda s_: int(s_[0]))
            outs = [np.concatenate(segs).tobytes()]
            for target, limit in limits.items():
                head = rd._top_n_records([], limit, None, t, vb, sel["n"], _cur(), sel=sel)   # the plain LIMIT: a prefix
                assert head["n"] == limit
                keep = np.arange(sel["n"]) < limit
                pairs = model_pairs(c, fnames, dnames, "left", "all", keep)
                assert len(pairs) % 64 == target and len(pairs) > 400
                res = rd.join_device(t, vb, head, km, "left", duplicates="all")
                check_join(res, pairs, pairs, "all", c.fact.rows, c.fact.off, c.fact.ln, ids)
                assert rd.join_expand_info().max_fanout == 321
                outs += [a.tobytes() for a in _sel_arrays(res.selection)] + [state_of(res.selection, 3).tobytes(),
                                                                            res.match.cpu().numpy().tobytes()]
            got.append(outs)
    assert got[0] == got[1]
