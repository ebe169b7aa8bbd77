"""Fan-out joins on the GPU (cbx_key_map_index_rows, cbx_join_records_expand through `KeyMap.index_rows`, the readers'
`join(..., duplicates="all")` / `join_count` and through the C ABI) against the contract: `rows_model` and
`expected_expand` of test_fanout.py over the ORACLE's rows of both files -- never the code under test.  Every test calls
a new entry point: none of them passes without the feature.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import keyset as K  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.reader import ReaderParameters  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_fanout import expected_expand, rows_model  # noqa: E402
from test_filter import row_value  # noqa: E402
from test_gpu_filter import narrow  # noqa: E402,F401  (fixture)
from test_gpu_keymap import SEL_KEYS, _cur, _joined_rows, _sel_arrays  # noqa: E402
from test_gpu_keyset_from import (NUM_COPYBOOK, PARAMS, TEXT_COPYBOOK, TEXT_WORDS, Side, _device, _text_records, dim,  # noqa: E402,F401
                                  probe)
from test_keyset import distinct_keys, expected_set_keep  # noqa: E402
from test_keyset_from import DIM_COPYBOOK, DIM_SIZE  # noqa: E402

COUNTS = [1, 63, 64, 65, 321]
HOW = {"inner": N.JOIN_INNER, "left": N.JOIN_LEFT}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------------------------
# Small files with chosen fan-outs: NUM_COPYBOOK records (K: a 4-byte binary key, C: 5 characters)
# ---------------------------------------------------------------------------------------------
def num_data(keys) -> bytes:
    return b"".join(int(v).to_bytes(4, "big", signed=True) + ("C" if i % 2 else "P").ljust(5).encode("cp037")
                    for i, v in enumerate(keys))


def reside(side: Side, data: bytes, rows=None) -> Side:
    """The same reader (and plan: a key map belongs to one) over other bytes."""
    part = object.__new__(Side)
    part.__dict__.update(side.__dict__)
    part.data = data
    part.rows = rows if rows is not None else RO.fixed_len_rows(side.cb, data, PARAMS)
    part.t = _device(data)
    return part


@pytest.fixture(scope="module")
def nums():
    """(fact reader, source reader) over NUM_COPYBOOK; `reside` gives them the bytes of a case."""
    f, s = Side(NUM_COPYBOOK, num_data([1])), Side(NUM_COPYBOOK, num_data([1]))
    yield f, s
    f.rd.close()
    s.rd.close()


def interleaved(fanouts: dict, seed=1):
    """Dimension keys with fanouts[key] rows each, shuffled so that no segment arrives in order."""
    keys = [k for k, c in fanouts.items() for _ in range(c)]
    np.random.default_rng(seed).shuffle(keys)
    return keys


def build(fact: Side, names, source: Side, snames, filters=(), **kw):
    """(key map on the device, {key: (first, count)}, {key: [ordinals]})."""
    m, mp, lists = rows_model(source.cb, source.rows, snames, fact.plan, names, filters)
    km = source.rd.key_map_of_device(source.t, len(source.data), snames, fact.rd, names, filters=list(filters) or None, **kw)
    return km, mp, lists


def check_lists(km, lists: dict, fact: Side = None, **kw):
    """The device lists against the model; rows[row_start[v]] == first_row[v] and the segment lengths equal n_rows (the
    payload as the lookup join reports it per fact row).  Returns (info, row_start, rows)."""
    assert not km.has_rows and km.row_lists() == (None, None)
    info = km.index_rows(**kw)
    assert km.has_rows and info.has_rows == 1
    total = sum(map(len, lists.values()))
    assert info.n_indexed_rows == total and info.n_short + info.n_lds + info.n_global == km.n_values == len(lists)
    assert info.n_short == sum(len(v) <= info.short_max for v in lists.values())
    assert info.n_lds == sum(info.short_max < len(v) <= info.lds_max for v in lists.values())
    assert info.n_global == sum(len(v) > info.lds_max for v in lists.values())
    rs, rows = km.row_lists()
    if not lists:
        assert rs is None and rows is None
        return info, None, None
    rs, rows = rs.cpu().numpy(), rows.cpu().numpy()
    assert len(rs) == km.n_values + 1 and rs[0] == 0 and rs[-1] == total == len(rows)
    segs = [rows[a:b].tolist() for a, b in zip(rs[:-1], rs[1:])]
    assert sorted(map(tuple, segs)) == sorted(map(tuple, lists.values()))
    if fact is not None:
        res = fact.rd._join_records(km, "inner", None, "first", fact.t, len(fact.data), len(fact.rows), _cur(), stride=fact.size,
                                    decode=False)
        payload = set(zip(res.match.cpu().tolist(), res.match_rows.cpu().tolist()))
        assert payload <= {(s[0], len(s)) for s in segs}
    return info, rs, rows


def check_expand(fact: Side, names, km, lists, how, keep_k=None, filters=None, first_record_id=0, rows_too=False):
    keep_k = np.ones(len(fact.rows), bool) if keep_k is None else keep_k
    want_f, want_m = expected_expand(fact.cb, fact.rows, keep_k, names, lists, how)
    # (the count-only form first: the plan's expand info afterwards is that of the join itself)
    counted = fact.rd.join_count_device(fact.t, len(fact.data), km, how, filters=filters)
    res = fact.rd.join_device(fact.t, len(fact.data), km, how, filters=filters, duplicates="all", first_record_id=first_record_id)
    T = len(want_f)
    assert res.selection["n"] == T == res.batch.n_rec and res.match_rows is None
    assert res.n_kept == len(set(want_f.tolist()))
    assert np.array_equal(res.match.cpu().numpy(), want_m), (names, how)
    assert np.array_equal(res.fact_row.cpu().numpy(), want_f), (names, how)
    assert np.array_equal(res.selection["record_id"][:T].cpu().numpy(), first_record_id + want_f)
    assert counted == (T, res.n_kept)
    if rows_too:
        assert res.batch.to_rows() == [fact.rows[i] for i in want_f]
    return res, want_f, want_m


def raw_expand(fact: Side, km, how, capacity, with_fact_row=True, n_rec=None, plan=None):
    """cbx_join_records_expand through ctypes into sentinel-filled buffers: (rc, n_out, n_kept, selection, match, fact)."""
    L = N.load()
    n = len(fact.rows) if n_rec is None else n_rec
    out, cs = fact.rd._empty_selection(max(capacity, 1), fact.t.device)
    for k in SEL_KEYS:
        out[k].fill_(-9)
    match = torch.full((max(1, capacity),), -7, dtype=torch.int64, device="cuda")
    frow = torch.full((max(1, capacity),), -7, dtype=torch.int64, device="cuda")
    no, nk = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.cbx_join_records_expand(plan or fact.rd.native.handle, fact.t.data_ptr(), len(fact.data), None, None, None, n, fact.size, 0,
                                   0, None, None, None, 0, km.handle if km is not None else None, HOW[how], ctypes.byref(cs),
                                   capacity, ctypes.byref(no), ctypes.byref(nk), match.data_ptr(),
                                   frow.data_ptr() if with_fact_row else None, None)
    torch.cuda.synchronize()
    return rc, no.value, nk.value, out, match, frow


def untouched(out, match, frow):
    return all(bool((out[k] == -9).all()) for k in SEL_KEYS) and bool((match == -7).all()) and bool((frow == -7).all())


# ---------------------------------------------------------------------------------------------
# Lists
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_lists_source_record_counts(probe, dim, n):  # noqa: F811
    for snames, names in ((["D-BR"], ["BR-ID"]), (["D-NAME"], ["NAME"])):   # a numeric key, a string key
        km, mp, lists = build(probe, names, dim.first(n), snames)
        with km:
            check_lists(km, lists, probe)
            assert km.index_rows().n_indexed_rows == sum(map(len, lists.values()))   # twice: nothing happens


def test_segment_lengths_one_two_and_all_rows_on_one_key(nums):
    nf, ns = nums
    fact = reside(nf, num_data([5, 6, 7, 8]))
    for fan in ({5: 1, 6: 2}, {7: 321}, {5: 1, 6: 2, 7: 318}):
        src = reside(ns, num_data(interleaved(fan)))
        km, mp, lists = build(fact, ["K"], src, ["K"])
        with km:
            check_lists(km, lists, fact)
            assert sorted(len(v) for v in lists.values()) == sorted(fan.values())
            for how in ("inner", "left"):
                check_expand(fact, ["K"], km, lists, how, rows_too=True)


def test_both_sort_path_boundaries_and_grid_independence(nums):
    """Segments of short_max, short_max + 1, lds_max and lds_max + 1 rows (and 1, 2, 3): each of the three paths runs;
    max_workgroups = 1 and the default give identical bytes."""
    nf, ns = nums
    fact = reside(nf, num_data([1, 2, 3, 10, 11, 12, 20, 21, 22, 99]))
    with ns.rd.key_map_of_device(ns.t, len(ns.data), ["K"], nf.rd) as tiny:
        bounds = tiny.rows_info()
    s, l = bounds.short_max, bounds.lds_max
    assert 0 < s < l and bounds.has_rows == 0
    fan = {1: 1, 2: 2, 3: 3, 10: s - 1, 11: s, 12: s + 1, 20: l - 1, 21: l, 22: l + 1}
    src = reside(ns, num_data(interleaved(fan, seed=4)))
    got = []
    for kw in (dict(max_workgroups=1), dict()):
        km, mp, lists = build(fact, ["K"], src, ["K"])
        with km:
            info, rs, rows = check_lists(km, lists, fact, **kw)
            assert (info.n_short, info.n_lds, info.n_global) == (5, 3, 1)   # each of the three paths ran
            # (index_rows runs once per map, and the numbering of a set's values is the distinct pass's claim order, which
            # differs from build to build: the bytes compared are the segments in the order of their first ordinal)
            segs = sorted((rows[a:b] for a, b in zip(rs[:-1], rs[1:])), key=lambda s_: int(s_[0]))
            got.append(np.concatenate(segs).tobytes())
            if not kw:
                res, wf, wm = check_expand(fact, ["K"], km, lists, "left")
                assert len(wf) == sum(fan.values()) + 1
    assert got[0] == got[1]


def test_lists_source_filter_composite_selection_source_and_empty(probe, dim, narrow, nums):  # noqa: F811
    # a source filter; a four-key composite
    for snames, names, filters in ((["D-BR"], ["BR-ID"], [F.IsNotNull("D-RATE")]),
                                   (["D-BR", "D-NAME", "D-AMT", "D-BIG"], ["BR-ID", "NAME", "AMT-01", "ACCT-NO"], [])):
        km, mp, lists = build(probe, names, dim, snames, filters)
        with km:
            check_lists(km, lists, probe)
            check_expand(probe, names, km, lists, "inner")
    # a variable-length source through a selection: the ordinals index the selection
    rd, p, raw, rows = narrow
    fact = reside(nums[0], num_data([1000 + 37 * k for k in range(0, 400, 3)]))
    m, mp, lists = rows_model(rd.copybook, rows, ["SEGMENT-ID"], fact.plan, ["C"])
    with rd.key_map_of(raw, ["SEGMENT-ID"], fact.rd, ["C"]) as km:
        assert max(map(len, lists.values())) > 64
        check_lists(km, lists, fact)
        for how in ("inner", "left"):
            res, wf, wm = check_expand(fact, ["C"], km, lists, how)
        assert res.dimension().to_rows() == [rows[j] for j in wm if j >= 0]
    # an empty source: an empty map, no lists, nothing launched; LEFT keeps every row with -1
    km, mp, lists = build(probe, ["BR-ID"], dim.first(0), ["D-BR"])
    with km:
        info, rs, rws = check_lists(km, lists)
        assert info.n_indexed_rows == 0 and rs is None
        res, wf, wm = check_expand(probe, ["BR-ID"], km, lists, "left")
        assert len(wm) == 321 and (wm == -1).all()
        assert probe.rd.join_count_device(probe.t, len(probe.data), km, "inner") == (0, 0)


# ---------------------------------------------------------------------------------------------
# Expand: record counts, nulls, no match
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dup(dim):  # noqa: F811
    """321 DIM records over 7 distinct D-BR values with uneven fan-outs."""
    seen = {}
    for i in range(321):
        v = row_value(dim.cb, dim.rows[i], "D-BR")
        if v is not None:
            seen.setdefault(v, i)
    recs = [dim.data[DIM_SIZE * i:DIM_SIZE * (i + 1)] for i in list(seen.values())[:7]]
    side = Side(DIM_COPYBOOK, b"".join(recs[(i * i) % 7] for i in range(321)))
    yield side
    side.rd.close()


@pytest.mark.parametrize("n", COUNTS)
def test_expand_fact_record_counts(probe, dup, n):  # noqa: F811
    fact = probe.first(n)
    km, mp, lists = build(fact, ["BR-ID"], dup, ["D-BR"])
    with km:
        check_lists(km, lists, fact)
        for how in ("inner", "left"):
            res, wf, wm = check_expand(fact, ["BR-ID"], km, lists, how, rows_too=n == 321)
            # without d_fact_row: the same selection and match
            rc, no, nk, out, match, frow = raw_expand(fact, km, how, max(len(wf), 1), with_fact_row=False)
            assert rc == 0 and (no, nk) == (len(wf), len(set(wf.tolist())))
            assert np.array_equal(match[:no].cpu().numpy(), wm) and bool((frow == -7).all())
            assert np.array_equal(out["record_id"][:no].cpu().numpy(), wf)
            if n == 321 and how == "left":
                assert (wm == -1).any() and len(wf) > 321   # null keys and rows with no match stay, the others fan out


# ---------------------------------------------------------------------------------------------
# Expand: window edges, skew, selectivity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [63, 64, 65, 129])
def test_a_kept_row_fills_or_straddles_a_waves_window(nums, c):
    """Key 7 has c rows; the fact rows put it first, in the middle, last and alone among rows of fan-out 1 and 2, and
    a tail of fan-out-1 rows brings T to one below, exactly and one above a multiple of 64."""
    nf, ns = nums
    fan = {7: c, 1: 1, 2: 2}
    src = reside(ns, num_data(interleaved(fan, seed=c)))
    km, mp, lists = build(nf, ["K"], src, ["K"])
    with km:
        check_lists(km, lists)
        for keys in ([7, 1, 2, 1], [1, 2, 7, 1, 1, 2], [1, 1, 2, 7], [7], [7, 7]):
            t0 = sum(fan[k] for k in keys)
            for target in (63, 0, 1):
                fact = reside(nf, num_data(keys[:-1] + [1] * ((target - t0) % 64) + keys[-1:]))
                res, wf, wm = check_expand(fact, ["K"], km, lists, "inner")
                assert len(wf) % 64 == target and fact.rd.join_expand_info().max_fanout == c


def test_left_with_matched_and_unmatched_rows_alternating(nums):
    nf, ns = nums
    src = reside(ns, num_data(interleaved({2: 2, 3: 3, 5: 70}, seed=9)))
    fact = reside(nf, num_data([(2, 100, 3, 101, 5, 102)[i % 6] for i in range(131)]))
    km, mp, lists = build(fact, ["K"], src, ["K"])
    with km:
        check_lists(km, lists, fact)
        res, wf, wm = check_expand(fact, ["K"], km, lists, "left", rows_too=True)
        assert (wm == -1).sum() == 65 and len(wf) > 131
        check_expand(fact, ["K"], km, lists, "inner")


def test_skew_a_hot_key_on_every_row_on_the_first_and_on_the_last(nums):
    """65 fact rows that all match the 321-row key: 20,865 outputs (the Python retry sizes them); the hot key only on the
    first and only on the last fact row."""
    nf, ns = nums
    src = reside(ns, num_data(interleaved({7: 321, 1: 1, 2: 2}, seed=2)))
    km, mp, lists = build(nf, ["K"], src, ["K"])
    with km:
        check_lists(km, lists)
        for keys in ([7] * 65, [7] + [1, 2, 50] * 40, [1, 2, 50] * 40 + [7]):
            fact = reside(nf, num_data(keys))
            for how in ("inner", "left"):
                res, wf, wm = check_expand(fact, ["K"], km, lists, how)
            info = fact.rd.join_expand_info()
            assert info.max_fanout == 321 and info.n_out == len(wf) and info.emit_grid == -(-len(wf) // info.outputs_per_workgroup)
        assert len(expected_expand(fact.cb, reside(nf, num_data([7] * 65)).rows, np.ones(65, bool), ["K"], lists, "inner")[0]) == 20865


@pytest.fixture(scope="module")
def big(nums):
    """70,000 fact rows with the keys 0 .. 69,999 (the oracle's rows computed once), on both readers."""
    nf, ns = nums
    data = num_data(range(70000))
    fact = reside(nf, data)
    kv = np.array([row_value(fact.cb, r, "K") for r in fact.rows])
    assert np.array_equal(kv, np.arange(70000))
    return fact, reside(ns, data, fact.rows), kv


def test_selectivity_the_filter_keeps_one_row_of_seventy_thousand(nums, big):
    fact, _, kv = big
    src = reside(nums[1], num_data(interleaved({0: 3, 35000: 2, 69999: 4, 5: 1}, seed=6)))
    km, mp, lists = build(fact, ["K"], src, ["K"])
    with km:
        check_lists(km, lists)
        for v, c in ((0, 3), (35000, 2), (69999, 4), (123, 0)):
            filters = [F.EqualTo("K", v)]
            keep_k = kv == v   # (the oracle's key column)
            assert keep_k.sum() == 1
            res, wf, wm = check_expand(fact, ["K"], km, lists, "inner", keep_k, filters)
            assert len(wf) == c
            res, wf, wm = check_expand(fact, ["K"], km, lists, "left", keep_k, filters)
            assert len(wf) == max(c, 1) and (wf == v).all()


def test_seventy_thousand_rows_all_kept_with_fan_out_one(big):
    fact, src, _ = big
    km, mp, lists = build(fact, ["K"], src, ["K"], max_values=70000)
    with km:
        info, rs, rows = check_lists(km, lists)
        assert info.n_short == 70000
        res, wf, wm = check_expand(fact, ["K"], km, lists, "inner")
        assert len(wf) == 70000 and np.array_equal(wf, wm)
        assert fact.rd.join_expand_info().max_fanout == 1


# ---------------------------------------------------------------------------------------------
# Equivalence with the lookup join; capacity; state
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def uniq(dim):  # noqa: F811
    """The DIM records with the first row of every D-BR value only: a unique dimension."""
    seen, recs = set(), []
    for i, r in enumerate(dim.rows):
        v = row_value(dim.cb, r, "D-BR")
        if v is not None and v not in seen:
            seen.add(v)
            recs.append(dim.data[DIM_SIZE * i:DIM_SIZE * (i + 1)])
    side = Side(DIM_COPYBOOK, b"".join(recs))
    yield side
    side.rd.close()


def test_a_unique_dimension_is_bit_identical_to_the_lookup_join(probe, uniq):  # noqa: F811
    km, mp, lists = build(probe, ["BR-ID"], uniq, ["D-BR"])
    zd = distinct_keys(probe.cb, probe.rows, ["ZD-01"])[::2]
    with km, probe.rd.key_set(["ZD-01"], zd) as other:
        assert km.n_duplicate_keys == 0
        check_lists(km, lists, probe)
        for filters in (None, [F.IsNotNull("AMT-01"), F.NotInSet(other)]):
            for how in ("inner", "left"):
                ref = probe.rd.join_device(probe.t, len(probe.data), km, how, filters=filters, first_record_id=100)
                res = probe.rd.join_device(probe.t, len(probe.data), km, how, filters=filters, duplicates="all", first_record_id=100)
                assert ref.selection["n"] == res.selection["n"] == res.n_kept > 0
                for a, b in zip(_sel_arrays(ref.selection), _sel_arrays(res.selection)):
                    assert a.tobytes() == b.tobytes()
                assert ref.match.cpu().numpy().tobytes() == res.match.cpu().numpy().tobytes()
                assert res.batch.to_rows() == ref.batch.to_rows()
        keep_k = expected_set_keep(probe.cb, probe.rows, [F.IsNotNull("AMT-01")], [(["ZD-01"], zd, 1)])
        check_expand(probe, ["BR-ID"], km, lists, "left", keep_k, [F.IsNotNull("AMT-01"), F.NotInSet(other)])


def test_capacity_count_only_retry_and_overflow(nums):
    """20 fact rows, ten of them on a 321-row key: more outputs than fact rows."""
    nf, ns = nums
    probe = reside(nf, num_data([7] * 10 + [1, 50] * 5))
    n = len(probe.rows)
    km, mp, lists = build(probe, ["K"], reside(ns, num_data(interleaved({7: 321, 1: 1}, seed=8))), ["K"])
    with km:
        check_lists(km, lists, probe)
        for how in ("inner", "left"):
            wf, wm = expected_expand(probe.cb, probe.rows, np.ones(n, bool), ["K"], lists, how)
            T, kept = len(wf), len(set(wf.tolist()))
            assert T > n   # the first attempt of the Python path (capacity n_rec) does not fit
            rc, no, nk, out, match, frow = raw_expand(probe, km, how, T - 1)
            assert rc == N.CBX_E_CAPACITY and (no, nk) == (T, kept) and untouched(out, match, frow)
            msg = N.load().cbx_last_error().decode()
            assert f"{T} output rows exceed out_capacity {T - 1}" in msg
            rc, no, nk, out, match, frow = raw_expand(probe, km, how, T)
            assert rc == 0 and (no, nk) == (T, kept)
            assert np.array_equal(match.cpu().numpy(), wm) and np.array_equal(frow.cpu().numpy(), wf)
            # count-only: out NULL, capacity 0, no match array
            L = N.load()
            no, nk = ctypes.c_int64(-1), ctypes.c_int64(-1)
            rc = L.cbx_join_records_expand(probe.rd.native.handle, probe.t.data_ptr(), len(probe.data), None, None, None, n, probe.size, 0, 0,
                                           None, None, None, 0, km.handle, HOW[how], None, 0, ctypes.byref(no), ctypes.byref(nk), None,
                                           None, None)
            assert rc == 0 and (no.value, nk.value) == (T, kept)
            check_expand(probe, ["K"], km, lists, how)   # the retry
            with pytest.raises(K.JoinOverflow) as e:
                probe.rd.join_device(probe.t, len(probe.data), km, how, duplicates="all", max_rows=T - 1)
            assert (e.value.needed, e.value.max_rows) == (T, T - 1)
            res = probe.rd.join_device(probe.t, len(probe.data), km, how, duplicates="all", max_rows=T)
            assert res.selection["n"] == T


def test_state_and_argument_refusals(probe, dup, dim):  # noqa: F811
    L = N.load()
    km, mp, lists = build(probe, ["BR-ID"], dup, ["D-BR"])
    with km:
        # expand before index_rows
        rc, no, nk, out, match, frow = raw_expand(probe, km, "inner", 321)
        assert rc == N.CBX_E_STATE and "no row lists" in L.cbx_last_error().decode() and untouched(out, match, frow)

        def index(plan=km._source_handle, n_rec=km._n_rec):
            return L.cbx_key_map_index_rows(km.handle, plan, ctypes.byref(km._source_table), km._data_ptr, km._n_bytes, None, None,
                                            None, n_rec, km._stride, 0, None, 0, None, None)

        for kw, word in ((dict(n_rec=320), "320 source records, the map was built from 321"),
                         (dict(plan=probe.rd.native.handle), "source_plan is not the plan the map was built from")):
            assert index(**kw) == N.CBX_E_ARGUMENT and word in L.cbx_last_error().decode()
            assert not km.has_rows
        assert L.cbx_key_map_index_rows(None, km._source_handle, None, None, 0, None, None, None, 0, 0, 0, None, 0, None, None) == N.CBX_E_ARGUMENT
        assert index() == 0 and km.has_rows
        first = km.rows_info()
        assert index() == 0   # twice: CBX_OK, nothing launched
        again = km.rows_info()
        assert (again.n_indexed_rows, again.n_short, again.n_lds, again.n_global) == (first.n_indexed_rows, first.n_short, first.n_lds,
                                                                                      first.n_global)
        # the lookup join's own refusals, message for message
        rc, *_ = raw_expand(probe, None, "inner", 321)
        assert rc == N.CBX_E_ARGUMENT and "cbx_join_records: map: null" in L.cbx_last_error().decode()
        rc, *_ = raw_expand(probe, km, "inner", 321, plan=dim.rd.native.handle)
        assert rc == N.CBX_E_ARGUMENT and "built for another probe plan" in L.cbx_last_error().decode()
        rc, *_ = raw_expand(probe, km, "inner", 400, n_rec=400)
        assert rc == N.CBX_E_ARGUMENT and "exceed n_bytes" in L.cbx_last_error().decode()
        rc, no, nk, *_ = raw_expand(probe, km, "inner", 1, n_rec=0)
        assert rc == 0 and (no, nk) == (0, 0)   # n_rec == 0 launches nothing
    with pytest.raises(ValueError, match="closed"):
        km.index_rows()
    with pytest.raises(ValueError, match="closed"):
        probe.rd.join_device(probe.t, len(probe.data), km, duplicates="all")


# ---------------------------------------------------------------------------------------------
# Decode, code pages, info, pass times
# ---------------------------------------------------------------------------------------------
def test_rows_and_dimension_against_both_oracles(probe, dup):  # noqa: F811
    km, mp, lists = build(probe, ["BR-ID"], dup, ["D-BR"])
    with km:
        for how in ("inner", "left"):
            wf, wm = expected_expand(probe.cb, probe.rows, np.ones(321, bool), ["BR-ID"], lists, how)
            res = probe.rd.join(probe.data, km, how, duplicates="all")   # (builds the lists on first use)
            assert km.has_rows and np.array_equal(res.fact_row.cpu().numpy(), wf) and np.array_equal(res.match.cpu().numpy(), wm)
            assert res.batch.to_rows() == [probe.rows[i] for i in wf]
            assert res.dimension().to_rows() == [dup.rows[j] for j in wm if j >= 0]
            assert res.rows() == _joined_rows(probe.rows, wf, wm, dup.rows)
            assert res.rows(prefix="d.") == _joined_rows(probe.rows, wf, wm, dup.rows, "d.")
        assert (wm == -1).any() and len(wf) > 321
        assert probe.rd.join_count(probe.data, km, "left") == (len(wf), len(set(wf.tolist())))
    with pytest.raises(ValueError, match="closed"):
        res.dimension()


def test_cp037_source_against_a_windows_1252_probe():
    rng = np.random.default_rng(5)
    swords = [TEXT_WORDS[int(k)] for k in rng.integers(0, 7, 130)]
    pwords = [TEXT_WORDS[int(k)] for k in rng.integers(3, 10, 321)]
    source = Side(TEXT_COPYBOOK, _text_records(swords, "cp037", b"\x40", 1),
                  ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", string_trimming_policy="both"))
    fact = Side(TEXT_COPYBOOK, _text_records(pwords, "cp1252", b" ", 2),
                ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset="windows-1252",
                                 string_trimming_policy="both"))
    for names in (["T"], ["T", "N"]):
        km, mp, lists = build(fact, names, source, names)
        with km:
            check_lists(km, lists, fact)
            res, wf, wm = check_expand(fact, names, km, lists, "inner", rows_too=True)
            if names == ["T"]:
                assert len(wf) > len(set(wf.tolist())) > 0
                assert res.dimension().to_rows() == [source.rows[j] for j in wm]
    source.rd.close()
    fact.rd.close()


def test_expand_info_and_pass_times(probe, dup):  # noqa: F811
    L = N.load()
    km, mp, lists = build(probe, ["BR-ID"], dup, ["D-BR"])
    with km:
        assert km.index_rows().index_ms == 0.0
        wf, wm = expected_expand(probe.cb, probe.rows, np.ones(321, bool), ["BR-ID"], lists, "inner")
        probe.rd.join_device(probe.t, len(probe.data), km, duplicates="all")
        info = probe.rd.join_expand_info()
        counts = np.bincount(wf)
        assert (info.n_out, info.n_kept, info.max_fanout) == (len(wf), len(set(wf.tolist())), counts.max())
        assert info.outputs_per_workgroup == 256 and info.emit_grid == -(-len(wf) // 256) and info.host_waits == 1
        assert probe.rd.join_expand_pass_times() == (0.0, 0.0, 0.0)
        assert probe.rd.join_count_device(probe.t, len(probe.data), km) == (len(wf), info.n_kept)
        assert probe.rd.join_expand_info().emit_grid == 0   # the count-only form does not launch the emit
    for rd in (dup.rd, probe.rd):
        N.check(L.cbx_plan_set_profiling(rd.native.handle, 1))
    try:
        km, mp, lists = build(probe, ["BR-ID"], dup, ["D-BR"])
        with km:
            assert km.index_rows().index_ms > 0 and km.rows_info().index_ms > 0
            probe.rd.join_device(probe.t, len(probe.data), km, duplicates="all")
            assert all(x >= 0 for x in probe.rd.join_expand_pass_times()) and probe.rd.join_expand_pass_times()[2] > 0
            assert probe.rd.join_expand_info().host_waits == 2   # (the emit's duration is read after one more wait)
    finally:
        for rd in (dup.rd, probe.rd):
            N.check(L.cbx_plan_set_profiling(rd.native.handle, 0))
