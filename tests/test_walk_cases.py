"""CPU: the inputs of the record-walk shape tests (tests/walk_cases.py).  The GPU module decodes wrapped
decoder slices, a dense string case and random layouts; a generator that emitted the wrong bytes, never a
null, never a long UTF-8 value or only one kind of layout would silently drop its coverage, so the
generators are pinned here against the oracle."""
from __future__ import annotations

import collections

import pytest

import staging_cases as S
import walk_cases as W
from cobrix_amd.plan import UnsupportedLayout, build_plan
from cobrix_amd.reader import ReaderParameters, parse_copybook_for
from oracle import oracle as O
from oracle import reader_oracle as RO


def _walk_plan(cb, p):
    return build_plan(cb, walk=True, variable_size_occurs=p.variable_size_occurs, string_views=1,
                      segment_field=p.segment_field, segment_redefine_map=p.segment_id_redefine_map or None)


def _events(cb, recs, var_size, active=None):
    return W.leaf_events(O.decode_records(cb, recs, variable_size_occurs=var_size, active_segments=active))


@pytest.mark.parametrize("how", W.WRAPPERS)
@pytest.mark.parametrize("sid", sorted(S.SLICE_TABLE))
def test_wrapped_slice_every_leaf_valid_and_null(sid, how):
    """Every leaf of every wrapped slice decodes to a value in some oracle row and, where it can be null,
    to null in some row: fixed-length records are whole, so there a string is never null and a number
    only where the fuzz's bytes for its shape can be malformed (a binary field never is)."""
    body, recs = W.wrapped_records(sid, how)
    p = W.wrapper_parameters(sid, how)
    cb = parse_copybook_for(W.copybook_text(body), p)
    plan = _walk_plan(cb, p)
    assert plan.walk is not None and plan.walk.variable_size_occurs == (how != "fixed")
    assert len(recs) == W.N_REC == 321
    if how == "fixed":
        assert {len(r) for r in recs} == {cb.record_size}
        assert cb.record_size == 2 * (1 + 2 * S.SLICE_TABLE[sid][2]) + 4
    else:
        again, full = W.records_and_full(body, W.N_REC, W.wrapped_seed(sid, how), ascii=sid[0] == "a")
        assert again == recs and all(len(r) <= f for r, f in zip(recs, full))
        assert 0.62 < sum(len(r) == f for r, f in zip(recs, full)) / W.N_REC < 0.8   # 70 % whole + cuts at the full length
        assert max(len(r) for r in recs) <= {"behind": 8, "inside": 5}[how] + {"behind": 1, "inside": 2}[how] * S.SLICE_TABLE[sid][2]
    ev = _events(cb, recs, how != "fixed")
    names = W.leaf_names(body)
    assert set(names) == set(ev) and len(names) == len(set(names))
    for name in names:
        rows = ev[name]
        assert any(r[2] for r in rows), f"{name}: never valid"
        if how != "fixed" or W.can_be_malformed(sid, name):
            assert any(not r[2] for r in rows), f"{name}: never null"
    if how != "behind":   # elements of the OCCURS: slot 1 is reached (slot > 0)
        inner = [n.name.replace("-", "_") for n in W.slice_nodes(sid)]
        assert all(any(r[1] > 0 for r in ev[n]) for n in inner)
    # TAIL, behind everything that moves: decoded from where the generator put it in every whole record
    if how != "fixed":
        tails = {r[0]: r for r in ev["TAIL"]}
        assert sum(1 for r in tails.values() if r[2]) > 0.6 * W.N_REC


def test_wrappers_shift_the_fields_through_every_alignment():
    body, recs = W.wrapped_records("f1", "behind")
    size = S.SLICE_TABLE["f1"][2]
    pads = collections.Counter(len(r) - size - 5 for r in recs if len(r) >= size + 5)
    assert set(pads) == {0, 1, 2, 3} and min(pads.values()) > 10
    assert max(len(r) for r in recs) <= 68


@pytest.mark.parametrize("place", W.DENSE_PLACES)
@pytest.mark.parametrize("page", W.DENSE_PAGES)
def test_dense_strings_cover_every_utf8_length(page, place):
    """The oracle's rows of the dense string case hold values of every UTF-8 length 0..12 from fields of at
    most 12 bytes, and values above 12 from 12 input bytes (the wave-wide fallback of the register path)."""
    two, three = W.multibyte(page)
    if page == "cp875":
        assert three == (0xCE, 0xCF, 0xDE, 0xE1, 0xFC)
    if page == "windows-1252":
        assert len(three) == 22
    for trim in W.TRIMS:
        body, recs = W.dense_records(page, place)
        p = W.dense_parameters(page, trim)
        cb = parse_copybook_for(W.copybook_text(body), p)
        assert _walk_plan(cb, p).walk is not None
        ev = _events(cb, recs, True)
        short = collections.Counter()
        over = 0
        for n in W.DENSE_SIZES:
            for r in ev[f"X{n:02d}"]:
                if r[2] and n <= 12:
                    short[len(r[3])] += 1
                    over += n == 12 and len(r[3]) > 12
        assert all(short[k] > 0 for k in range(13)), (trim, sorted(short.items()))
        assert over > 10, (trim, over)
        assert any(r[2] and len(r[3]) > 12 for r in ev["X13"]) and any(r[2] and len(r[3]) > 24 for r in ev["X24"])
        if place == "inside":
            assert all(any(r[1] == 1 for r in ev[f"X{n:02d}"]) for n in W.DENSE_SIZES)


@pytest.mark.parametrize("seed", W.SEEDS)
def test_random_layout_builds_a_walk_plan_and_frames(seed):
    """Every fixed seed builds a walk plan (none skipped); back to back, the oracle's
    VarOccursRecordExtractor finds exactly the lengths the generator emitted."""
    lay = W.random_layout(seed)
    assert len(W.leaf_names(lay.body)) <= W.MAX_LEAVES == 25
    p = ReaderParameters(**lay.options)
    cb = parse_copybook_for(lay.text, p)
    plan = _walk_plan(cb, p)
    assert plan.walk is not None
    names = {a.depending_on for a in _arrays(cb.ast) if a.depending_on}
    assert len(names) == lay.n_names <= W.MAX_NAMES
    recs = lay.records(W.N_REC, framed=False)
    got = RO.var_occurs_records(cb, b"".join(recs))
    assert [len(r) for r in got] == [len(r) for r in recs]
    assert got == recs
    assert len({len(r) for r in recs}) > 1
    # RDW records: 70 % whole, the others cut
    cut = lay.records(W.N_REC, framed=True)
    assert len(cut) == W.N_REC and min(len(r) for r in cut) >= 1


def _arrays(g):
    for c in g.children:
        if c.is_array:
            yield c
        if hasattr(c, "children"):
            yield from _arrays(c)


def test_random_layouts_cover_every_feature():
    lays = [W.random_layout(s) for s in W.SEEDS]
    assert len(lays) == 24
    count = collections.Counter(f for lay in lays for f in lay.features)
    assert all(count[f] >= 2 for f in W.FEATURES), {f: count[f] for f in W.FEATURES}
    assert set(count) <= set(W.FEATURES)
    assert any(lay.n_names == 8 for lay in lays)
    assert {lay.n_names for lay in lays} >= {1, 8}
    # the features are what the copybook holds, not what the generator meant to draw
    for lay in lays:
        cb = parse_copybook_for(lay.text, ReaderParameters(**lay.options))
        arrays = list(_arrays(cb.ast))
        by_dep = collections.Counter(a.depending_on for a in arrays if a.depending_on)
        assert ("shared_dependee" in lay.features) == any(v > 1 for v in by_dep.values())
        assert ("min_count_1" in lay.features) == any(a.depending_on and a.array_min_size == 1 for a in arrays)
        assert ("redefines" in lay.features) == any(c.redefines and not c.is_segment_redefine for c in cb.ast.children[0].children
                                                    if hasattr(c, "children"))
        assert ("segment_odo" in lay.features) == bool(lay.segments) == (len(cb.all_segment_redefines()) == 2)
        assert ("dep_string" in lay.features) == bool(lay.options.get("occurs_mappings"))


def test_a_ninth_name_is_refused():
    lay = W.random_layout(0, names=9)
    p = ReaderParameters(**lay.options)
    cb = parse_copybook_for(lay.text, p)
    with pytest.raises(UnsupportedLayout, match="more than 8 DEPENDING ON names"):
        _walk_plan(cb, p)
    ok = W.random_layout(0, names=8)
    assert _walk_plan(parse_copybook_for(ok.text, ReaderParameters(**ok.options)), p).walk is not None


def test_counts_are_drawn_in_range_out_of_range_and_null():
    """A dependee's bytes come from all three kinds of value (the framing test above checks that the generator
    then lays the arrays out as the reference does: null keeps the previous entry, out of range is the maximum)."""
    import numpy as np
    n = W.count_node("N", "comp3", 3)
    seen = collections.Counter()
    rng = np.random.default_rng(1)
    for _ in range(400):
        b, v = W.draw_count(rng, n)
        seen["null" if v is None else "in" if v <= 3 else "out"] += 1
        assert len(b) == 2
    assert min(seen["null"], seen["in"], seen["out"]) > 10
