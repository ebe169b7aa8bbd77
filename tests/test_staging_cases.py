"""CPU: the inputs of the staging-path tests (tests/staging_cases.py).  The GPU module decodes the
decoder fuzz's copybooks slice by slice; a slicing bug there would silently drop decoder shapes from its
coverage, so the slices, the small copybooks and the file builders are pinned here against the oracle."""
from __future__ import annotations

import numpy as np
import pytest

import staging_cases as S
from oracle import oracle as O
from test_decode_fuzz import ASCII_COPYBOOK, FUZZ_COPYBOOK

SOURCES = {"fuzz": (FUZZ_COPYBOOK, False, S.fuzz_slices), "ascii": (ASCII_COPYBOOK, True, S.ascii_slices)}
PARSE_KW = {"fuzz": dict(code_page="cp037"), "ascii": {}}


def _names(text, ascii):
    return [p.name for p in S.leaves(S.parse(text, ascii))]


@pytest.mark.parametrize("which", sorted(SOURCES))
def test_slices_hold_every_leaf_once_in_order(which):
    text, ascii, get = SOURCES[which]
    sl = get()
    sizes = [S.parse(t, ascii).record_size for t in sl]
    assert all(0 < s <= S.SLICE_BYTES == 60 for s in sizes)
    assert sum(sizes) == S.parse(text, ascii).record_size
    assert [n for t in sl for n in _names(t, ascii)] == _names(text, ascii)
    # greedy: the next slice's first field would not have fitted
    for t, nxt, s in zip(sl, sl[1:], sizes):
        first = S.parse(S.HEADER + S.field_lines(nxt)[0] + "\n", ascii).record_size
        assert s + first > S.SLICE_BYTES
    if which == "fuzz":
        assert sizes == [57, 38, 47, 57, 54, 52, 59, 59, 59, 35]
        assert len(_names(text, ascii)) == 66
    else:
        assert sizes == [60, 57, 58, 53, 26, 38]


def test_slice_properties_the_gpu_tables_rely_on():
    """What tests/test_gpu_staging.py writes literally in its tables: which slices hold strings, which the
    floats, which a field wider than a 16-byte window, and the one slice of a single field."""
    fz = [S.parse(t) for t in S.fuzz_slices()]
    az = [S.parse(t, True) for t in S.ascii_slices()]
    assert [i for i, cb in enumerate(fz) if any(p.is_string for p in S.leaves(cb))] == [0]
    assert [i for i, cb in enumerate(az) if any(p.is_string for p in S.leaves(cb))] == [0]
    assert [p.name for p in S.leaves(az[0])][1:4] == ["N1", "N2", "N3"]
    assert [i for i, cb in enumerate(fz) if {"F01", "F02"} & {p.name for p in S.leaves(cb)}] == [9]
    wide = lambda cbs: [i for i, cb in enumerate(cbs) if max(p.data_size for p in S.leaves(cb)) > 16]   # noqa: E731
    assert wide(fz) == [1, 2, 3, 8, 9] and wide(az) == [0, 1, 2, 3, 5]
    assert [i for i, cb in enumerate(fz + az) if len(S.leaves(cb)) == 1] == [len(fz) + 5]
    assert S.parse(S.MIX).record_size == 16 and [p.data_size for p in S.leaves(S.parse(S.MIX))] == [3, 3, 3, 2, 4, 1]
    assert S.parse(S.TINY).record_size == 4 and [p.data_size for p in S.leaves(S.parse(S.TINY))] == [2, 2]


def test_slice_table_matches_the_slices():
    assert len(S.SLICE_TABLE) == len(S.fuzz_slices()) + len(S.ascii_slices())
    for sid, (source, index, size, plain, padded) in S.SLICE_TABLE.items():
        assert sid == source[0] + str(index)
        assert S.parse(S.slice_text(sid), source == "ascii").record_size == size
        assert plain == next(s for s in range(size, size + 9) if s % 4 == 0 and (s // 4) % 2 == 1)
        assert padded == (size + 15) // 16 * 16
        assert plain <= 252 and padded <= 252


@pytest.mark.parametrize("which", sorted(SOURCES))
def test_slice_decodes_equal_the_whole_copybook(which):
    """One seeded file of the whole copybook: every field's oracle events equal those of decoding the
    slice's byte columns through the slice."""
    text, ascii, get = SOURCES[which]
    kw = PARSE_KW[which]
    whole = S.parse(text, ascii, **kw)
    n = 300
    data = S.payloads(whole, n, 20261020, ascii)
    assert data.shape == (n, whole.record_size)
    want = S.field_events(O.decode_fixed(whole, data.tobytes()))
    assert list(want) == _names(text, ascii)
    lo = 0
    seen = []
    for t in get():
        cb = S.parse(t, ascii, **kw)
        cols = np.ascontiguousarray(data[:, lo:lo + cb.record_size])
        got = S.field_events(O.decode_fixed(cb, cols.tobytes()))
        for name, rows in got.items():
            assert len(rows) == n and rows == want[name], name
            seen.append(name)
        lo += cb.record_size
    assert lo == whole.record_size and seen == list(want)
    assert any(r[2] for rows in want.values() for r in rows)


def test_fixed_file_pads_around_the_same_payloads():
    cb = S.parse(S.fuzz_slices()[1])
    n, size = 130, cb.record_size
    base = np.frombuffer(S.fixed_file(cb, n, 5), dtype=np.uint8).reshape(n, size)
    assert np.array_equal(base, S.payloads(cb, n, 5))
    assert len({r.tobytes() for r in base}) > n // 2
    for start, end in ((3, 1), (0, 6), (2, 0)):
        rec = np.frombuffer(S.fixed_file(cb, n, 5, start, end), dtype=np.uint8).reshape(n, start + size + end)
        assert np.array_equal(rec[:, start:start + size], base)
        pad = np.concatenate([rec[:, :start], rec[:, start + size:]], axis=1)
        assert len(np.unique(pad)) > 50   # random bytes, not a constant a decoder could mistake for blanks
        a = S.field_events(O.decode_fixed(cb, rec.tobytes(), record_size=size, start_offset=start, end_offset=end))
        assert a == S.field_events(O.decode_fixed(cb, base.tobytes()))
    # more records than the pool holds: drawn from it
    assert S.payloads(cb, 1500, 5).shape == (1500, size)


@pytest.mark.parametrize("long_every", [0, 5])
def test_rdw_file_lengths(long_every):
    cb = S.parse(S.fuzz_slices()[0])
    n, size = 1089, cb.record_size
    raw, recs = S.rdw_file(cb, n, 9, long_every=long_every)
    off, ln = O.frame_rdw(raw)
    assert len(recs) == n and [raw[o:o + l] for o, l in zip(off, ln)] == recs
    body = S.payloads(cb, n, 9)
    is_long = np.array([long_every > 0 and i % (64 * long_every) == 0 for i in range(n)])
    lens = np.array([len(r) for r in recs])
    for i, r in enumerate(recs):
        assert r[:size] == body[i].tobytes()[:len(r)]
    assert is_long.sum() == (4 if long_every else 0)
    assert ((lens[is_long] >= 300) & (lens[is_long] <= 3000)).all()
    short = lens[~is_long]
    assert short.min() == 1 and short.max() == size
    whole = (short == size).mean()
    assert 0.25 < whole < 0.37             # 30 % whole + the cuts that land on the full length
    assert len(set(short.tolist())) > size * 3 // 4
