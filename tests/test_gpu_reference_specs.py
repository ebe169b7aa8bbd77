"""The reference's known-answer specs (tests/golden/specs, tests/reference_specs.py) through the HIP
path: rows decoded by libcobrix_hip.so against the answers the reference holds and, row for row, against
the oracle; sparse index entries against the asserted counts and the oracle's entries.

The literal files are 2 to 12 records -- one partial 64-record tile.  A fixture whose rows do not depend
on the file around them (`replicate`) is also read repeated 65 times (more than one tile, at most 780
records) by the same reader: the spec's rows repeated, Record_Id advancing by the copy's records
(tests/test_reference_specs.py::test_oracle_rows_of_repeated_file proves the rule on the oracle).  Not
repeated: the sparse index cases (Test02, Test12), the file-level data sets (Test2, Test4, Test15,
Test18: already several tiles), the text file and the Seg_Id case of Test01 (its ids hold record numbers).

Run on an MI355X: python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread
"""
from __future__ import annotations

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import reference_specs as RS  # noqa: E402
from test_reference_specs import FIXTURES, ROW_KEYS  # noqa: E402

from oracle import reader_oracle as RO  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# (jit, views, lists) as in test_gpu_golden.py::test_gpu_golden_rows: both decode kernels (table-driven:
# jit=-1; copybook-specialised: jit=1), the three string layouts and both OCCURS DEPENDING ON layouts.
# Every reader these fixtures build (fixed-length, RDW, VarOccursRecordExtractor framing, text, hierarchical)
# takes every combination.
COMBOS = [(-1, False, False), (1, False, False), (-1, True, True), (1, True, True), (-1, "utf8", True), (1, "utf8", False)]

ROW_FIXTURES = [n for n in FIXTURES if any(k in RS.load(n) for k in ROW_KEYS)]
# The copybook of test1 (Test2RecordOffsetsSpec, Test15PathWithAsteriskSpec: an OCCURS of 80 groups) takes
# 8-13 s to specialise (hipRTC), per string layout: these two run the table-driven kernel in the three
# layouts; test_gpu_golden_rows[test1], [test1b] run that copybook's specialised kernels.
TABLE_DRIVEN_ONLY = ("test2_record_offsets", "test15_path_with_asterisk")
ROW_PARAMS = [(n, *c) for c in COMBOS for n in ROW_FIXTURES if not (n in TABLE_DRIVEN_ONLY and c[0] == 1)]
INDEX_FIXTURES = [n for n in FIXTURES if "index_entries" in RS.load(n)]


def _reader(fx, jit=-1, views=False, lists=False):
    from cobrix_amd.reader import FixedLenNestedReader, VarLenNestedReader
    p, var_len = RS.params(fx)
    p.jit_min_records, p.string_views, p.string_utf8, p.occurs_lists = jit, views is True, views == "utf8", lists
    var = var_len or p.is_text
    return (VarLenNestedReader if var else FixedLenNestedReader)(RS.copybook_text(fx), p), var


def _read(rd, var, files):
    rows = []
    for file_id, data in enumerate(files):
        rows += (rd.read(data, file_id=file_id) if var else rd.decode(data)).to_rows()
    return rows


@pytest.mark.parametrize("name,jit,views,lists", ROW_PARAMS)
def test_gpu_spec_rows(name, jit, views, lists):
    fx = RS.load(name)
    rd, var = _reader(fx, jit, views, lists)
    p, var_len = RS.params(fx)
    for copies in (1, RS.COPIES) if fx.get("replicate") else (1,):
        files = RS.data_files(fx, copies)
        rows = _read(rd, var, files)
        errs = RS.check_rows(fx, rows, copies)
        assert not errs, (copies, errs[:10])
        exp = RS.oracle_rows(rd.copybook, p, var_len, files)
        assert len(rows) == len(exp), copies
        bad = [i for i, (a, b) in enumerate(zip(rows, exp)) if a != b]
        assert not bad, (copies, bad[:5], rows[bad[0]], exp[bad[0]])


@pytest.mark.parametrize("name", INDEX_FIXTURES)
def test_gpu_spec_index_entries(name):
    """generate_index: the asserted number of entries, each equal to the IndexGenerator restatement's (the
    index is cut before any decode: no kernel or column layout to choose)."""
    fx = RS.load(name)
    rd, var = _reader(fx)
    assert var and rd.index_generation_needed()
    (data,) = RS.data_files(fx)
    t = rd._device_file(data)
    off, ln, _ = rd.frame_file(t, len(data))
    got = [(e.offset_from, e.offset_to, e.record_index) for e in rd.generate_index(t, len(data), off, ln, 0)]
    assert len(got) == fx["index_entries"]
    p, _ = RS.params(fx)
    assert got == [(e.offset_from, e.offset_to, e.record_index) for e in RO.sparse_index(rd.copybook, data, p)]


def test_gpu_spec_record_length_not_divisible():
    """Test27RecordLengthSpec.scala:76-83 on the reader itself: nothing is decoded from such a file."""
    fx = RS.load("test27_record_length_not_divisible")
    rd, var = _reader(fx)
    assert not var
    with pytest.raises(ValueError) as e:
        rd.decode(RS.data_files(fx)[0])
    assert e.type is ValueError and fx["error"]["contains"] in str(e.value)
