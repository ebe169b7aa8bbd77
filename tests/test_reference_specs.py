"""The reference's regression, integration and text specs that hold a copybook, a few literal bytes,
Spark options and the exact expected result (tests/golden/specs, tests/reference_specs.py), replayed on
the CPU: options -> copybook -> the oracle's restatement of the readers, against the answers the
reference itself holds.  This is what checks the oracle (and the option handling the GPU readers share)
where no data-set golden does; tests/test_gpu_reference_specs.py replays the same fixtures on the GPU.
"""
from __future__ import annotations

import json

import pytest

import goldens as G
import reference_specs as RS

from cobrix_amd.reader import FixedLenNestedReader, parse_copybook_for, reader_schema
from cobrix_amd.schema import schema_json
from oracle import reader_oracle as RO

# every fixture, by name: a fixture dropped from (or added to) tests/golden/specs fails test_fixture_set
FIXTURES = [
    "occurs_extractor_string_depending_on",
    "occurs_extractor_string_depending_on_handlers",
    "test01_record_id_sequence_all",
    "test01_record_id_sequence_root_segment",
    "test01_record_id_sequence_segment_filter",
    "test02_header_no_segment_options",
    "test02_header_only_no_segment_options",
    "test02_header_only_segment_filter",
    "test02_header_only_segment_root",
    "test02_header_segment_filter",
    "test02_header_segment_root",
    "test02_no_header_no_segment_options",
    "test02_no_header_segment_filter",
    "test02_no_header_segment_root",
    "test03_ibm_big_endian",
    "test03_ibm_little_endian",
    "test03_ieee754_big_endian",
    "test03_ieee754_little_endian",
    "test04_varchar",
    "test04_varchar_no_trimming",
    "test05_comma_decimals",
    "test05_fixed_length_var_occurs",
    "test05_fixed_length_var_occurs_debug",
    "test06_empty_segment_id",
    "test06_empty_segment_id_and_some_id",
    "test09_primitive_occurs",
    "test09_primitive_occurs_debug",
    "test10_deep_segment_redefines",
    "test12_multi_root_sparse_index",
    "test12_multi_root_sparse_index_short_file",
    "test15_path_with_asterisk",
    "test18_path_special_char",
    "test22_hierarchical_occurs",
    "test23_national_big_endian",
    "test23_national_little_endian",
    "test27_record_length_bigger_than_copybook",
    "test27_record_length_conflict_is_rdw_big_endian",
    "test27_record_length_conflict_is_rdw_part_of_record_length",
    "test27_record_length_conflict_is_record_sequence",
    "test27_record_length_conflict_is_xcom",
    "test27_record_length_conflict_rdw_adjustment",
    "test27_record_length_conflict_record_header_parser",
    "test27_record_length_conflict_record_length_field",
    "test27_record_length_conflict_rhp_additional_info",
    "test27_record_length_not_divisible",
    "test27_record_length_same_as_copybook",
    "test27_record_length_smaller_than_copybook",
    "test2_record_offsets",
    "test4_multisegment_ascii",
    "test4a_multisegment_ascii_iso_8859_1",
    "text02_text_files_old_school",
    "var_size_arrays_fixed_size",
    "var_size_arrays_variable_size",
]

# specs of the same directories that are not replayed, and why
EXCLUDED = {
    "regression/Test07IgnoreHiddenFiles": "lists a directory through Hadoop's FileSystem: no reader is involved",
    "regression/Test08InputFileName": "tests/test_options.py::test_input_file_name_needs_record_sequence covers it",
    "regression/Test11NoCopybookErrMsg": "the message of a load() without a copybook: DefaultSource, not a reader",
    "regression/Test11CustomRDWParser": "a custom record header parser class (option 'record_header_parser': unsupported)",
    "integration/Test12MergeCopybooksSpec": "multiple copybooks (option 'copybooks': unsupported)",
    "integration/Test26CustomRecordExtractor": "a custom record extractor class (option 'record_extractor': unsupported)",
    "integration/Test20InputFileNameSpec": "tests/test_options.py and tests/test_gpu_rdw.py cover the file name column",
    "BinaryNumbersSpec": "random values against scodec: it holds no literal answers",
    "cobol-parser reader/SparseIndexSpecSpec": "IndexGenerator over a TextRecordExtractor: the readers cut no index "
                                               "for text files (VarLenNestedReader.read), the oracle restates none",
}

ROW_KEYS = ("expected", "expected_file", "count", "float_close")


def test_fixture_set():
    assert RS.files() == sorted(n + ".json" for n in FIXTURES)   # and nothing but .json
    assert FIXTURES == sorted(FIXTURES) and len(set(FIXTURES)) == len(FIXTURES)


def test_fixtures_are_well_formed():
    for name in FIXTURES:
        fx = RS.load(name)
        assert fx["spec"].startswith(("SCT/", "CPT/")) and ":" in fx["spec"], name
        assert ("copybook" in fx) != ("copybook_file" in fx), name
        kinds = [k for k in ("error", "parses", "index_entries") + ROW_KEYS if k in fx]
        assert kinds, name
        assert "error" not in kinds or kinds == ["error"], name
        assert ("data_hex" in fx) != ("data" in fx) or kinds[0] in ("error", "parses"), name
        assert all(isinstance(k, str) and isinstance(v, str) for k, v in fx["options"].items()), name
        if fx.get("replicate") and fx["options"].get("generate_record_id") == "true":
            assert fx["records_per_copy"] > 0, name


def host_reader(fx):
    """(copybook, parameters, variable-length?) and, for a fixed-length read, the reader's host checks
    (FixedLenNestedReader.check_binary_data_validity: host logic, run without a device plan)."""
    p, var_len = RS.params(fx)
    cb = parse_copybook_for(RS.copybook_text(fx), p)
    check = None
    if not var_len and not p.is_text:
        rd = object.__new__(FixedLenNestedReader)
        rd.params, rd.copybook = p, cb
        check = rd.check_binary_data_validity
    return cb, p, var_len, check


def replay(fx, copies: int = 1):
    cb, p, var_len, check = host_reader(fx)
    if "data_hex" not in fx and "data" not in fx:   # a parser spec: nothing to read
        return []
    data = RS.data_files(fx, copies)
    for d in data:
        if check is not None:
            check(len(d))
    return RS.oracle_rows(cb, p, var_len, data)


@pytest.mark.parametrize("name", [n for n in FIXTURES if any(k in RS.load(n) for k in ROW_KEYS)])
def test_oracle_rows(name):
    fx = RS.load(name)
    errs = RS.check_rows(fx, replay(fx))
    assert not errs, errs[:10]


@pytest.mark.parametrize("name", [n for n in FIXTURES if RS.load(n).get("replicate")])
def test_oracle_rows_of_repeated_file(name):
    """The rule the GPU tests rely on: a record-independent file repeated gives its rows repeated, each
    copy's Record_Id moved on by the copy's records."""
    fx = RS.load(name)
    rows = replay(fx, RS.COPIES)
    assert len(rows) == len(replay(fx)) * RS.COPIES > 64
    errs = RS.check_rows(fx, rows, RS.COPIES)
    assert not errs, errs[:10]


@pytest.mark.parametrize("name", [n for n in FIXTURES if "index_entries" in RS.load(n)])
def test_oracle_index_entries(name):
    fx = RS.load(name)
    cb, p, var_len, _ = host_reader(fx)
    assert var_len and RO.index_generation_needed(p)
    (data,) = RS.data_files(fx)
    entries = RO.sparse_index(cb, data, p)
    assert len(entries) == fx["index_entries"]
    assert entries[0].offset_from == 0 and entries[-1].offset_to == -1
    assert all(a.offset_to == b.offset_from and a.record_index < b.record_index for a, b in zip(entries, entries[1:]))


def test_multi_root_index_entries():
    """Test12MultiRootSparseIndex: 4 records per entry, cut only at a record of root id 0 or 1 -- the
    entries start at records 0, 5 and 9 of the 3-byte records, with or without the last 2 bytes."""
    for name in ("test12_multi_root_sparse_index", "test12_multi_root_sparse_index_short_file"):
        fx = RS.load(name)
        cb, p, _, _ = host_reader(fx)
        entries = RO.sparse_index(cb, RS.data_files(fx)[0], p)
        assert [(e.offset_from, e.offset_to, e.record_index) for e in entries] == [(0, 15, 0), (15, 27, 5), (27, -1, 9)]


@pytest.mark.parametrize("name", [n for n in FIXTURES if "error" in RS.load(n)])
def test_errors(name):
    fx = RS.load(name)
    with pytest.raises(RS.EXCEPTIONS[fx["error"]["type"]]) as e:
        replay(fx)
    assert e.type is RS.EXCEPTIONS[fx["error"]["type"]]
    assert fx["error"]["contains"] in str(e.value)


@pytest.mark.parametrize("name", [n for n in FIXTURES if "parses" in RS.load(n)])
def test_copybook_parses(name):
    """OccursExtractorSpec.scala:59-73: OCCURS DEPENDING ON a string field, with a handler for every array."""
    fx = RS.load(name)
    cb, p, _, _ = host_reader(fx)
    arrays = {st.name: st for st in cb.ast.children[0].children[1].children if st.is_array}
    assert {k: v.depending_on_handlers for k, v in arrays.items()} == p.occurs_mappings != {}


@pytest.mark.parametrize("name", [n for n in FIXTURES if "schema_file" in RS.load(n)])
def test_schema(name):
    fx = RS.load(name)
    cb, p, var_len, _ = host_reader(fx)
    got = schema_json(reader_schema(cb, p, var_len))
    assert got == json.loads(G.read(*fx["schema_file"].split("/")).decode("latin-1"))


@pytest.mark.parametrize("name", [n for n in FIXTURES if "layout_file" in RS.load(n)])
def test_layout(name):
    """Test18PathSpecialCharSpec: the layout of the copybook parsed with the parser's defaults."""
    from cobrix_amd.copybook import parse_copybook
    fx = RS.load(name)
    cb = parse_copybook(RS.copybook_text(fx))
    assert cb.generate_record_layout_positions() == G.read(*fx["layout_file"].split("/")).decode("latin-1")
