"""Column projection on the GPU (readers built with columns=...) against the contract: for every record of
the unprojected ORACLE read (after filters, in file order) the same values for the requested fields and
nothing else.  Expected rows are the oracle's, cut down by test_project.prune_row (copybook AST + requested
names only); bit-level values by parity.compare_batch over the batch's own visible columns.

Where both kernels can run a plan, every case runs with direct_decode=False (the staged kernels) and
direct_decode=True (the direct kernel, cbx_gather.h), and asserts which kernel ran against `predict_kind`
-- the eligibility rules written out here, not read from the library.
"""
from __future__ import annotations

import ctypes
import dataclasses
import random
from decimal import Decimal

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader  # noqa: E402
from cobrix_amd.synth import (RDW_NARROW_COPYBOOK, SYN200_COPYBOOK, WALK_NESTED_COPYBOOK, WIDE_ODO_COPYBOOK,  # noqa: E402
                              WIDE_ODO_SEGMENTS, rdw_file, syn200, walk_nested_record, wide_odo)
from oracle import oracle as O  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from parity import compare_batch  # noqa: E402
from test_filter import LADDER_COPYBOOK, ladder_file, ladder_params, narrow_file, narrow_params, py_keep  # noqa: E402
from test_project import leaf_names, prune_row  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def kernel_kind(rd) -> int:
    k = ctypes.c_int32(-1)
    N.check(N.load().cbx_plan_kernel_kind(rd.out_native.handle, ctypes.byref(k)))
    return k.value


def eligible(rd):
    """(eligible, reason) as cbx_plan_direct_eligible reports it for the reader's decode plan."""
    e = ctypes.c_int32(-1)
    L = N.load()
    N.check(L.cbx_plan_direct_eligible(rd.out_native.handle, ctypes.byref(e)))
    return e.value, L.cbx_last_error().decode()


def predict_eligible(rd, peer: bool = False) -> bool:
    """The direct kernel's eligibility rules: no record walk, no OCCURS (every field n_dims == 0, no array),
    no list layout, no Seg_Id level columns, string columns absent or in the view layout, no pipeline peer."""
    plan = rd.out_plan
    strings = any(c.out_type in (N.O_STRING, N.O_BINARY) for c in plan.columns)
    return (not rd.walk and not plan.arrays and all(f.n_dims == 0 and not (f.flags & N.F_LIST) for f in plan.fields)
            and not plan.seg_id_columns and (not strings or plan.options.string_views == 1) and not peer)


def predict_kind(rd, n_rec: int, staged_kind: int = 0, peer: bool = False) -> int:
    """4 when the reader asked for the direct kernel and its plan is eligible; else what the staged path runs
    (staged_kind: 0 table-driven, 1 specialised, 2 / 3 the record walk).  A call of no record launches
    nothing: the staged path leaves the plan's initial 0."""
    if rd.out_plan.options.direct_decode == 1 and predict_eligible(rd, peer):
        return 4
    return staged_kind if n_rec > 0 else 0


LAYOUTS = {"large": {}, "views": {"string_views": True}, "utf8": {"string_utf8": True}}


def _device(data: bytes):
    return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()


def _for(res, rd):
    """The shared oracle decode as a result over the reader's own parse of the same copybook (the oracle's
    node table is keyed by the copybook object; node numbers are the copybook's DFS order)."""
    return O.OracleResult(O.OracleAst(rd.copybook), res.events, res.heap, res.n_rec)


def _same_rows(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if a != b]
    assert not bad, (what, bad[:5], got[bad[0]], exp[bad[0]])


# ---------------------------------------------------------------------------------------------
# 1. SYN200, tile edges
# ---------------------------------------------------------------------------------------------
SYN_N = 4097
SYN_P = ReaderParameters(schema_policy="collapse_root", jit_min_records=-1)
SINGLES = ["REC-ID", "BR-ID", "ACCT-NO", "AMT-01", "RATE-01", "QTY-01", "ZN-01", "ZD-01", "FX-RATE", "NAME"]
THREE = ["REC-ID", "AMT-01", "NAME"]


@pytest.fixture(scope="module")
def syn():
    """(copybook, records [SYN_N, 200], oracle rows, oracle decode per n) -- computed once, shared, unchanged."""
    from cobrix_amd.reader import parse_copybook_for
    cb = parse_copybook_for(SYN200_COPYBOOK, SYN_P)
    recs = syn200(SYN_N, seed=11, malformed_rate=0.2)
    data = recs.numpy().tobytes()
    rows = RO.fixed_len_rows(cb, data, SYN_P)
    res = {n: O.decode_fixed(cb, data[:n * 200]) for n in (0, 1, 63, 64, 65, 67, 257, SYN_N)}
    return cb, recs, rows, res


def _syn_projections(cb):
    return [[nm] for nm in SINGLES] + [THREE, [], leaf_names(cb)]


def _syn_modes():
    """(layout, direct_decode): the staged kernels in all three string layouts, the direct kernel asked for in
    all three too (it takes the view layout; with a string column in another layout it must fall back)."""
    return [(lay, d) for d in (False, True) for lay in LAYOUTS]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, SYN_N])
def test_syn200_tile_edges(syn, n):
    cb, recs, rows, res = syn
    data = recs[:n].numpy().tobytes()
    t = _device(data)
    ran = set()
    for cols in _syn_projections(cb):
        exp_rows = [prune_row(cb, r, cols) for r in rows[:n]] if (n <= 65 or cols == THREE) else None
        for layout, direct in _syn_modes():
            if direct and layout != "views" and "NAME" not in cols and cols != leaf_names(cb):
                continue   # no string column: the layouts do not differ
            rd = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, direct_decode=direct, **LAYOUTS[layout]),
                                      columns=cols)
            b = rd.decode_device(t, len(data))
            assert b.n_rec == n
            what = (cols if len(cols) < 5 else "all", layout, direct, n)
            if cols:
                kind = kernel_kind(rd)
                assert kind == predict_kind(rd, n), (what, kind)
                has_str = "NAME" in cols or len(cols) > 5
                assert (kind == 4) == (direct and (layout == "views" or not has_str)), what
                ran.add(kind)
            else:
                assert rd.out_native is None and b.cols == []
            errs = compare_batch(b, _for(res[n], rd)) if n else []   # (no record: the rows below are the check)
            assert not errs, (what, errs[:3])
            assert sorted(c.node.name for c in b.plan.columns if c.kind == "value") == \
                   sorted(cb.get_field_by_name(nm).name for nm in cols)
            if exp_rows is not None:
                _same_rows(b.to_rows(), exp_rows, what)
            rd.close()
    assert ran == {0, 4}


def test_syn200_column_buffers_hold_the_projection_only(syn):
    cb, recs, rows, res = syn
    t = recs.cuda().reshape(-1)
    sizes = {}
    for cols in (None, THREE):
        rd = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, string_views=True), columns=cols)
        b = rd.decode_device(t, SYN_N * 200)
        sizes[cols is None] = sum(v.numel() * v.element_size() for c in b.cols for v in c.values() if torch.is_tensor(v))
        assert len(b.cols) == (len(rd.plan.columns) if cols is None else 3)
        assert rd.plan is (rd.out_plan if cols is None else rd.plan) and (cols is None) == (rd.out_plan is rd.plan)
        rd.close()
    assert sizes[False] * 2 < sizes[True]


# ---------------------------------------------------------------------------------------------
# 2. Data pointer edges (direct)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [9, 0])
def test_direct_data_pointer_edges(syn, shift):
    """67 records at +9 bytes inside a larger buffer (every SWAR load unaligned), and in a buffer that starts
    at record 0 (nothing readable in front: the first record's leading fields take the byte loop)."""
    cb, recs, rows, res = syn
    t = torch.zeros(200 * 67 + shift, dtype=torch.uint8, device="cuda")
    t[shift:] = recs[:67].reshape(-1).cuda()
    for cols in (THREE, leaf_names(cb), ["BR-ID"], ["AMT-01", "ZN-01"]):
        rd = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, direct_decode=True, string_views=True),
                                  columns=cols)
        b = rd.decode_device(t[shift:], 200 * 67, first_record_id=5)
        assert kernel_kind(rd) == predict_kind(rd, 67) == 4
        errs = compare_batch(b, _for(res[67], rd))
        assert not errs, (cols, errs[:3])
        rd.close()


# ---------------------------------------------------------------------------------------------
# 3. RDW multisegment, short records
# ---------------------------------------------------------------------------------------------
NARROW_COLS = ["COMPANY-ID", "COMPANY-NAME", "PHONE-NUMBER", "TAXPAYER-NUM"]


@pytest.fixture(scope="module")
def narrow():
    raw = narrow_file(1000, 9)
    p = dataclasses.replace(narrow_params(), generate_record_id=True, jit_min_records=-1, string_views=True)
    from cobrix_amd.reader import parse_copybook_for
    cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == 1000
    return raw, p, cb, rows


@pytest.mark.parametrize("direct", [False, True])
def test_rdw_multisegment_projection(narrow, direct):
    raw, p, cb, rows = narrow
    exp = [prune_row(cb, r, NARROW_COLS) for r in rows]
    assert any(r["STATIC_DETAILS"] is None for r in exp) and any(r["CONTACTS"] is None for r in exp)
    assert any(r["STATIC_DETAILS"] is None and r["CONTACTS"] is None for r in exp)     # an id outside the map
    assert all(set(r) == {"File_Id", "Record_Id", "COMPANY_ID", "STATIC_DETAILS", "CONTACTS"} for r in exp)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, dataclasses.replace(p, direct_decode=direct), columns=NARROW_COLS)
    # through the selection (read: frame -> index -> select -> decode_selected) and as framed records (decode)
    for call in (lambda: rd.read(raw), lambda: rd.decode(raw)):
        b = call()
        assert kernel_kind(rd) == predict_kind(rd, 1000) == (4 if direct else 0)
        got = b.to_rows()
        _same_rows(got, exp, direct)
        assert [g["Record_Id"] for g in got] == [r["Record_Id"] for r in rows]     # generate_record_id ids unchanged
    # per sparse-index entry
    t = rd._device_file(raw)
    off, ln, vb = rd.frame_file(t, len(raw))
    ents = rd.generate_index(t, len(raw), off, ln, 0)
    _same_rows([r for b in rd.read_entries(t, len(raw), ents, 1) for r in b.to_rows()], exp, "entries")
    # the pruned schema
    names = [f.name for f in rd.spark_schema()]
    assert names == ["File_Id", "Record_Id", "COMPANY_ID", "STATIC_DETAILS", "CONTACTS"]
    rd.close()


def test_seg_id_levels_fall_back(narrow):
    raw, p, cb, rows = narrow
    p2 = dataclasses.replace(p, segment_id_levels=["C", "P"], direct_decode=True)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p2, columns=NARROW_COLS)
    exp = [prune_row(rd.copybook, r, NARROW_COLS) for r in RO.var_len_rows(rd.copybook, raw, p2)]
    assert {"Seg_Id0", "Seg_Id1"} <= set(exp[0])
    b = rd.read(raw)
    assert not predict_eligible(rd) and kernel_kind(rd) == predict_kind(rd, len(exp)) == 0
    ok, why = eligible(rd)
    assert ok == 0 and "Seg_Id" in why
    _same_rows(b.to_rows(), exp, "levels")
    rd.close()


LADDER_COLS = ["X01", "P05", "Z09", "X12", "X17", "P16", "Z16", "X33", "P47", "X47", "Z40"]


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("trim", ["none", "both"])
def test_short_records_cut_strings_and_null_numerics(trim, direct):
    """The width ladder on RDW records cut at random lengths and one record per length 1..L: a numeric the
    record ends inside is null, a string that starts inside it is the truncated value, one past it null."""
    for every in (False, True):
        raw, off, ln = ladder_file(seed=34 if every else 33, every_length=every)
        p = dataclasses.replace(ladder_params(trim), jit_min_records=-1, string_views=True, direct_decode=direct)
        rd = VarLenNestedReader(LADDER_COPYBOOK, p, columns=LADDER_COLS)
        exp = [prune_row(rd.copybook, r, LADDER_COLS) for r in RO.var_len_rows(rd.copybook, raw, p)]
        assert any(r["P47"] is None for r in exp) and any(r["X47"] is None for r in exp)
        for call in (lambda: rd.read(raw), lambda: rd.decode(raw)):
            b = call()
            assert kernel_kind(rd) == predict_kind(rd, len(exp)) == (4 if direct else 0)
            errs = compare_batch(b, O.decode_var(rd.copybook, raw, off, ln))
            assert not errs, (trim, direct, every, errs[:3])
            _same_rows(b.to_rows(), exp, (trim, direct, every))
        rd.close()


# ---------------------------------------------------------------------------------------------
# 4. Filter + projection
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [False, True])
def test_filter_on_a_field_that_is_not_projected(syn, narrow, direct):
    cb, recs, rows, res = syn
    f = [F.GreaterThan("AMT-01", Decimal("1234567.89"))]
    cols = ["NAME", "REC-ID"]
    exp = [prune_row(cb, r, cols) for r in rows if py_keep(cb, r, f)]
    assert 0 < len(exp) < SYN_N
    rd = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, string_views=True, direct_decode=direct), columns=cols)
    b = rd.decode_device(recs.cuda().reshape(-1), SYN_N * 200, filters=f)
    assert b.unhandled_filters == [] and kernel_kind(rd) == predict_kind(rd, len(exp)) == (4 if direct else 0)
    assert [c.node.name for c in b.plan.columns] == ["REC_ID", "NAME"]      # the filter's field is not written
    _same_rows(b.to_rows(), exp, direct)
    rd.close()
    raw, p, ncb, nrows = narrow
    f = [F.EqualTo("SEGMENT-ID", "C")]
    cols = ["COMPANY-NAME", "TAXPAYER-NUM"]
    exp = [prune_row(ncb, r, cols) for r in nrows if py_keep(ncb, r, f)]
    assert 0 < len(exp) < len(nrows)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, dataclasses.replace(p, direct_decode=direct), columns=cols)
    b = rd.read(raw, filters=f)
    assert b.unhandled_filters == [] and kernel_kind(rd) == (4 if direct else 0)
    _same_rows(b.to_rows(), exp, direct)
    rd.close()


# ---------------------------------------------------------------------------------------------
# 5. OCCURS
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    raw_t, hdr = wide_odo(70, seed=5)
    raw = raw_t.numpy().tobytes()
    eo, el = O.frame_rdw(raw)
    segs = [{0xC3: "STATIC_DETAILS", 0xD7: "CONTACTS"}.get(raw[o]) for o in eo]
    from cobrix_amd.reader import parse_copybook_for
    p = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID", segment_id_redefine_map=WIDE_ODO_SEGMENTS,
                         jit_min_records=-1, direct_decode=True)
    cb = parse_copybook_for(WIDE_ODO_COPYBOOK, p)
    res = O.decode_records(cb, [raw[o:o + l] for o, l in zip(eo, el)], active_segments=segs)
    return raw_t, raw, p, res


@pytest.mark.parametrize("lists", [False, True])
def test_occurs_counts_from_the_hidden_dependee(wide, lists):
    raw_t, raw, p, res = wide
    rd = VarLenNestedReader(WIDE_ODO_COPYBOOK, dataclasses.replace(p, occurs_lists=lists), columns=["NUM2"])
    plan = rd.out_plan
    assert [c.node.name for c in plan.columns if c.kind == "value" and c.hidden] == ["NUM_STRAT"]
    assert bool(plan.fields[1].flags & N.F_LIST) == lists
    t = raw_t.cuda()
    off, ln = rd.frame(t, len(raw))
    b = rd.decode_device(t, len(raw), off, ln)
    assert not predict_eligible(rd) and kernel_kind(rd) == predict_kind(rd, b.n_rec) == 0
    ok, why = eligible(rd)
    assert ok == 0 and "OCCURS" in why
    errs = compare_batch(b, _for(res, rd))
    assert not errs, errs[:3]
    rows = b.to_rows()
    assert any(r["COMPANY_DETAILS"]["STATIC_DETAILS"] is None for r in rows)     # the 'P' records: a null struct
    row = next(r for r in rows if r["COMPANY_DETAILS"]["STATIC_DETAILS"] is not None)
    assert set(row["COMPANY_DETAILS"]) == {"STATIC_DETAILS"}       # nothing of CONTACTS is requested
    assert set(row["COMPANY_DETAILS"]["STATIC_DETAILS"]) == {"STRATEGY"}
    assert all(set(e) == {"NUM2"} for e in row["COMPANY_DETAILS"]["STATIC_DETAILS"]["STRATEGY"]["STRATEGY_DETAIL"])
    rd.close()


def test_occurs_array_dropped(wide):
    raw_t, raw, p, res = wide
    rd = VarLenNestedReader(WIDE_ODO_COPYBOOK, p, columns=["COMPANY-ID"])
    assert not rd.out_plan.arrays and len(rd.out_plan.fields) == 1 and rd.plan.arrays
    t = raw_t.cuda()
    off, ln = rd.frame(t, len(raw))
    b = rd.decode_device(t, len(raw), off, ln)
    # nothing of the array is left, but COMPANY-ID is a string in the large-string layout: the staged kernels
    assert not predict_eligible(rd) and kernel_kind(rd) == predict_kind(rd, b.n_rec) == 0
    ok, why = eligible(rd)
    assert ok == 0 and "view" in why
    errs = compare_batch(b, _for(res, rd))
    assert not errs, errs[:3]
    assert all(set(r["COMPANY_DETAILS"]) == {"COMPANY_ID"} for r in b.to_rows()[:50])
    rd.close()


# ---------------------------------------------------------------------------------------------
# 6. Record walk
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [["SEG", "TAIL-TXT", "KIND"], ["AMT", "TAIL-NUM"], ["INNER"], []])
def test_record_walk_projection(cols):
    """variable_size_occurs: every array moves the offsets behind it, so the walk keeps the arrays and their
    DEPENDING ON sources (N-OUT, N-IN hidden) whatever is requested."""
    rnd = random.Random(6)
    raw = rdw_file([walk_nested_record(rnd, True) for _ in range(300)])
    p = ReaderParameters(is_record_sequence=True, variable_size_occurs=True, generate_record_id=True,
                         schema_policy="collapse_root", jit_min_records=-1, direct_decode=True)
    rd = VarLenNestedReader(WALK_NESTED_COPYBOOK, p, columns=cols)
    assert rd.walk and not predict_eligible(rd)
    b = rd.read(raw, file_id=1)
    assert kernel_kind(rd) == predict_kind(rd, 300, staged_kind=2) == 2
    ok, why = eligible(rd)
    assert ok == 0 and "walk" in why
    exp = [prune_row(rd.copybook, r, cols) for r in RO.var_len_rows(rd.copybook, raw, p, file_id=1)]
    _same_rows(b.to_rows(), exp, cols)
    rd.close()


# ---------------------------------------------------------------------------------------------
# 7. Specialised kernel, 8. Utf8 pipeline
# ---------------------------------------------------------------------------------------------
def test_specialised_kernel_on_a_projected_plan(syn):
    cb, recs, rows, res = syn
    rd = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, jit_min_records=64, direct_decode=False),
                              columns=THREE)
    b = rd.decode_device(recs.cuda().reshape(-1), SYN_N * 200)
    assert kernel_kind(rd) == predict_kind(rd, SYN_N, staged_kind=1) == 1
    errs = compare_batch(b, _for(res[SYN_N], rd))
    assert not errs, errs[:3]
    _same_rows(b.to_rows(), [prune_row(cb, r, THREE) for r in rows], "jit")
    rd.close()


@pytest.mark.parametrize("direct", [False, True])
def test_utf8_pipeline_projection(syn, direct):
    cb, recs, rows, res = syn
    cols = ["REC-ID", "NAME"]
    rd = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, string_utf8=True, direct_decode=direct), columns=cols)
    batches = rd.decode_batches(recs[:300].cuda().reshape(-1), 300 * 200, 100, first_record_id=10)
    assert [b.n_rec for b in batches] == [100, 100, 100] and rd._peer is not None and rd._peer.columns == cols
    assert kernel_kind(rd) == predict_kind(rd, 100, peer=True) == 0       # Utf8 strings, a pipeline peer: staged
    assert all("offsets32" in b.cols[1] and len(b.cols) == 2 for b in batches)
    got = [r for b in batches for r in b.to_rows()]
    _same_rows(got, [prune_row(cb, r, cols) for r in rows[:300]], direct)
    rd.close()


# ---------------------------------------------------------------------------------------------
# 9. Hierarchical refusal, 10. Arrow, 11. eligibility reasons
# ---------------------------------------------------------------------------------------------
def test_hierarchical_read_with_columns_raises():
    from test_gpu_hier import _reader, hier_stream
    full, p = _reader()
    rd = VarLenNestedReader(full.copybook_contents, p, columns=["SEGMENT-ID"])
    assert rd.hierarchical
    with pytest.raises(N.CbxError) as e:
        rd.read(hier_stream(50, 1, 1.0))
    assert e.value.code == N.CBX_E_UNSUPPORTED and "columns" in str(e.value)
    rd.close()
    full.close()


@pytest.mark.parametrize("policy", ["collapse_root", "keep_original"])
@pytest.mark.parametrize("direct", [False, True])
def test_arrow_of_a_projected_batch(narrow, direct, policy):
    pytest.importorskip("pyarrow")
    from test_gpu_golden import _norm
    raw, p, cb, rows = narrow
    p2 = dataclasses.replace(p, direct_decode=direct, schema_policy=policy)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p2, columns=NARROW_COLS)
    exp = [prune_row(rd.copybook, r, NARROW_COLS, policy == "collapse_root") for r in RO.var_len_rows(rd.copybook, raw, p2)]
    table = rd.read(raw).to_arrow()
    table.validate(full=True)
    assert table.column_names == list(exp[0]) == [f.name for f in rd.spark_schema()]
    assert _norm(table.to_pylist()) == _norm(exp)
    rd.close()
    # no column at all: the row count and the generated columns
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p2, columns=[])
    b = rd.read(raw)
    assert b.n_rec == len(rows) and b.to_arrow().column_names == ["File_Id", "Record_Id"]
    _same_rows(b.to_rows(), [{"File_Id": r["File_Id"], "Record_Id": r["Record_Id"]} for r in rows], "empty")
    rd.close()


def test_eligibility_reasons(syn):
    """cbx_plan_direct_eligible: the reason for each ineligible shape (OCCURS, Seg_Id levels and the record
    walk are asserted beside their cases above)."""
    cb, recs, rows, res = syn
    for layout, word in (("large", "view"), ("utf8", "view")):
        rd = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, direct_decode=True, **LAYOUTS[layout]), columns=THREE)
        ok, why = eligible(rd)
        assert ok == 0 and word in why and not predict_eligible(rd), (layout, why)
        rd.close()
    rd = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, direct_decode=True, string_views=True), columns=THREE)
    assert eligible(rd)[0] == 1 and predict_eligible(rd)
    other = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, string_views=True), columns=THREE)
    N.check(N.load().cbx_plan_pipeline(rd.out_native.handle, other.out_native.handle, 0, 0))
    ok, why = eligible(rd)
    assert ok == 0 and "peer" in why
    N.check(N.load().cbx_plan_pipeline(rd.out_native.handle, None, 0, 0))
    assert eligible(rd)[0] == 1
    # the option is the projected plan's only; a reader without a projection never sets it
    plain = FixedLenNestedReader(SYN200_COPYBOOK, dataclasses.replace(SYN_P, direct_decode=True, string_views=True))
    assert plain.plan.options.direct_decode == 0 and plain.out_plan is plain.plan
    assert rd.plan.options.direct_decode == 0 and rd.out_plan.options.direct_decode == 1
    for r in (rd, other, plain):
        r.close()


def test_direct_profiling_record_base_and_default_rule(syn):
    """The profiling events wrap the direct kernel as they do the decode kernel (no post passes: post_ms 0);
    Record_Id honours first_record_id plus the device base of cbx_plan_set_record_base; File_Id is the call's.
    With direct_decode left at None the reader applies its measured rule: never (the kernel is opt-in)."""
    from cobrix_amd import reader as R
    cb, recs, rows, res = syn
    p = ReaderParameters(jit_min_records=-1, string_views=True, generate_record_id=True, direct_decode=True)
    rd = VarLenNestedReader(SYN200_COPYBOOK, p, columns=["BR-ID"])
    L = N.load()
    h = rd.out_native.handle
    t = recs[:130].cuda().reshape(-1)
    off, ln = rd.frame_fixed(t, 130 * 200)
    base = torch.tensor([1000], dtype=torch.int64, device="cuda")
    N.check(L.cbx_plan_set_profiling(h, 1))
    N.check(L.cbx_plan_set_record_base(h, base.data_ptr()))
    b = rd.decode_device(t, 130 * 200, off, ln, first_record_id=7)
    N.check(L.cbx_plan_set_record_base(h, None))
    assert kernel_kind(rd) == predict_kind(rd, 130) == 4
    dec, post = (ctypes.c_float * 4)(), (ctypes.c_float * 4)()
    n = ctypes.c_int32(0)
    N.check(L.cbx_plan_kernel_times(h, dec, post, 4, ctypes.byref(n)))
    assert n.value == 1 and dec[0] > 0 and post[0] == 0
    got = b.to_rows()
    assert [r["Record_Id"] for r in got] == [1007 + i for i in range(130)] and {r["File_Id"] for r in got} == {0}
    assert [r["SYN200_REC"]["BR_ID"] for r in got] == [r["BR_ID"] for r in rows[:130]]
    rd.close()
    assert R.DIRECT_MAX_SHARE is None
    rd = FixedLenNestedReader(SYN200_COPYBOOK, ReaderParameters(string_views=True), columns=["BR-ID"])
    assert rd.out_plan.options.direct_decode == 0 and R.projection_share(rd.copybook, rd.out_plan.projected) == 2 / 200   # PIC S9(4) COMP of 200 bytes
    rd.close()
