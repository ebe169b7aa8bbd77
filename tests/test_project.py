"""Column projection (build_plan(columns=...), the readers' columns=), the parts that need no GPU: the
projected plans' structure, the pruned Spark schema, and the direct projected-decode kernel's per-record
core (cobrix_amd/csrc/cbx_gather.h) run on the host (tests/native/gather_host.cpp) against the oracle.

The contract: a projected read returns, for every record of the unprojected read, the same values for the
requested fields and nothing else; a group appears where a kept primitive lies below it; output stays in
copybook order.  Expected values come from the oracle; `prune_row` below cuts its rows down to a projection
from the copybook AST and the requested names alone (test_gpu_project.py uses the same helper).
"""
from __future__ import annotations

import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from cobrix_amd import copybook as cbk
from cobrix_amd import native as N
from cobrix_amd.plan import build_plan
from cobrix_amd.reader import ReaderParameters, parse_copybook_for, reader_schema
from cobrix_amd.schema import schema_json
from cobrix_amd.synth import (RDW_NARROW_COPYBOOK, SYN200_COPYBOOK, WALK_NESTED_COPYBOOK, WIDE_ODO_COPYBOOK,
                              WIDE_ODO_SEGMENTS, syn200)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------
# The contract over the oracle's rows: from the AST and the requested names alone
# ---------------------------------------------------------------------------------------------
def _prims(st):
    if isinstance(st, cbk.Group):
        for c in st.children:
            yield from _prims(c)
    else:
        yield st


def kept_ids(cb: cbk.Copybook, names):
    """id() of the primitives a request keeps: a named primitive, every primitive below a named group."""
    out = set()
    for nm in names:
        out.update(id(q) for q in _prims(cb.get_field_by_name(nm)))
    return out


def _keeps(st, kept) -> bool:
    return any(id(q) in kept for q in _prims(st))


def _prune_group(g: cbk.Group, d, kept):
    if d is None:
        return None   # an inactive segment redefine stays a null struct
    out = {}
    for c in g.children:
        if c.name not in d or not _keeps(c, kept):
            continue
        v = d[c.name]
        if isinstance(c, cbk.Group) and v is not None:
            v = [_prune_group(c, e, kept) for e in v] if c.is_array else _prune_group(c, v, kept)
        out[c.name] = v
    return out


def prune_row(cb: cbk.Copybook, row: dict, names, collapse_root: bool = True) -> dict:
    """The oracle's row cut down to the projection `names`; generated columns (every key that is not a
    record of the copybook / a child of one) stay."""
    kept = kept_ids(cb, names)
    roots = [g for g in cb.ast.children if isinstance(g, cbk.Group)]
    if collapse_root:
        own = {c.name for g in roots for c in g.children}
        out = {k: v for k, v in row.items() if k not in own}
        for g in roots:
            out.update(_prune_group(g, row, kept))
        return out
    own = {g.name for g in roots}
    out = {k: v for k, v in row.items() if k not in own}
    for g in roots:
        if _keeps(g, kept):
            out[g.name] = _prune_group(g, row[g.name], kept)
    return out


def leaf_names(cb: cbk.Copybook):
    return [q.name for q in _prims(cb.ast) if not q.is_filler]


def test_prune_row_helper():
    cb = cbk.parse_copybook(RDW_NARROW_COPYBOOK, segment_redefines=["STATIC-DETAILS", "CONTACTS"])
    row = {"File_Id": 0, "SEGMENT_ID": "C", "COMPANY_ID": "1", "CONTACTS": None,
           "STATIC_DETAILS": {"COMPANY_NAME": "A", "ADDRESS": "B", "TAXPAYER": {"TAXPAYER_TYPE": "x", "TAXPAYER_STR": "s",
                                                                                  "TAXPAYER_NUM": 5}}}
    assert prune_row(cb, row, ["TAXPAYER-NUM", "PHONE-NUMBER", "COMPANY-ID"]) == {
        "File_Id": 0, "COMPANY_ID": "1", "CONTACTS": None, "STATIC_DETAILS": {"TAXPAYER": {"TAXPAYER_NUM": 5}}}
    assert prune_row(cb, row, []) == {"File_Id": 0}
    assert prune_row(cb, {"COMPANY_DETAILS": row}, ["TAXPAYER"], collapse_root=False) == {
        "COMPANY_DETAILS": {"STATIC_DETAILS": {"TAXPAYER": row["STATIC_DETAILS"]["TAXPAYER"]}}}
    assert prune_row(cb, {"COMPANY_DETAILS": row}, [], collapse_root=False) == {}


# ---------------------------------------------------------------------------------------------
# Plan structure
# ---------------------------------------------------------------------------------------------
def _names(plan, hidden=None):
    return [c.node.name for c in plan.columns if c.kind == "value" and (hidden is None or c.hidden == hidden)]


def _field_tuple(f: N.CbxField):
    return tuple(getattr(f, n) if not hasattr(getattr(f, n), "__len__") else tuple(getattr(f, n)) for n, _ in f._fields_)


def _wide_plan(**kw):
    cb = cbk.parse_copybook(WIDE_ODO_COPYBOOK, segment_redefines=sorted(set(WIDE_ODO_SEGMENTS.values())))
    return build_plan(cb, segment_field="SEGMENT-ID", segment_redefine_map=WIDE_ODO_SEGMENTS, **kw)


def test_syn200_kept_fields_in_copybook_order():
    cb = cbk.parse_copybook(SYN200_COPYBOOK)
    full = build_plan(cb)
    plan = build_plan(cb, columns=["NAME", "AMT-01", "REC-ID"])     # the order of the request does not matter
    assert _names(plan) == ["REC_ID", "AMT_01", "NAME"] and not any(c.hidden for c in plan.columns)
    assert [f.column for f in plan.fields] == [0, 1, 2] and plan.options.n_columns == 3 and not plan.arrays
    for f in plan.fields:   # the descriptors are the full plan's, but for the column index
        node = plan.columns[f.column].node
        g = full.fields[full.field_of_node[id(node)]]
        assert _field_tuple(f)[:-1] == _field_tuple(g)[:-1]
    assert bytes(plan.options.lut) == bytes(full.options.lut)
    assert plan.keeps(cb.get_field_by_name("NAME")) and not plan.keeps(cb.get_field_by_name("BR-ID"))


def test_columns_none_is_todays_plan():
    for text, kw in ((SYN200_COPYBOOK, {}), (SYN200_COPYBOOK, {"generate_record_id": True, "string_views": 1})):
        cb = cbk.parse_copybook(text)
        a, b = build_plan(cb, **kw), build_plan(cb, columns=None, **kw)
        assert [_field_tuple(f) for f in a.fields] == [_field_tuple(f) for f in b.fields]
        assert [(c.kind, c.out_type, c.n_slots, c.hidden) for c in a.columns] == \
               [(c.kind, c.out_type, c.n_slots, c.hidden) for c in b.columns]
        assert bytes(a.options) == bytes(b.options) and b.projected is None
        assert b.options.direct_decode == 0
    a, b = _wide_plan(occurs_lists=True), _wide_plan(occurs_lists=True, columns=None)
    assert [_field_tuple(f) for f in a.fields] == [_field_tuple(f) for f in b.fields]
    assert [bytes(x) for x in a.arrays] == [bytes(x) for x in b.arrays] and bytes(a.options) == bytes(b.options)
    all_cols = build_plan(cbk.parse_copybook(SYN200_COPYBOOK), columns=["SYN200-REC"])   # the record group: every field
    full = build_plan(cbk.parse_copybook(SYN200_COPYBOOK))
    assert _names(all_cols) == _names(full) and len(all_cols.fields) == len(full.fields)


def test_empty_projection_and_bad_names():
    cb = cbk.parse_copybook(SYN200_COPYBOOK)
    plan = build_plan(cb, columns=[])
    assert plan.fields == [] and plan.columns == [] and plan.projected == frozenset()
    gen = build_plan(cb, columns=[], generate_record_id=True)
    assert [c.kind for c in gen.columns] == ["file_id", "record_id"] and len(gen.fields) == 2
    with pytest.raises(ValueError, match="not found"):
        build_plan(cb, columns=["REC-ID", "NO-SUCH-FIELD"])
    dup = cbk.parse_copybook("""
       01  R.
           05  A.
              10  X   PIC X(2).
           05  B.
              10  X   PIC X(2).
    """)
    with pytest.raises(ValueError, match="Multiple fields"):
        build_plan(dup, columns=["X"])
    assert _names(build_plan(dup, columns=["B.X"])) == ["X"]
    assert build_plan(dup, columns=["B.X"]).fields[0].offset == 2
    with pytest.raises(TypeError):
        build_plan(dup, columns="X")


def test_narrow_group_selects_subtree_and_segment_map_stays():
    cb = cbk.parse_copybook(RDW_NARROW_COPYBOOK, segment_redefines=["STATIC-DETAILS", "CONTACTS"])
    kw = dict(segment_field="SEGMENT-ID", segment_redefine_map={"C": "STATIC-DETAILS", "P": "CONTACTS"},
              generate_record_id=True, segment_levels=["C", "P"])
    full = build_plan(cb, **kw)
    plan = build_plan(cb, columns=["TAXPAYER", "PHONE-NUMBER"], **kw)
    assert _names(plan) == ["TAXPAYER_TYPE", "TAXPAYER_STR", "TAXPAYER_NUM", "PHONE_NUMBER"]
    assert [f.segment for f in plan.fields[:4]] == [0, 0, 0, 1]
    assert [g.name for g in plan.segment_groups] == [g.name for g in full.segment_groups]
    # the string segment-id field is matched from the record's bytes: no column needed for it
    a, b = full.options.segments, plan.options.segments
    assert (a.field_offset, a.field_size, a.n_keys, a.n_levels, a.field_is_int) == \
           (b.field_offset, b.field_size, b.n_keys, b.n_levels, b.field_is_int)
    assert bytes(a.key) == bytes(b.key) and list(a.key_segment) == list(b.key_segment)
    assert [c.kind for c in plan.columns[4:]] == ["segment", "file_id", "record_id", "seg_id", "seg_id"]
    assert plan.segment_column == 4 and plan.options.segment_column == 4 and plan.seg_id_columns == [7, 8]
    assert plan.keeps(cb.get_field_by_name("STATIC-DETAILS")) and plan.keeps(cb.get_field_by_name("CONTACTS"))
    assert not plan.keeps(cb.get_field_by_name("COMPANY-ID"))


def test_integral_segment_field_stays_hidden():
    text = """
       01  R.
           05  SEG    PIC 9(2).
           05  A.
              10  X   PIC X(4).
           05  B REDEFINES A.
              10  Y   PIC 9(4).
    """
    cb = cbk.parse_copybook(text, segment_redefines=["A", "B"])
    kw = dict(segment_field="SEG", segment_redefine_map={"1": "A", "2": "B"})
    plan = build_plan(cb, columns=["Y"], **kw)
    assert _names(plan, hidden=True) == ["SEG"] and _names(plan, hidden=False) == ["Y"]
    assert plan.options.segments.field == plan.field_of_node[id(cb.get_field_by_name("SEG"))] == 0
    asked = build_plan(cb, columns=["Y", "SEG"], **kw)
    assert _names(asked, hidden=False) == ["SEG", "Y"] and not _names(asked, hidden=True)


def test_wide_odo_hidden_dependee_and_dropped_array():
    plan = _wide_plan(columns=["NUM2"])
    cb = plan.copybook
    assert _names(plan, hidden=True) == ["NUM_STRAT"] and _names(plan, hidden=False) == ["NUM2"]
    assert len(plan.arrays) == 1 and len(plan.fields) == 2
    ar, f = plan.arrays[0], plan.fields[1]
    assert ar.dependee == 0 and plan.fields[0].column == plan.field_of_node[id(cb.get_field_by_name("NUM-STRAT"))] == 0
    assert plan.columns[ar.count_column].kind == "count" and not plan.columns[ar.count_column].hidden
    assert (f.n_dims, f.dim_array[0], f.dim_count[0], f.dim_stride[0]) == (1, 0, 2000, 8)
    assert plan.columns[f.column].n_slots == 2000 and ar.parent == -1
    # requested: the dependee is an ordinary column
    assert not _names(_wide_plan(columns=["NUM2", "NUM-STRAT"]), hidden=True)
    # no member requested: the array and its count column are gone, and so is its dependee
    plan = _wide_plan(columns=["COMPANY-ID"])
    assert _names(plan) == ["COMPANY_ID"] and not plan.arrays and [c.kind for c in plan.columns] == ["value", "segment"]
    # the list layout over the kept array
    lists = _wide_plan(columns=["NUM1"], occurs_lists=True)
    assert lists.arrays[0].offsets_column >= 0 and lists.fields[1].flags & N.F_LIST
    assert lists.columns[lists.fields[1].column].list_array == 0


def test_array_indices_remapped():
    text = """
       01  R.
           05  N1     PIC 9(1).
           05  N2     PIC 9(1).
           05  A1     OCCURS 0 TO 3 TIMES DEPENDING ON N1.
              10  P   PIC X(2).
           05  A2     OCCURS 0 TO 4 TIMES DEPENDING ON N2.
              10  Q   PIC X(3).
              10  A3  OCCURS 2 TIMES.
                 15  S   PIC 9(2).
    """
    cb = cbk.parse_copybook(text)
    full = build_plan(cb)
    assert len(full.arrays) == 3
    plan = build_plan(cb, columns=["S"])
    assert _names(plan, hidden=True) == ["N2"] and _names(plan, hidden=False) == ["S"]
    assert len(plan.arrays) == 2    # A2 and A3; A1 dropped
    a2, a3 = plan.arrays
    assert (a2.max_count, a2.dependee, a2.parent, a2.n_dims) == (4, 0, -1, 0)
    assert (a3.max_count, a3.dependee, a3.parent, a3.n_dims) == (2, -1, 0, 1)
    s = plan.fields[1]
    assert list(s.dim_array)[:2] == [0, 1] and list(s.dim_count)[:2] == [4, 2] and s.n_dims == 2
    assert [plan.columns[a.count_column].node.name for a in plan.arrays] == ["A2", "A3"]
    assert plan.array_of_node == {id(cb.get_field_by_name("A2")): 0, id(cb.get_field_by_name("A3")): 1}
    only_q = build_plan(cb, columns=["Q"])
    assert len(only_q.arrays) == 1 and only_q.fields[1].dim_array[0] == 0


def test_walk_plan_keeps_every_array_and_dependee():
    cb = cbk.parse_copybook(WALK_NESTED_COPYBOOK)
    full = build_plan(cb, walk=True, variable_size_occurs=True, string_views=1)
    plan = build_plan(cb, walk=True, variable_size_occurs=True, string_views=1, columns=["SEG", "TAIL-TXT"])
    assert _names(plan, hidden=False) == ["SEG", "TAIL_TXT"]
    assert _names(plan, hidden=True) == ["N_OUT", "N_IN"]
    assert len(plan.arrays) == len(full.arrays) == 2
    assert all(plan.columns[a.count_column].hidden for a in plan.arrays)
    assert [plan.columns[a.count_column].n_slots for a in plan.arrays] == [1, 3]
    # the walk's node table is the full one; unrequested primitives carry no field
    assert len(plan.walk.nodes) == len(full.walk.nodes)
    by_name = {}
    for nd, fnd in zip(plan.walk.nodes, full.walk.nodes):
        assert (nd.kind, nd.next, nd.child, nd.array, nd.flags, nd.data_size, nd.actual_size, nd.dep_slot) == \
               (fnd.kind, fnd.next, fnd.child, fnd.array, fnd.flags, fnd.data_size, fnd.actual_size, fnd.dep_slot)
        if fnd.field >= 0:
            by_name[full.columns[full.fields[fnd.field].column].node.name] = nd.field
    assert {k for k, v in by_name.items() if v < 0} == {"KIND", "AMT", "NAME", "TAIL_NUM"}
    assert all(plan.columns[plan.fields[v].column].node.name == k for k, v in by_name.items() if v >= 0)
    # a member requested: its arrays' counts are visible
    inner = build_plan(cb, walk=True, variable_size_occurs=True, string_views=1, columns=["AMT"])
    assert [inner.columns[a.count_column].hidden for a in inner.arrays] == [False, False]


# ---------------------------------------------------------------------------------------------
# The pruned Spark schema
# ---------------------------------------------------------------------------------------------
def _schema_names(fields):
    return [(f.name, _schema_names(f.children) if f.children is not None else None) for f in fields]


@pytest.mark.parametrize("policy", ["collapse_root", "keep_original"])
def test_pruned_spark_schema(policy):
    from cobrix_amd.plan import project_columns
    p = ReaderParameters(is_record_sequence=True, schema_policy=policy, segment_field="SEGMENT-ID",
                         segment_id_redefine_map={"C": "STATIC-DETAILS", "P": "CONTACTS"}, generate_record_id=True,
                         segment_id_levels=["C"])
    cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
    kept = project_columns(cb, ["TAXPAYER-NUM", "COMPANY-ID", "CONTACTS"])
    got = _schema_names(reader_schema(cb, p, True, kept))
    body = [("COMPANY_ID", None), ("STATIC_DETAILS", [("TAXPAYER", [("TAXPAYER_NUM", None)])]),
            ("CONTACTS", [("PHONE_NUMBER", None), ("CONTACT_PERSON", None)])]
    gen = [("File_Id", None), ("Record_Id", None), ("Seg_Id0", None)]
    assert got == gen + (body if policy == "collapse_root" else [("COMPANY_DETAILS", body)])
    full = reader_schema(cb, p, True)
    assert schema_json(reader_schema(cb, p, True, None)) == schema_json(full)
    assert _schema_names(reader_schema(cb, p, True, project_columns(cb, []))) == gen
    js = schema_json(reader_schema(cb, p, True, project_columns(cb, ["TAXPAYER-NUM"])))
    names = [f["name"] for f in js["fields"]]
    assert names == ["File_Id", "Record_Id", "Seg_Id0"] + (["STATIC_DETAILS"] if policy == "collapse_root" else ["COMPANY_DETAILS"])


# ---------------------------------------------------------------------------------------------
# The direct kernel's per-record core on the host
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    so = tmp_path_factory.mktemp("gather_host") / "libcbx_gather_host.so"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-o", str(so), os.path.join(ROOT, "tests", "native", "gather_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_gather.argtypes = [P, i32, P, P, i64, P, P, P, i64, i32, i32, P, P, P, P, P, P, i64, ctypes.c_char_p, i32]
    return lib


class HostBatch:
    """The host core's output in the shape parity.compare_batch reads a batch (plan, n_rec, host_column)."""

    def __init__(self, plan, n_rec, valid, lo, hi, pos, ln, heap):
        self.plan, self.n_rec = plan, n_rec
        self._v, self._lo, self._hi, self._pos, self._ln, self._heap = valid, lo, hi, pos, ln, heap

    def host_column(self, ci):
        plan, n = self.plan, self.n_rec
        fi = next(k for k, f in enumerate(plan.fields) if f.column == ci)
        ot = plan.columns[ci].out_type
        out = {"validity": self._v[fi].astype(bool).reshape(1, n), "values": None}
        lo, hi = self._lo[fi], self._hi[fi]
        if ot in (N.O_STRING, N.O_BINARY):
            out["strings"] = [[self._heap[int(p):int(p) + int(k)] for p, k in zip(self._pos[fi], self._ln[fi])]]
        elif ot in (N.O_I32, N.O_F32):
            out["values"] = (lo & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        elif ot == N.O_DEC128:
            out["values"] = np.stack([lo.view(np.int64), hi.view(np.int64)], axis=1)
        else:
            out["values"] = lo.view(np.int64)
        return out


def host_gather(lib, plan, data: bytes, *, stride: int = 0, rec_off=None, rec_len=None, rec_seg=None, start_off: int = 0):
    """The plan's fields decoded by the host core over fixed-length (stride) or framed records -> HostBatch."""
    nf = len(plan.fields)
    fields = (N.CbxField * max(1, nf))(*plan.fields)
    if rec_off is not None:
        off = np.ascontiguousarray(rec_off, dtype=np.int64)
        ln = np.ascontiguousarray(rec_len, dtype=np.int32)
        n = len(off)
    else:
        off = ln = None
        n = len(data) // stride
    seg = np.ascontiguousarray(rec_seg, dtype=np.int32) if rec_seg is not None else None
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    shape = (max(1, nf), max(1, n))
    valid = np.zeros(shape, np.uint8)
    lo, hi = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64)
    pos, sl = np.zeros(shape, np.int64), np.zeros(shape, np.int32)
    cap = max(64, 3 * sum(f.size for f in plan.fields) * max(1, n))
    heap = np.zeros(cap, np.uint8)
    err = ctypes.create_string_buffer(256)
    rc = lib.cbxh_gather(ctypes.addressof(fields), nf, ctypes.addressof(plan.options.lut), buf.ctypes.data, len(data),
                         off.ctypes.data if off is not None else None, ln.ctypes.data if ln is not None else None,
                         seg.ctypes.data if seg is not None else None, n, stride, start_off, valid.ctypes.data,
                         lo.ctypes.data, hi.ctypes.data, pos.ctypes.data, sl.ctypes.data, heap.ctypes.data, cap, err, 256)
    assert rc == 0, (rc, err.value.decode())
    return HostBatch(plan, n, valid[:, :n], lo[:, :n], hi[:, :n], pos[:, :n], sl[:, :n], heap.tobytes())


SUBSETS = 40


def projections(names, seed: int):
    """Every field alone, then SUBSETS seeded random subsets (2 .. all of the fields)."""
    rng = random.Random(seed)
    out = [[nm] for nm in names]
    for _ in range(SUBSETS):
        out.append(rng.sample(names, rng.randint(2, len(names))))
    return out


def check_projections(lib, cb, res, names, seed, plan_kw, **gather_kw):
    """Every projection of `projections`: the host core over the projected plan equals the oracle's decode
    (res) bit for bit -- values, validity, string bytes -- on the plan's visible columns."""
    from parity import compare_batch
    checked = 0
    for cols in projections(names, seed):
        plan = build_plan(cb, columns=cols, string_views=1, **plan_kw)
        assert sorted(c.node.name for c in plan.columns if c.kind == "value" and not c.hidden) == \
               sorted(cb.get_field_by_name(nm).name for nm in cols)
        errs = compare_batch(host_gather(lib, plan, **gather_kw), res)
        assert not errs, (cols, errs[:3])
        checked += 1
    assert checked == len(names) + SUBSETS
    return checked


def test_host_core_syn200(host_shim):
    """2,000 SYN200 records, a fifth of the numeric fields malformed; with a 3-byte start offset too (every
    SWAR load at another alignment; the first record's fields have fewer than 16 bytes in front)."""
    from oracle import oracle as O
    cb = parse_copybook_for(SYN200_COPYBOOK, ReaderParameters())
    data = syn200(2000, seed=5, malformed_rate=0.2).numpy().tobytes()
    res = O.decode_fixed(cb, data)
    check_projections(host_shim, cb, res, leaf_names(cb), 41, {}, data=data, stride=200)
    rng = np.random.default_rng(3)
    recs = np.frombuffer(data, np.uint8).reshape(-1, 200)[:300]
    padded = np.concatenate([rng.integers(0, 256, (300, 3), dtype=np.uint8), recs,
                             rng.integers(0, 256, (300, 2), dtype=np.uint8)], axis=1).tobytes()
    res2 = O.decode_fixed(cb, padded, start_offset=3, end_offset=2)
    from parity import compare_batch
    plan = build_plan(cb, columns=leaf_names(cb), string_views=1)
    assert not compare_batch(host_gather(host_shim, plan, padded, stride=205, start_off=3), res2)


@pytest.mark.parametrize("code_page,trim", [("cp037", "both"), ("common", "none"), ("cp875", "left")])
def test_host_core_fuzz_copybook(host_shim, code_page, trim):
    """FUZZ_COPYBOOK: every zoned / binary / COMP-3 shape of the decode fuzz, strings, COMP-1 / COMP-2."""
    from oracle import oracle as O
    from test_decode_fuzz import FUZZ_COPYBOOK
    from test_filter import fuzz_records
    p = ReaderParameters(ebcdic_code_page=code_page, string_trimming_policy=trim)
    cb = parse_copybook_for(FUZZ_COPYBOOK, p)
    data = fuzz_records(cb, 321, 31)
    res = O.decode_fixed(cb, data)
    assert check_projections(host_shim, cb, res, leaf_names(cb), 42, {}, data=data, stride=cb.record_size) > 60


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_host_core_ascii_copybook(host_shim, charset):
    """ASCII_COPYBOOK: every CBX_K_ASCII_NUM shape, an ASCII string (ascii_lut, or the charset's table), PIC N
    (UTF-16) fields."""
    from oracle import oracle as O
    from test_decode_fuzz import ASCII_COPYBOOK
    from test_filter import ascii_records
    p = ReaderParameters(is_ebcdic=False, ascii_charset=charset)
    cb = parse_copybook_for(ASCII_COPYBOOK, p)
    data = ascii_records(cb, 321, 32)
    res = O.decode_fixed(cb, data)
    plan = build_plan(cb, string_views=1)
    assert {N.K_ASCII_NUM, N.K_UTF16_BE} <= {f.kind for f in plan.fields} or \
           {N.K_ASCII_NUM, N.K_UTF16_LE} <= {f.kind for f in plan.fields}
    check_projections(host_shim, cb, res, leaf_names(cb), 43, {}, data=data, stride=cb.record_size)


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_core_records_cut_at_every_length(host_shim, trim):
    """One ladder record per length 1..L (strings of 1-47 bytes, COMP-3 and zoned of every width): every
    field cut inside at every byte and in front of its first byte -- a cut numeric is null, a cut string the
    truncated value, a string that starts past the end null.  Framed records at their file offsets (the RDW
    headers between them are the bytes in front of each record)."""
    from oracle import oracle as O
    from test_filter import LADDER_COPYBOOK, ladder_file, ladder_params
    p = ladder_params(trim)
    cb = parse_copybook_for(LADDER_COPYBOOK, p)
    raw, off, ln = ladder_file(seed=34, every_length=True)
    assert ln.tolist() == list(range(1, cb.record_size + 1))
    res = O.decode_var(cb, raw, off, ln)
    check_projections(host_shim, cb, res, leaf_names(cb), 44, {}, data=raw, rec_off=off, rec_len=ln)


def test_host_core_segment_redefines(host_shim):
    """RDW_NARROW with its redefine map: a field of a redefine that is not the record's is null."""
    from oracle import oracle as O
    from oracle import reader_oracle as RO
    from test_filter import narrow_file, narrow_params
    p = narrow_params()
    cb = parse_copybook_for(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(300, 21)
    off, ln = O.frame_rdw(raw)
    recs = RO.var_len_records(cb, raw, p)
    kw = dict(segment_field=p.segment_field, segment_redefine_map=p.segment_id_redefine_map)
    groups = [g.name.upper() for g in build_plan(cb, **kw).segment_groups]
    seg = np.array([groups.index(r.active_segment.upper()) if r.active_segment is not None else -1 for r in recs], np.int32)
    assert {-1, 0, 1} == set(seg.tolist())
    res = O.decode_var(cb, raw, off, ln, active_segments=[r.active_segment for r in recs])
    check_projections(host_shim, cb, res, leaf_names(cb), 45, kw, data=raw, rec_off=off, rec_len=ln, rec_seg=seg)


def test_host_core_refuses_occurs(host_shim):
    plan = _wide_plan(columns=["NUM2"], string_views=1)
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    err = ctypes.create_string_buffer(256)
    z = np.zeros(16, np.uint64)
    rc = host_shim.cbxh_gather(ctypes.addressof(fields), len(plan.fields), ctypes.addressof(plan.options.lut), z.ctypes.data,
                               0, None, None, None, 0, 8, 0, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                               z.ctypes.data, z.ctypes.data, 0, err, 256)
    assert rc == N.CBX_E_UNSUPPORTED and "OCCURS" in err.value.decode()
