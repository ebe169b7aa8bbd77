"""Fan-out joins (cbx_key_map_index_rows, cbx_join_records_expand and their info calls), the parts that need no GPU: the
two new ABI structs' layout, the symbols, every refusal with its message, and the host/device part of
cobrix_amd/csrc/cbx_keymap_rows.h (the scatter's placement rule with its bound check, the cursor check, the sorting
network, the wave-first search, the in-window locate, the output-row rule) run on the host
(tests/native/fanout_host.cpp) against a Python model.

The model takes the oracle's rows only: `map_model` (test_keymap.py) for the member set, `expected_rows` for
{key: [ordinals ascending]} and `expected_expand` for (fact index per output row, match per output row).  It never
uses the code under test.  The GPU tests (test_gpu_fanout.py) use the same one.
"""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from cobrix_amd import aggregate as A
from cobrix_amd import filter as F
from cobrix_amd import keyset as K
from cobrix_amd import native as N
from cobrix_amd.reader import JOIN_MAX_ROWS, ReaderParameters, VarLenNestedReader, _BaseReader
from test_aggregate import _filter_table
from test_filter import FUZZ_N, fuzz_records, py_keep, reader_plan, row_value
from test_group import _hipcc, _key_candidates
from test_keymap import HostMap, _StubReader, map_model
from test_keyset import HostError, _source, expected_set_keep
from test_keyset_from import DIM_SIZE, _mixed, dim, syn  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")
INNER, LEFT = N.JOIN_INNER, N.JOIN_LEFT


# ---------------------------------------------------------------------------------------------
# The contract over decoded rows
# ---------------------------------------------------------------------------------------------
def expected_rows(scb, source_rows, kept, source_names, keys) -> dict:
    """{key: [ordinals, ascending]} for every key of `keys` (the members): the source rows with kept[i] true (None:
    all) whose key it is, numbered by their position in `source_rows`."""
    members = {tuple(k) for k in keys}
    out = {}
    for i, r in enumerate(source_rows):
        if kept is not None and not kept[i]:
            continue
        key = tuple(row_value(scb, r, c) for c in source_names)
        if key in members:
            out.setdefault(key, []).append(i)
    assert set(out) == members
    return out


def expected_expand(pcb, probe_rows, keep_k, names, lists: dict, how: str):
    """(fact index per output row, match per output row): a kept row's outputs are consecutive, one per entry of its
    key's list in list order; LEFT gives a row without a list one output with match -1."""
    fact, match = [], []
    for i, r in enumerate(probe_rows):
        if not keep_k[i]:
            continue
        key = tuple(row_value(pcb, r, c) for c in names)
        rows = lists.get(key, []) if all(v is not None for v in key) else []
        for m in rows:
            fact.append(i)
            match.append(m)
        if not rows and how == "left":
            fact.append(i)
            match.append(-1)
    return np.array(fact, dtype=np.int64), np.array(match, dtype=np.int64)


def rows_model(scb, srows, snames, pplan, names, filters=()):
    """(Model of the member set, {key: (first, count)}, {key: [ordinals]})."""
    m, mp = map_model(scb, srows, snames, pplan, names, filters)
    kept = [py_keep(scb, r, filters) for r in srows] if filters else None
    lists = expected_rows(scb, srows, kept, snames, m.values)
    assert {k: (v[0], len(v)) for k, v in lists.items()} == mp
    return m, mp, lists


# ---------------------------------------------------------------------------------------------
# ABI structs, symbols
# ---------------------------------------------------------------------------------------------
FANOUT_STRUCTS = {"cbx_keymap_rows_info": N.CbxKeymapRowsInfo, "cbx_expand_info": N.CbxJoinExpandInfo}


def test_fanout_struct_layout_matches_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cobrix_hip.h"', "int main(void) {"]
    for cname, py in FANOUT_STRUCTS.items():
        src.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            src.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    src.append('printf("const CBX_ABI_VERSION %d\\n", (int)CBX_ABI_VERSION);')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-I", os.path.dirname(HDR), "-o", str(exe), str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        cname, what, val = line.split()
        seen += 1
        if cname == "const":
            assert N.ABI_VERSION == int(val) == 25   # the extension is additive
        else:
            py = FANOUT_STRUCTS[cname]
            got = ctypes.sizeof(py) if what == "sizeof" else getattr(py, what).offset
            assert got == int(val), f"{cname}.{what}: ctypes {got} != C {val}"
    assert seen == 1 + sum(1 + len(py._fields_) for py in FANOUT_STRUCTS.values())


def test_fanout_symbols():
    assert N.FANOUT_SYMBOLS == ("cbx_key_map_index_rows", "cbx_key_map_rows_info", "cbx_key_map_rows", "cbx_join_records_expand",
                                "cbx_join_expand_info", "cbx_join_expand_pass_times")
    assert set(N.FANOUT_SYMBOLS) <= set(N.EXPORTED_SYMBOLS)
    text = open(HDR).read()
    for s in N.FANOUT_SYMBOLS:
        assert s + "(" in text
    lib = N.load()
    assert all(hasattr(lib, s) for s in N.FANOUT_SYMBOLS)
    # the lookup join's tuple stays as it was
    assert N.KEYMAP_SYMBOLS == ("cbx_key_map_create_from_records", "cbx_key_map_info", "cbx_key_map_destroy", "cbx_key_map_set",
                                "cbx_join_records", "cbx_select_ordinals", "cbx_join_pass_times")


# ---------------------------------------------------------------------------------------------
# The host shim
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("fanout_host") / "libcbx_fanout_host.so"
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(so),
                        os.path.join(ROOT, "tests", "native", "fanout_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_keymap_from_records.argtypes = [P, i32, i32, P, P, i32, i32, P, P, P, P, i64, P, P, P, i64, i32, i32, i32, i64,
                                             ctypes.POINTER(P), P, ctypes.c_char_p, i32]
    lib.cbxh_keymap_destroy.argtypes = [P]
    lib.cbxh_keymap_destroy.restype = None
    lib.cbxh_keymap_pin_failures.argtypes = [P]
    lib.cbxh_keymap_pin_failures.restype = i64
    lib.cbxh_keymap_payload.argtypes = [P, P, P]
    lib.cbxh_keymap_payload.restype = i64
    lib.cbxh_join_check.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.c_char_p, i32]
    lib.cbxh_keyset_create.argtypes = [P, i32, i32, P, P, P, i32, P, i64, ctypes.POINTER(P), ctypes.c_char_p, i32]
    lib.cbxh_keyset_destroy.argtypes = [P]
    lib.cbxh_keyset_destroy.restype = None
    lib.cbxh_fanout_index_rows.argtypes = [P, P, i32, i32, P, P, i32, i32, P, P, P, P, i64, P, P, P, i64, i32, i32, i32,
                                           ctypes.POINTER(P), ctypes.c_char_p, i32]
    lib.cbxh_fanout_lists_destroy.argtypes = [P]
    lib.cbxh_fanout_lists_destroy.restype = None
    lib.cbxh_fanout_lists.argtypes = [P, P, P, P, P]
    lib.cbxh_fanout_lists.restype = i64
    lib.cbxh_fanout_expand.argtypes = [P, i32, i32, P, P, P, i64, P, P, P, i64, i32, i32, i32, P, P, i32, P, P, i32, i64, P, P, P, P,
                                       ctypes.c_char_p, i32]
    lib.cbxh_expand_check.argtypes = [i32, i32, i64, ctypes.c_char_p, i32]
    lib.cbxh_rows_check.argtypes = [i32, i32, i64, i64, ctypes.c_char_p, i32]
    lib.cbxh_fanout_messages.argtypes = [i64, i64, ctypes.c_char_p, ctypes.c_char_p, i32]
    lib.cbxh_fanout_messages.restype = None
    lib.cbxh_rows_sort.argtypes = [P, i64, i32]
    lib.cbxh_rows_sort.restype = None
    lib.cbxh_fanout_bounds.argtypes = [P, P, P]
    lib.cbxh_fanout_bounds.restype = None
    return lib


class HostLists:
    """The row lists the host shim builds for a HostMap from a source's records (any source of the source plan)."""

    def __init__(self, lib, hm: HostMap, pplan, names, splan, source_names, data: bytes, filters=(), stride=0, framing=None,
                 start_off=0):
        self.lib = lib
        pt, st = K.compile_key_pairs(pplan, names, splan, source_names)
        pf = (N.CbxField * len(pplan.fields))(*pplan.fields)
        sf = (N.CbxField * len(splan.fields))(*splan.fields)
        flt = _filter_table(splan, filters)
        buf, src, alive = _source(data, stride, framing)
        err = ctypes.create_string_buffer(256)
        h = ctypes.c_void_p()
        self.handle = None
        rc = lib.cbxh_fanout_index_rows(hm.handle, ctypes.addressof(pf), len(pplan.fields), 0, ctypes.addressof(pt),
                                        ctypes.addressof(sf), len(splan.fields), 0, ctypes.addressof(st),
                                        ctypes.addressof(flt) if flt is not None else None, ctypes.addressof(splan.options.lut),
                                        *src, start_off, -1, ctypes.byref(h), err, 256)
        if rc != 0:
            raise HostError(rc, err.value.decode())
        self.handle = h
        nv = lib.cbxh_keymap_payload(hm.handle, None, None)
        bad, mism = ctypes.c_int64(0), ctypes.c_int64(0)
        total = lib.cbxh_fanout_lists(h, None, None, ctypes.byref(bad), ctypes.byref(mism))
        self.row_start, self.rows = np.zeros(nv + 1, dtype=np.int64), np.zeros(max(1, total), dtype=np.int64)
        lib.cbxh_fanout_lists(h, self.row_start.ctypes.data, self.rows.ctypes.data, None, None)
        self.rows = self.rows[:total]
        self.bad_slots, self.mismatches = bad.value, mism.value

    def segments(self):
        return [self.rows[a:b].tolist() for a, b in zip(self.row_start[:-1], self.row_start[1:])]

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.cbxh_fanout_lists_destroy(self.handle)
            self.handle = None


def host_expand(lib, plan, data: bytes, hm: HostMap, hl, how, capacity=None, sets=(), negate=(), filters=(), stride=0, framing=None,
                start_off=0):
    """(n_out, n_kept, fact, match) of the host shim's expand; capacity None: count first, then the exact size;
    capacity "count": the count-only form."""
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    flt = _filter_table(plan, filters)
    buf, src, alive = _source(data, stride, framing)
    handles = (ctypes.c_void_p * max(1, len(sets)))(*[s.handle for s in sets])
    neg = (ctypes.c_int32 * max(1, len(sets)))(*negate)
    n_out, n_kept = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def call(cap, fact, match):
        err = ctypes.create_string_buffer(256)
        rc = lib.cbxh_fanout_expand(ctypes.addressof(fields), len(plan.fields), 0, ctypes.addressof(flt) if flt is not None else None,
                                    ctypes.addressof(plan.options.lut), *src, start_off, -1,
                                    ctypes.addressof(handles) if sets else None, ctypes.addressof(neg) if sets else None, len(sets),
                                    hm.handle, hl.handle if hl is not None else None, {"inner": 0, "left": 1}.get(how, how), cap,
                                    ctypes.byref(n_out), ctypes.byref(n_kept), fact.ctypes.data if fact is not None else None,
                                    match.ctypes.data if match is not None else None, err, 256)
        if rc != 0:
            raise HostError(rc, err.value.decode())

    if capacity is None or capacity == "count":
        call(0, None, None)
        if capacity == "count":
            return n_out.value, n_kept.value, None, None
        capacity = n_out.value
    fact, match = np.full(max(1, capacity), -7, dtype=np.int64), np.full(max(1, capacity), -7, dtype=np.int64)
    try:
        call(capacity, fact, match)
    except HostError as e:
        e.buffers, e.numbers = (fact, match), (n_out.value, n_kept.value)
        raise
    return n_out.value, n_kept.value, fact[:n_out.value], match[:n_out.value]


def check_lists_and_expand(lib, probe, names, source, snames, filters=(), probe_src=None, source_src=None):
    """probe / source: (copybook, plan, data, rows).  The shim's lists equal the model's, member by member (aligned
    with the payload), and its INNER and LEFT expansions equal expected_expand.  Returns (lists model, INNER fact)."""
    pcb, pplan, pdata, prows = probe
    scb, splan, sdata, srows = source
    probe_src = probe_src or dict(stride=len(pdata) // len(prows))
    source_src = source_src or dict(stride=len(sdata) // len(srows))
    m, mp, lists = rows_model(scb, srows, snames, pplan, names, filters)
    hm = HostMap(lib, pplan, names, splan, snames, sdata, filters, **source_src)
    hl = HostLists(lib, hm, pplan, names, splan, snames, sdata, filters, **source_src)
    assert (hl.bad_slots, hl.mismatches) == (0, 0)
    first, n_rows = hm.payload()
    segs = hl.segments()
    assert sorted(map(tuple, segs)) == sorted(map(tuple, lists.values())), (names, snames)
    assert [s[0] for s in segs] == first.tolist() and [len(s) for s in segs] == n_rows.tolist()
    assert int(hl.row_start[-1]) == int(n_rows.sum()) == len(hl.rows)
    inner = None
    for how in ("inner", "left"):
        fact, match = expected_expand(pcb, prows, np.ones(len(prows), bool), names, lists, how)
        n_out, n_kept, gf, gm = host_expand(lib, pplan, pdata, hm, hl, how, **probe_src)
        assert (n_out, n_kept) == (len(fact), len(set(fact.tolist()))), (names, how)
        assert np.array_equal(gf, fact) and np.array_equal(gm, match), (names, how)
        assert host_expand(lib, pplan, pdata, hm, hl, how, "count", **probe_src)[:2] == (n_out, n_kept)
        if how == "inner":
            inner = fact
    return lists, inner


# ---------------------------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_of_the_c_side(host_shim):
    def status(fn, *args):
        err = ctypes.create_string_buffer(256)
        return fn(*args, err, 256), err.value.decode()

    assert status(host_shim.cbxh_expand_check, 1, 1, 0) == (0, "") and status(host_shim.cbxh_expand_check, 1, 0, 0) == (0, "")
    rc, err = status(host_shim.cbxh_expand_check, 0, 1, 10)
    assert rc == N.CBX_E_STATE and err == "cbx_join_records_expand: the map has no row lists (cbx_key_map_index_rows)"
    for args in ((1, 0, 5), (1, 1, -1)):
        rc, err = status(host_shim.cbxh_expand_check, *args)
        assert rc == N.CBX_E_ARGUMENT and f"out_capacity {args[2]} without output arrays" in err
    assert status(host_shim.cbxh_rows_check, 1, 1, 321, 321) == (0, "")
    for args, word in (((0, 0, 1, 1), "cbx_key_map_index_rows: map: null"),
                       ((1, 0, 1, 1), "cbx_key_map_index_rows: source_plan is not the plan the map was built from"),
                       ((1, 1, 320, 321), "cbx_key_map_index_rows: 320 source records, the map was built from 321")):
        rc, err = status(host_shim.cbxh_rows_check, *args)
        assert rc == N.CBX_E_ARGUMENT and err == word
    # every other refusal of the expand is the lookup join's own, message for message: it shares km_join_check
    for args, word in (((0, 0, 0, 1, 0, 0), "cbx_join_records: map: null"),
                       ((1, 0, 0, 1, 0, 0), "cbx_join_records: map: built for another probe plan"),
                       ((1, 1, 2, 1, 0, 0), "cbx_join_records: join_type 2 is neither CBX_JOIN_INNER nor CBX_JOIN_LEFT"),
                       ((1, 1, 0, 0, 0, 0), "cbx_join_records: d_match must not be NULL"),
                       ((1, 1, 0, 1, 5, 1), "cbx_join_records: 0 to 4 key sets")):
        rc, err = status(host_shim.cbxh_join_check, *args)
        assert rc == N.CBX_E_ARGUMENT and err == word
    cap, differs = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
    host_shim.cbxh_fanout_messages(20865, 20864, cap, differs, 256)
    assert cap.value.decode() == "cbx_join_records_expand: 20865 output rows exceed out_capacity 20864"
    assert differs.value.decode() == "cbx_key_map_index_rows: source differs from the one the map was built from"


def _fake_map(plan, dup=0, most=1, closed=False, lists=True):
    m = SimpleNamespace(plan=plan, closed=closed, n_duplicate_keys=dup, max_rows_per_key=most, handle=None)
    if lists:
        m.index_rows = lambda **kw: None
    return m


def test_check_join_accepts_all_and_join_overflow(syn):  # noqa: F811
    pplan = syn[1]
    assert K.check_join(pplan, _fake_map(pplan, 3, 9), "inner", "all") == N.JOIN_INNER   # duplicates are the point
    assert K.check_join(pplan, _fake_map(pplan), "left", "all") == N.JOIN_LEFT
    with pytest.raises(ValueError, match="neither 'inner' nor 'left'"):
        K.check_join(pplan, _fake_map(pplan), "full", "all")
    with pytest.raises(ValueError, match="nor 'all'"):
        K.check_join(pplan, _fake_map(pplan), "inner", "every")
    with pytest.raises(ValueError, match="closed"):
        K.check_join(pplan, _fake_map(pplan, closed=True), "inner", "all")
    with pytest.raises(ValueError, match="row lists"):   # something that cannot carry lists
        K.check_join(pplan, _fake_map(pplan, lists=False), "inner", "all")
    e = K.JoinOverflow(20865, 1000)
    assert (e.needed, e.max_rows) == (20865, 1000) and "20865 output rows" in str(e) and "max_rows=1000" in str(e)
    assert JOIN_MAX_ROWS == 1 << 26
    for name in ("index_rows", "has_rows", "rows_info", "row_lists"):
        assert hasattr(K.KeyMap, name)


def test_reader_refusals_before_any_launch(syn):  # noqa: F811
    """With duplicates="all" the refusals of `join` come first: no device is there (the data is None)."""
    pplan = syn[1]
    rd = _StubReader(pplan)
    with pytest.raises(A.Unhandled, match="table limits"):
        _BaseReader._join_records(rd, _fake_map(pplan, 2, 3), "inner", [F.In("BR-ID", list(range(65)))], "all", None, 0, 0, None)
    with pytest.raises(A.Unhandled, match="table limits"):
        _BaseReader._join_records(rd, _fake_map(pplan), "left", [F.In("BR-ID", list(range(65)))], "all", None, 0, 0, None,
                                  count_only=True)
    hier = _StubReader(pplan, hierarchical=True)
    for call in (lambda: VarLenNestedReader.join_device(hier, None, 0, None, _fake_map(pplan), duplicates="all"),
                 lambda: VarLenNestedReader.join(hier, b"", _fake_map(pplan), duplicates="all"),
                 lambda: VarLenNestedReader.join_count(hier, b"", _fake_map(pplan)),
                 lambda: VarLenNestedReader.join_count_device(hier, None, 0, None, _fake_map(pplan))):
        with pytest.raises(N.CbxError, match="hierarchical read") as e:
            call()
        assert e.value.code == N.CBX_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# The host/device part on the host
# ---------------------------------------------------------------------------------------------
def test_host_sorting_network_every_length(host_shim):
    """Every length up to 70 and the lengths around powers of two and around both path boundaries, as 1, 3 and 256
    threads would run the steps: a permutation comes out ascending (padding to a power of two is virtual)."""
    s_max, l_max, per_wg = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    host_shim.cbxh_fanout_bounds(ctypes.byref(s_max), ctypes.byref(l_max), ctypes.byref(per_wg))
    assert (s_max.value, l_max.value, per_wg.value) == (16, 4096, 256)
    rng = np.random.default_rng(3)
    lengths = list(range(0, 71)) + [127, 128, 129, 321, 1023, 1025, l_max.value - 1, l_max.value, l_max.value + 1, 5000]
    for n in lengths:
        for threads in (1, 3, 256):
            a = rng.permutation(n).astype(np.int64) * 3 - 7
            want = np.sort(a)
            buf = np.ascontiguousarray(a)
            host_shim.cbxh_rows_sort(buf.ctypes.data, n, threads)
            assert np.array_equal(buf, want), (n, threads)


def _dup_dimension(dim, n=321, keys=7):  # noqa: F811
    """n DIM records over `keys` distinct D-BR values (quadratic residues: uneven fan-outs), D-NAME etc. following."""
    from oracle import reader_oracle as RO
    scb, splan, sdata, srows = dim
    recs = [sdata[DIM_SIZE * i:DIM_SIZE * (i + 1)] for i in range(321)]
    good = [i for i in range(321) if row_value(scb, srows[i], "D-BR") is not None][:keys]
    data = b"".join(recs[good[(i * i) % keys]] for i in range(n))
    return scb, splan, data, RO.fixed_len_rows(scb, data, ReaderParameters(schema_policy="collapse_root"))


def test_host_duplicate_dimension_against_syn200(host_shim, syn, dim):  # noqa: F811
    dup = _dup_dimension(dim)
    lists, inner = check_lists_and_expand(host_shim, syn, ["BR-ID"], dup, ["D-BR"])
    assert len(lists) <= 7 and sum(map(len, lists.values())) == 321 and max(map(len, lists.values())) > 64
    assert len(inner) > len(set(inner.tolist())) > 0   # rows fan out
    # the plain dimension: mostly unique keys, some duplicates; a source filter; a string key; a composite
    for snames, names, filters in ((["D-BR"], ["BR-ID"], []), (["D-BR"], ["BR-ID"], [F.IsNotNull("D-RATE")]),
                                   (["D-NAME"], ["NAME"], []),
                                   (["D-BR", "D-NAME", "D-AMT", "D-BIG"], ["BR-ID", "NAME", "AMT-01", "ACCT-NO"], [])):
        lists, inner = check_lists_and_expand(host_shim, syn, names, dim, snames, filters)
        assert len(inner) > 0
    # record counts around a wave on both sides
    for n in (1, 63, 64, 65):
        check_lists_and_expand(host_shim, syn, ["BR-ID"], (dup[0], dup[1], dup[2][:DIM_SIZE * n], dup[3][:n]), ["D-BR"])
        check_lists_and_expand(host_shim, (syn[0], syn[1], syn[2][:200 * n], syn[3][:n]), ["BR-ID"], dup, ["D-BR"])


def test_host_expand_with_a_filter_a_negated_set_and_capacity(host_shim, syn, dim):  # noqa: F811
    from test_keyset import HostSet, distinct_keys
    pcb, pplan, pdata, prows = syn
    dup = _dup_dimension(dim)
    m, mp, lists = rows_model(dup[0], dup[3], ["D-BR"], pplan, ["BR-ID"])
    hm = HostMap(host_shim, pplan, ["BR-ID"], dup[1], ["D-BR"], dup[2], stride=DIM_SIZE)
    hl = HostLists(host_shim, hm, pplan, ["BR-ID"], dup[1], ["D-BR"], dup[2], stride=DIM_SIZE)
    zd = distinct_keys(pcb, prows, ["ZD-01"])[::2]
    other = HostSet(host_shim, pplan, ["ZD-01"], zd)
    filters = [F.IsNotNull("AMT-01")]
    K_ = expected_set_keep(pcb, prows, filters, [(["ZD-01"], zd, 1)])
    for how in ("inner", "left"):
        fact, match = expected_expand(pcb, prows, K_, ["BR-ID"], lists, how)
        n_out, n_kept, gf, gm = host_expand(host_shim, pplan, pdata, hm, hl, how, None, [other], [1], filters, stride=200)
        assert n_out == len(fact) > n_kept == len(set(fact.tolist())) > 0
        assert np.array_equal(gf, fact) and np.array_equal(gm, match)
        if how == "left":
            assert (match == -1).any() and (match >= 0).any()
        # one row short: CBX_E_CAPACITY, both numbers reported, nothing written
        with pytest.raises(HostError) as e:
            host_expand(host_shim, pplan, pdata, hm, hl, how, n_out - 1, [other], [1], filters, stride=200)
        assert e.value.rc == N.CBX_E_CAPACITY and f"{n_out} output rows exceed out_capacity {n_out - 1}" in e.value.reason
        assert e.value.numbers == (n_out, n_kept) and all((b == -7).all() for b in e.value.buffers)
    # no lists: CBX_E_STATE
    with pytest.raises(HostError) as e:
        host_expand(host_shim, pplan, pdata, hm, None, "inner", 10, stride=200)
    assert e.value.rc == N.CBX_E_STATE and "no row lists" in e.value.reason


def test_host_unique_dimension_equals_the_lookup_join(host_shim, syn, dim):  # noqa: F811
    """On a map without duplicate keys the expansion is the lookup join: same kept rows, same match."""
    from test_keymap import expected_join
    scb, splan, sdata, srows = dim
    seen, recs = set(), []
    for i, r in enumerate(srows):
        v = row_value(scb, r, "D-BR")
        if v is not None and v not in seen:
            seen.add(v)
            recs.append(sdata[DIM_SIZE * i:DIM_SIZE * (i + 1)])
    from oracle import reader_oracle as RO
    data = b"".join(recs)
    uniq = (scb, splan, data, RO.fixed_len_rows(scb, data, ReaderParameters(schema_policy="collapse_root")))
    m, mp, lists = rows_model(uniq[0], uniq[3], ["D-BR"], syn[1], ["BR-ID"])
    assert max(map(len, lists.values())) == 1
    check_lists_and_expand(host_shim, syn, ["BR-ID"], uniq, ["D-BR"])
    for how in ("inner", "left"):
        idx, match, _ = expected_join(syn[0], syn[3], np.ones(321, bool), ["BR-ID"], mp, how)
        fact, fmatch = expected_expand(syn[0], syn[3], np.ones(321, bool), ["BR-ID"], lists, how)
        assert np.array_equal(idx, fact) and np.array_equal(match, fmatch)


def test_host_decoder_fuzz_copybook_as_source_and_probe(host_shim):
    from oracle import reader_oracle as RO
    from test_decode_fuzz import FUZZ_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page="cp037", string_trimming_policy="both",
                         start_offset=3, end_offset=2)
    cb, plan = reader_plan(FUZZ_COPYBOOK, p)
    stride = cb.record_size + 5
    sdata = fuzz_records(cb, FUZZ_N, 31, 3, 2)
    sdata = sdata + sdata[:stride * 40] + sdata[:stride * 40]   # the first 40 records three times: fan-outs of 3 and more
    source = (cb, plan, sdata, RO.fixed_len_rows(cb, sdata, p))
    probe = _mixed(cb, plan, p, sdata, fuzz_records(cb, len(sdata) // stride, 77, 3, 2), stride, 100)
    some = 0
    for cols in _key_candidates(plan, cb).values():
        for names in ([cols[0]], cols[-2:]):
            lists, inner = check_lists_and_expand(host_shim, probe, names, source, names, probe_src=dict(stride=stride, start_off=3),
                                                  source_src=dict(stride=stride, start_off=3))
            some += len(inner) > len(set(inner.tolist()))
    assert some >= 4


def test_host_different_source_with_the_same_record_count(host_shim, syn, dim):  # noqa: F811
    """The map does not keep its source: presented with another one of the same length, the placement rule writes
    nothing outside a member's segment (it does not write at all past n_rows) and the check reports the mismatch."""
    pplan = syn[1]
    dup = _dup_dimension(dim)
    scb, splan, data, rows = dup
    m, mp, lists = rows_model(scb, rows, ["D-BR"], pplan, ["BR-ID"])
    hm = HostMap(host_shim, pplan, ["BR-ID"], splan, ["D-BR"], data, stride=DIM_SIZE)
    n = 321
    recs = [data[DIM_SIZE * i:DIM_SIZE * (i + 1)] for i in range(n)]
    # the same records backwards: every count fits, the first rows do not
    hl = HostLists(host_shim, hm, pplan, ["BR-ID"], splan, ["D-BR"], b"".join(reversed(recs)), stride=DIM_SIZE)
    assert hl.bad_slots == 0 and hl.mismatches == sum(n - 1 - v[-1] != v[0] for v in lists.values()) > 0
    # one member's record n times: its segment is full after n_rows of them, the rest is counted and not written
    key = tuple(row_value(scb, rows[0], c) for c in ["D-BR"])
    hl = HostLists(host_shim, hm, pplan, ["BR-ID"], splan, ["D-BR"], recs[0] * n, stride=DIM_SIZE)
    assert hl.bad_slots == n - len(lists[key]) > 0 and hl.mismatches == len(lists)
    first, n_rows = hm.payload()
    for seg, f, c in zip(hl.segments(), first.tolist(), n_rows.tolist()):
        # (the shim visits the records last to first: the last c copies were placed) -- others' segments are untouched
        assert len(seg) == c and (seg == list(range(n - c, n)) if f == 0 else seg == [-1] * c)
    # a source from which a member is missing: its cursor falls short, another member's runs over
    j = next(i for i in range(n) if row_value(scb, rows[i], "D-BR") != key[0])
    gone = b"".join(recs[j] if row_value(scb, rows[i], "D-BR") == key[0] else recs[i] for i in range(n))
    hl = HostLists(host_shim, hm, pplan, ["BR-ID"], splan, ["D-BR"], gone, stride=DIM_SIZE)
    assert hl.mismatches >= 2 and hl.bad_slots == len(lists[key])
    # and the right source again
    hl = HostLists(host_shim, hm, pplan, ["BR-ID"], splan, ["D-BR"], data, stride=DIM_SIZE)
    assert (hl.bad_slots, hl.mismatches) == (0, 0)


# ---------------------------------------------------------------------------------------------
# The stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snames,names", [(["D-BR"], ["BR-ID"]), (["D-NAME"], ["NAME"])])
def test_host_program_under_the_sanitizers(tmp_path_factory, syn, dim, snames, names):  # noqa: F811
    """tests/native/fanout_host_main.cpp built with -fsanitize=address,undefined over exact-size heap buffers: the lists,
    both expansions (count-only, one row short, exact) and two different sources of the same record count.  A subprocess
    of its own: nothing loaded into Python runs under a sanitizer."""
    pcb, pplan, pdata, prows = syn
    scb, splan, sdata, srows = _dup_dimension(dim, 300) if snames == ["D-BR"] else (dim[0], dim[1], dim[2][:DIM_SIZE * 300], dim[3][:300])
    n = 300
    exe = tmp_path_factory.getbasetemp() / "fanout_host_check"
    if not exe.exists():
        r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "native", "fanout_host_main.cpp")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    m, mp, lists = rows_model(scb, srows, snames, pplan, names)
    flood = next(i for i, r in enumerate(srows) if tuple(row_value(scb, r, c) for c in snames) in lists)
    flood_key = tuple(row_value(scb, srows[flood], c) for c in snames)
    pt, st = K.compile_key_pairs(pplan, names, splan, snames)
    head = struct.pack("<6i3q4i4i", len(pplan.fields), len(splan.fields), 200, DIM_SIZE, len(names), flood, len(prows), n, 65536,
                       *(list(pt.fields)[:4]), *(list(st.fields)[:4]))
    case = tmp_path_factory.mktemp("fx_case") / "case.bin"
    pf = (N.CbxField * len(pplan.fields))(*pplan.fields)
    sf = (N.CbxField * len(splan.fields))(*splan.fields)
    case.write_bytes(head + bytes(pf) + bytes(sf) + bytes(pplan.options.lut) + bytes(splan.options.lut) + pdata + sdata)
    r = subprocess.run([str(exe), str(case)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-4000:], r.stdout)
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    total = sum(map(len, lists.values()))
    want = [["lists", "rows", str(total), "bad", "0", "mismatch", "0", "sum", str(sum(map(sum, lists.values()))), "firsts",
             str(sum(v[0] for v in lists.values())), "sorted", "1"]]
    for how in ("inner", "left"):
        fact, match = expected_expand(pcb, prows, np.ones(len(prows), bool), names, lists, how)
        want.append([how, "out", str(len(fact)), "kept", str(len(set(fact.tolist()))), "short", str(N.CBX_E_CAPACITY), "untouched", "1",
                     "fact", str(int(fact.sum())), "match", str(int(match[match >= 0].sum())), "unmatched", str(int((match < 0).sum()))])
    want.append(["other", "bad", "0", "mismatch", str(sum(n - 1 - v[-1] != v[0] for v in lists.values()))])
    want.append(["flood", "bad", str(n - len(lists[flood_key])), "mismatch", str(len(lists))])
    assert lines == want
    assert int(want[1][2]) > 0
