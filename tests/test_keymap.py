"""Lookup joins (cbx_key_map_create_from_records, cbx_join_records, cbx_select_ordinals), the parts that need no GPU:
the new ABI struct's layout, every refusal with its message, and the host/device part of cobrix_amd/csrc/cbx_keymap.h
(ks_find, the payload update rule, the join verdict, the ordinal gather's row) run on the host
(tests/native/keymap_host.cpp) against a Python model.

The model takes the oracle's rows only: `model_of` (test_keyset_from.py) for the member set, `expected_map` for
{key: (first ordinal, count)} and `expected_join` for (kept indices, match, match_rows).  It never uses the code under
test.  The GPU tests (test_gpu_keymap.py) use the same one.
"""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess
from decimal import Decimal
from types import SimpleNamespace

import numpy as np
import pytest

from cobrix_amd import aggregate as A
from cobrix_amd import filter as F
from cobrix_amd import keyset as K
from cobrix_amd import native as N
from cobrix_amd.reader import ReaderParameters, VarLenNestedReader, _BaseReader, parse_copybook_for
from cobrix_amd.synth import rdw_file
from test_aggregate import _filter_table
from test_filter import (FUZZ_N, FUZZ_OPTIONS, LADDER_COPYBOOK, ascii_records, fuzz_records, ladder_file, ladder_params, narrow_file,
                         narrow_params, py_keep, reader_plan, row_value)
from test_group import EQUAL_COPYBOOK, EQUAL_SIZE, _hipcc, _key_candidates, equal_records
from test_keyset import HostError, _source, expected_set_keep
from test_keyset_from import DIM_COPYBOOK, DIM_SIZE, _mixed, counts_of, dim, model_of, syn  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")


# ---------------------------------------------------------------------------------------------
# The contract over decoded rows
# ---------------------------------------------------------------------------------------------
def expected_map(scb, source_rows, kept, source_names, keys) -> dict:
    """{key: (first ordinal, count)} for every key of `keys` (the members): over the source rows with kept[i] true
    (None: all), numbered by their position in `source_rows`."""
    members = {tuple(k) for k in keys}
    out = {}
    for i, r in enumerate(source_rows):
        if kept is not None and not kept[i]:
            continue
        key = tuple(row_value(scb, r, c) for c in source_names)
        if key in members:
            first, n = out.get(key, (i, 0))
            out[key] = (first, n + 1)
    assert set(out) == members   # every member came from a kept row
    return out


def expected_join(pcb, probe_rows, keep_k, names, mp: dict, how: str):
    """(kept indices, match, match_rows): K from the caller, m(r) from the map, the keep rule of the join type."""
    idx, match, rows = [], [], []
    for i, r in enumerate(probe_rows):
        if not keep_k[i]:
            continue
        key = tuple(row_value(pcb, r, c) for c in names)
        first, n = mp.get(key, (-1, 0)) if all(v is not None for v in key) else (-1, 0)
        if how == "left" or first >= 0:
            idx.append(i)
            match.append(first)
            rows.append(n)
    return np.array(idx, dtype=np.int64), np.array(match, dtype=np.int64), np.array(rows, dtype=np.int64)


def map_model(scb, srows, snames, pplan, names, filters=()):
    """(Model of the member set, {key: (first, count)})."""
    m = model_of(scb, srows, snames, pplan, names, filters)
    kept = [py_keep(scb, r, filters) for r in srows] if filters else None
    return m, expected_map(scb, srows, kept, snames, m.values)


def duplicates_of(mp: dict):
    counts = [n for _, n in mp.values()]
    return sum(n > 1 for n in counts), max(counts, default=0)


# ---------------------------------------------------------------------------------------------
# ABI struct, symbols
# ---------------------------------------------------------------------------------------------
KEYMAP_STRUCTS = {"cbx_keymap_info": N.CbxKeymapInfo, "cbx_keyset_source_info": N.CbxKeysetSourceInfo}


def test_keymap_struct_layout_matches_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cobrix_hip.h"', "int main(void) {"]
    for cname, py in KEYMAP_STRUCTS.items():
        src.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            src.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    src.append('printf("const CBX_ABI_VERSION %d\\n", (int)CBX_ABI_VERSION);')
    src.append('printf("const CBX_JOIN_INNER %d\\n", (int)CBX_JOIN_INNER);')
    src.append('printf("const CBX_JOIN_LEFT %d\\n", (int)CBX_JOIN_LEFT);')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-I", os.path.dirname(HDR), "-o", str(exe), str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    consts = {"CBX_ABI_VERSION": N.ABI_VERSION, "CBX_JOIN_INNER": N.JOIN_INNER, "CBX_JOIN_LEFT": N.JOIN_LEFT}
    seen = 0
    for line in filter(None, out):
        cname, what, val = line.split()
        seen += 1
        if cname == "const":
            assert consts[what] == int(val)
        else:
            py = KEYMAP_STRUCTS[cname]
            got = ctypes.sizeof(py) if what == "sizeof" else getattr(py, what).offset
            assert got == int(val), f"{cname}.{what}: ctypes {got} != C {val}"
    assert seen == 3 + sum(1 + len(py._fields_) for py in KEYMAP_STRUCTS.values())
    assert N.ABI_VERSION == 25
    # the map's info starts with the source info, field by field
    n = len(N.CbxKeysetSourceInfo._fields_)
    assert N.CbxKeymapInfo._fields_[:n] == N.CbxKeysetSourceInfo._fields_
    for fname, _ in N.CbxKeysetSourceInfo._fields_:
        assert getattr(N.CbxKeymapInfo, fname).offset == getattr(N.CbxKeysetSourceInfo, fname).offset


def test_keymap_symbols():
    assert N.KEYMAP_SYMBOLS == ("cbx_key_map_create_from_records", "cbx_key_map_info", "cbx_key_map_destroy", "cbx_key_map_set",
                                "cbx_join_records", "cbx_select_ordinals", "cbx_join_pass_times")
    assert set(N.KEYMAP_SYMBOLS) <= set(N.EXPORTED_SYMBOLS)
    text = open(HDR).read()
    for s in N.KEYMAP_SYMBOLS:
        assert s + "(" in text
    lib = N.load()
    assert all(hasattr(lib, s) for s in N.KEYMAP_SYMBOLS)
    # the earlier extensions' tuples stay as they were
    assert N.KEYSET_FROM_SYMBOLS == ("cbx_key_set_create_from_records",)
    assert N.KEYSET_SYMBOLS == ("cbx_key_set_create", "cbx_key_set_info", "cbx_key_set_destroy", "cbx_filter_records_keyed")


# ---------------------------------------------------------------------------------------------
# The host shim
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("keymap_host") / "libcbx_keymap_host.so"
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(so),
                        os.path.join(ROOT, "tests", "native", "keymap_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_keymap_from_records.argtypes = [P, i32, i32, P, P, i32, i32, P, P, P, P, i64, P, P, P, i64, i32, i32, i32, i64,
                                             ctypes.POINTER(P), P, ctypes.c_char_p, i32]
    lib.cbxh_keymap_destroy.argtypes = [P]
    lib.cbxh_keymap_destroy.restype = None
    lib.cbxh_keymap_set.argtypes = [P]
    lib.cbxh_keymap_set.restype = P
    lib.cbxh_keymap_pin_failures.argtypes = [P]
    lib.cbxh_keymap_pin_failures.restype = i64
    lib.cbxh_keymap_payload.argtypes = [P, P, P]
    lib.cbxh_keymap_payload.restype = i64
    lib.cbxh_keymap_join.argtypes = [P, i32, i32, P, P, P, i64, P, P, P, i64, i32, i32, i32, P, P, i32, P, i32, P, P, P,
                                     ctypes.c_char_p, i32]
    lib.cbxh_join_check.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.c_char_p, i32]
    lib.cbxh_ordinal_rows.argtypes = [P, i64, i64, P, P, i32, i64, P, P, P, P]
    lib.cbxh_ordinal_rows.restype = None
    lib.cbxh_keyset_create.argtypes = [P, i32, i32, P, P, P, i32, P, i64, ctypes.POINTER(P), ctypes.c_char_p, i32]
    lib.cbxh_keyset_info.argtypes = [P, P]
    lib.cbxh_keyset_info.restype = None
    lib.cbxh_keyset_destroy.argtypes = [P]
    lib.cbxh_keyset_destroy.restype = None
    lib.cbxh_keyset_keep.argtypes = [P, i32, i32, P, P, P, i64, P, P, P, i64, i32, i32, i32, P, P, i32, P, ctypes.c_char_p, i32]
    return lib


class HostMap:
    """A key map of `pplan` over `names` the host shim builds from the `source_names` keys of a source's records."""

    def __init__(self, lib, pplan, names, splan, source_names, data: bytes, filters=(), stride=0, framing=None, start_off=0,
                 max_values=65536):
        self.lib, self.plan = lib, pplan
        pt, st = K.compile_key_pairs(pplan, names, splan, source_names)
        pf = (N.CbxField * len(pplan.fields))(*pplan.fields)
        sf = (N.CbxField * len(splan.fields))(*splan.fields)
        flt = _filter_table(splan, filters)
        buf, src, alive = _source(data, stride, framing)
        self.info = N.CbxKeymapInfo()
        err = ctypes.create_string_buffer(256)
        h = ctypes.c_void_p()
        self.handle = None
        rc = lib.cbxh_keymap_from_records(ctypes.addressof(pf), len(pplan.fields), 0, ctypes.addressof(pt), ctypes.addressof(sf),
                                          len(splan.fields), 0, ctypes.addressof(st),
                                          ctypes.addressof(flt) if flt is not None else None, ctypes.addressof(splan.options.lut),
                                          *src, start_off, -1, max_values, ctypes.byref(h), ctypes.addressof(self.info), err, 256)
        if rc != 0:
            raise HostError(rc, err.value.decode())
        self.handle = h

    @property
    def pin_failures(self) -> int:
        return self.lib.cbxh_keymap_pin_failures(self.handle)

    def payload(self):
        n = self.lib.cbxh_keymap_payload(self.handle, None, None)
        first, rows = np.zeros(max(1, n), dtype=np.int64), np.zeros(max(1, n), dtype=np.int64)
        self.lib.cbxh_keymap_payload(self.handle, first.ctypes.data, rows.ctypes.data)
        return first[:n], rows[:n]

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.cbxh_keymap_destroy(self.handle)
            self.handle = None


def host_join(lib, plan, data: bytes, hm: HostMap, how: str, sets=(), negate=(), filters=(), stride=0, framing=None, start_off=0):
    """(keep, match, rows) per input record of the host shim's join verdict."""
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    flt = _filter_table(plan, filters)
    buf, src, alive = _source(data, stride, framing)
    n = src[5]
    keep = np.zeros(max(1, n), dtype=np.uint8)
    match, rows = np.zeros(max(1, n), dtype=np.int64), np.zeros(max(1, n), dtype=np.int64)
    handles = (ctypes.c_void_p * max(1, len(sets)))(*[s.handle for s in sets])
    neg = (ctypes.c_int32 * max(1, len(sets)))(*negate)
    err = ctypes.create_string_buffer(256)
    rc = lib.cbxh_keymap_join(ctypes.addressof(fields), len(plan.fields), 0, ctypes.addressof(flt) if flt is not None else None,
                              ctypes.addressof(plan.options.lut), *src, start_off, -1, ctypes.addressof(handles) if sets else None,
                              ctypes.addressof(neg) if sets else None, len(sets), hm.handle, {"inner": 0, "left": 1}.get(how, how),
                              keep.ctypes.data, match.ctypes.data, rows.ctypes.data, err, 256)
    if rc != 0:
        raise HostError(rc, err.value.decode())
    return keep[:n].astype(bool), match[:n], rows[:n]


def check_map(lib, probe, names, source, snames, filters=(), probe_src=None, source_src=None):
    """probe / source: (copybook, plan, data, rows).  The host shim's map equals the model's -- counts, the pinned
    assumption, the payload as a multiset, the duplicate numbers -- and its INNER and LEFT joins over the probe records
    equal expected_join.  Returns (map model, INNER keep flags)."""
    pcb, pplan, pdata, prows = probe
    scb, splan, sdata, srows = source
    probe_src = probe_src or dict(stride=len(pdata) // len(prows))
    source_src = source_src or dict(stride=len(sdata) // len(srows))
    m, mp = map_model(scb, srows, snames, pplan, names, filters)
    hm = HostMap(lib, pplan, names, splan, snames, sdata, filters, **source_src)
    assert counts_of(hm.info) == m.counts(), (names, snames, counts_of(hm.info), m.counts())
    assert hm.pin_failures == 0, (names, snames)
    first, rows = hm.payload()
    assert sorted(zip(first.tolist(), rows.tolist())) == sorted(mp.values()), (names, snames)
    assert (hm.info.n_duplicate_keys, hm.info.max_rows_per_key) == duplicates_of(mp)
    inner = None
    for how in ("inner", "left"):
        idx, match, mrows = expected_join(pcb, prows, np.ones(len(prows), bool), names, mp, how)
        keep, gm, gr = host_join(lib, pplan, pdata, hm, how, **probe_src)
        assert np.array_equal(np.flatnonzero(keep), idx), (names, how)
        assert np.array_equal(gm[keep], match) and np.array_equal(gr[keep], mrows), (names, how)
        if how == "inner":
            inner = keep
            assert np.array_equal(keep, expected_set_keep(pcb, prows, [], [(names, m.values, 0)]))
        else:
            assert keep.all()
    return mp, inner


# ---------------------------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------------------------
def test_join_argument_refusals_of_the_c_side(host_shim):
    def status(*args):
        err = ctypes.create_string_buffer(256)
        return host_shim.cbxh_join_check(*args, err, 256), err.value.decode()

    assert status(1, 1, 0, 1, 0, 0) == (0, "") and status(1, 1, 1, 1, 4, 1) == (0, "")
    for args, word in (((0, 0, 0, 1, 0, 0), "cbx_join_records: map: null"),
                       ((1, 0, 0, 1, 0, 0), "cbx_join_records: map: built for another probe plan"),
                       ((1, 1, 2, 1, 0, 0), "cbx_join_records: join_type 2 is neither CBX_JOIN_INNER nor CBX_JOIN_LEFT"),
                       ((1, 1, -1, 1, 0, 0), "join_type -1"),
                       ((1, 1, 0, 0, 0, 0), "cbx_join_records: d_match must not be NULL"),
                       ((1, 1, 0, 1, 5, 1), "cbx_join_records: 0 to 4 key sets"),
                       ((1, 1, 0, 1, -1, 1), "0 to 4 key sets"), ((1, 1, 0, 1, 1, 0), "0 to 4 key sets")):
        rc, err = status(*args)
        assert rc == N.CBX_E_ARGUMENT and word in err, (args, err)


def _fake_map(plan, dup=0, most=1, closed=False):
    return SimpleNamespace(plan=plan, closed=closed, n_duplicate_keys=dup, max_rows_per_key=most, handle=None)


def test_check_join_every_refusal(syn, dim):  # noqa: F811
    pplan, splan = syn[1], dim[1]
    assert K.check_join(pplan, _fake_map(pplan), "inner", "error") == N.JOIN_INNER
    assert K.check_join(pplan, _fake_map(pplan), "left", "error") == N.JOIN_LEFT
    assert K.check_join(pplan, _fake_map(pplan, 3, 9), "left", "first") == N.JOIN_LEFT
    with pytest.raises(ValueError, match="neither 'inner' nor 'left'"):
        K.check_join(pplan, _fake_map(pplan), "right", "error")
    with pytest.raises(ValueError, match="neither 'error' nor 'first'"):
        K.check_join(pplan, _fake_map(pplan), "inner", "all")
    with pytest.raises(ValueError, match="closed"):
        K.check_join(pplan, _fake_map(pplan, closed=True), "inner", "error")
    with pytest.raises(N.CbxError, match="built for another reader's plan") as e:
        K.check_join(pplan, _fake_map(splan), "inner", "error")
    assert e.value.code == N.CBX_E_ARGUMENT
    with pytest.raises(K.DuplicateKeys, match="3 dimension keys have more than one row .up to 9 rows per key") as e:
        K.check_join(pplan, _fake_map(pplan, 3, 9), "inner", "error")
    assert (e.value.n_duplicate_keys, e.value.max_rows_per_key) == (3, 9)
    with pytest.raises(TypeError, match="from_records"):
        K.KeyMap()


class _StubReader(_BaseReader):
    """A reader's Python side without a device plan: what the refusals in front of every launch look at."""

    def __init__(self, plan, hierarchical=False):
        self.plan, self.hierarchical = plan, hierarchical


def test_reader_refusals_before_any_launch(syn, dim):  # noqa: F811
    """An unpushed filter and DuplicateKeys raise before the join touches the device (no device is there: the data is
    None); hierarchical readers refuse on both sides."""
    pplan = syn[1]
    rd = _StubReader(pplan)
    with pytest.raises(A.Unhandled, match="table limits"):
        _BaseReader._join_records(rd, _fake_map(pplan), "inner", [F.In("BR-ID", list(range(65)))], "error", None, 0, 0, None)
    with pytest.raises(K.DuplicateKeys):
        _BaseReader._join_records(rd, _fake_map(pplan, 1, 2), "left", None, "error", None, 0, 0, None)
    with pytest.raises(A.Unhandled, match="table limits"):   # the source side: a map over unfiltered rows would be wrong
        _BaseReader._key_map_from(_StubReader(dim[1]), ["D-BR"], rd, ["BR-ID"], [F.In("D-BR", list(range(65)))], 65536,
                                  None, 0, 0, None)
    hier = _StubReader(pplan, hierarchical=True)
    for call in (lambda: VarLenNestedReader.key_map_of_device(hier, None, 0, None, ["K"], rd),
                 lambda: VarLenNestedReader.key_map_of(hier, b"", ["K"], rd),
                 lambda: VarLenNestedReader.join_device(hier, None, 0, None, _fake_map(pplan)),
                 lambda: VarLenNestedReader.join(hier, b"", _fake_map(pplan))):
        with pytest.raises(N.CbxError, match="hierarchical read") as e:
            call()
        assert e.value.code == N.CBX_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# The host/device part on the host
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snames,names", [(["D-BR"], ["BR-ID"]), (["D-ACCT"], ["ACCT-NO"]), (["D-AMT"], ["AMT-01"]),
                                          (["D-NAME"], ["NAME"]), (["D-BIG"], ["ACCT-NO"]),
                                          (["D-BR", "D-NAME", "D-AMT", "D-BIG"], ["BR-ID", "NAME", "AMT-01", "ACCT-NO"])])
def test_host_dimension_against_syn200(host_shim, syn, dim, snames, names):  # noqa: F811
    for filters in ([], [F.IsNotNull("D-RATE")], [F.GreaterThan("D-BR", 0), F.LessThan("D-AMT", Decimal("5000000.00"))]):
        mp, inner = check_map(host_shim, syn, names, dim, snames, filters)
        assert 0 < inner.sum() < len(inner), (snames, filters)
    # the dimension against itself under its own columns: every non-null row finds the FIRST row with its key
    mp, inner = check_map(host_shim, dim, snames, dim, snames)
    keep, match, _ = host_join(host_shim, dim[1], dim[2], HostMap(host_shim, dim[1], snames, dim[1], snames, dim[2], stride=DIM_SIZE),
                               "inner", stride=DIM_SIZE)
    assert (match[keep] <= np.flatnonzero(keep)).all() and (match[keep] == np.flatnonzero(keep)).any()


def test_host_duplicate_dimension_keys_and_record_counts(host_shim, syn, dim):  # noqa: F811
    scb, splan, sdata, srows = dim
    recs = [sdata[DIM_SIZE * i:DIM_SIZE * (i + 1)] for i in range(321)]
    good = [i for i in range(321) if row_value(scb, srows[i], "D-BR") is not None][:7]
    from oracle import reader_oracle as RO
    data = b"".join(recs[good[(i * i) % 7]] for i in range(321))
    dup = (scb, splan, data, RO.fixed_len_rows(scb, data, ReaderParameters(schema_policy="collapse_root")))
    mp, _ = check_map(host_shim, syn, ["BR-ID"], dup, ["D-BR"])
    assert len(mp) <= 7 and duplicates_of(mp)[0] == len(mp) and sum(n for _, n in mp.values()) == 321
    assert sorted(f for f, _ in mp.values())[0] == 0
    for n in (1, 63, 64, 65):
        part = (scb, splan, sdata[:DIM_SIZE * n], srows[:n])
        check_map(host_shim, syn, ["BR-ID"], part, ["D-BR"])
        check_map(host_shim, (syn[0], syn[1], syn[2][:200 * n], syn[3][:n]), ["BR-ID"], dim, ["D-BR"])
    # an empty source, a source filter that keeps nothing: LEFT keeps every row with -1, INNER none
    for hm in (HostMap(host_shim, syn[1], ["BR-ID"], splan, ["D-BR"], b"", stride=DIM_SIZE),
               HostMap(host_shim, syn[1], ["BR-ID"], splan, ["D-BR"], sdata, [F.GreaterThan("D-BR", 10 ** 6)], stride=DIM_SIZE)):
        assert (hm.info.n_duplicate_keys, hm.info.max_rows_per_key, hm.pin_failures) == (0, 0, 0)
        keep, match, rows = host_join(host_shim, syn[1], syn[2], hm, "left", stride=200)
        assert keep.all() and (match == -1).all() and (rows == 0).all()
        assert not host_join(host_shim, syn[1], syn[2], hm, "inner", stride=200)[0].any()


def test_host_join_with_a_filter_and_a_negated_set(host_shim, syn, dim):  # noqa: F811
    from test_keyset import HostSet, distinct_keys
    pcb, pplan, pdata, prows = syn
    m, mp = map_model(dim[0], dim[3], ["D-BR"], pplan, ["BR-ID"])
    hm = HostMap(host_shim, pplan, ["BR-ID"], dim[1], ["D-BR"], dim[2], stride=DIM_SIZE)
    zd = distinct_keys(pcb, prows, ["ZD-01"])[::2]
    other = HostSet(host_shim, pplan, ["ZD-01"], zd)
    filters = [F.IsNotNull("AMT-01")]
    K_ = expected_set_keep(pcb, prows, filters, [(["ZD-01"], zd, 1)])
    for how in ("inner", "left"):
        idx, match, mrows = expected_join(pcb, prows, K_, ["BR-ID"], mp, how)
        keep, gm, gr = host_join(host_shim, pplan, pdata, hm, how, [other], [1], filters, stride=200)
        assert np.array_equal(np.flatnonzero(keep), idx) and np.array_equal(gm[keep], match) and np.array_equal(gr[keep], mrows)
        assert 0 < len(idx) < 321
    assert (expected_join(pcb, prows, K_, ["BR-ID"], mp, "left")[1] == -1).any()


@pytest.mark.parametrize("start,end", [(0, 0), (3, 2)])
@pytest.mark.parametrize("code_page,trim", FUZZ_OPTIONS)
def test_host_every_key_kind_ebcdic(host_shim, code_page, trim, start, end):
    """The decoder fuzz copybook as source and as probe: every accepted key kind on both sides of the map."""
    from oracle import reader_oracle as RO
    from test_decode_fuzz import FUZZ_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim,
                         start_offset=start, end_offset=end)
    cb, plan = reader_plan(FUZZ_COPYBOOK, p)
    stride = cb.record_size + start + end
    sdata = fuzz_records(cb, FUZZ_N, 31, start, end)
    source = (cb, plan, sdata, RO.fixed_len_rows(cb, sdata, p))
    probe = _mixed(cb, plan, p, sdata, fuzz_records(cb, FUZZ_N, 77, start, end), stride, 100)
    by_kind = _key_candidates(plan, cb)
    assert {k for k, _ in by_kind} >= {N.K_STRING, N.K_BCD, N.K_BINARY, N.K_ZONED}
    some = 0
    for cols in by_kind.values():
        for names in ([cols[0]], cols[-2:]):
            _, inner = check_map(host_shim, probe, names, source, names, probe_src=dict(stride=stride, start_off=start),
                                 source_src=dict(stride=stride, start_off=start))
            some += 0 < inner.sum() < len(inner)
    assert some >= len(by_kind)


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_host_every_key_kind_ascii(host_shim, charset):
    from oracle import reader_oracle as RO
    from test_decode_fuzz import ASCII_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
    cb, plan = reader_plan(ASCII_COPYBOOK, p)
    sdata = ascii_records(cb, FUZZ_N, 32)
    source = (cb, plan, sdata, RO.fixed_len_rows(cb, sdata, p))
    probe = _mixed(cb, plan, p, sdata, ascii_records(cb, FUZZ_N, 78), cb.record_size, 100)
    for cols in _key_candidates(plan, cb).values():
        assert check_map(host_shim, probe, cols[:1], source, cols[:1])[1].any()


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_short_records(host_shim, trim):
    """Strings of every width class cut by short records on both sides: a key past the record's end is null (no member,
    no match), one that starts at its end is ""."""
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    sraw, soff, sln = ladder_file(seed=34, every_length=True)
    praw, poff, pln = ladder_file(n=300, seed=35)
    source = (cb, plan, sraw, RO.var_len_rows(cb, sraw, p))
    probe = (cb, plan, praw, RO.var_len_rows(cb, praw, p))
    for names in (["X05"], ["X32"], ["X01"], ["P05"], ["Z07"], ["X03", "P03"], ["X02", "X01", "Z01", "P01"]):
        mp, inner = check_map(host_shim, probe, names, source, names, probe_src=dict(framing=(poff, pln, None)),
                              source_src=dict(framing=(soff, sln, None)))
        if names == ["X01"]:
            assert inner.any() and duplicates_of(mp)[0] > 0
    check_map(host_shim, probe, ["X05"], source, ["X12"], probe_src=dict(framing=(poff, pln, None)),
              source_src=dict(framing=(soff, sln, None)))   # what does not fit is dropped: those rows find no member


def test_host_segment_redefines(host_shim):
    from cobrix_amd.synth import RDW_NARROW_COPYBOOK
    from oracle import oracle as O
    from oracle import reader_oracle as RO
    p = narrow_params()
    cb, plan = reader_plan(RDW_NARROW_COPYBOOK, p)
    groups = [g.name.upper() for g in plan.segment_groups]

    def side(n, seed):
        raw = narrow_file(n, seed)
        off, ln = O.frame_rdw(raw)
        recs = RO.var_len_records(cb, raw, p)
        seg = np.array([groups.index(r.active_segment.upper()) if r.active_segment is not None else -1 for r in recs], dtype=np.int32)
        return (cb, plan, raw, RO.var_len_rows(cb, raw, p)), dict(framing=(off, ln, seg))

    source, ssrc = side(300, 21)
    probe, psrc = side(321, 22)
    for names in (["SEGMENT-ID"], ["TAXPAYER-NUM"], ["SEGMENT-ID", "TAXPAYER-TYPE"]):
        for filters in ([], [F.EqualTo("SEGMENT-ID", "C")]):
            mp, inner = check_map(host_shim, probe, names, source, names, filters, probe_src=psrc, source_src=ssrc)
            assert inner.any(), names
    mp, _ = check_map(host_shim, probe, ["SEGMENT-ID"], source, ["SEGMENT-ID"], probe_src=psrc, source_src=ssrc)
    assert duplicates_of(mp)[1] > 100


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_equal_values_of_different_bytes_share_the_lowest_ordinal(host_shim, trim):
    """The copybook of test_group.py: sign nibbles of a COMP-3 zero, overpunch spellings, padding and code-page twins
    are one member each, and its first_row is the lowest ordinal among ALL its spellings."""
    from oracle import reader_oracle as RO
    p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=trim)
    cb, plan = reader_plan(EQUAL_COPYBOOK, p)
    data = equal_records(plan)
    rows = RO.fixed_len_rows(cb, data, p)
    whole = (cb, plan, data, rows)
    n = len(rows)
    back = b"".join(data[EQUAL_SIZE * i:EQUAL_SIZE * (i + 1)] for i in reversed(range(n)))
    flipped = (cb, plan, back, rows[::-1])
    for names in (["KB"], ["KP"], ["KZ"], ["KX4"], ["KX3"], ["KB", "KP", "KX4", "KX3"]):
        mp, _ = check_map(host_shim, whole, names, whole, names)
        assert duplicates_of(mp)[0] > 0
        mp2, _ = check_map(host_shim, whole, names, flipped, names)   # another spelling comes first
        assert set(mp) == set(mp2) and {k: c for k, (_, c) in mp.items()} == {k: c for k, (_, c) in mp2.items()}


def test_host_ordinal_rows(host_shim):
    n = 10
    off = np.arange(n, dtype=np.int64) * 50 + 4
    ln = (np.arange(n, dtype=np.int32) * 3) % 46 + 1
    ord_ = np.array([9, 9, 5, 4, 3, 0, 10, -1, 2 ** 40, 7], dtype=np.int64)
    for framed in (True, False):
        o_off, o_id = np.zeros(len(ord_), np.int64), np.zeros(len(ord_), np.int64)
        o_len, o_seg = np.zeros(len(ord_), np.int32), np.zeros(len(ord_), np.int32)
        host_shim.cbxh_ordinal_rows(ord_.ctypes.data, len(ord_), n, off.ctypes.data if framed else None,
                                    ln.ctypes.data if framed else None, 0 if framed else 50, 1000, o_off.ctypes.data,
                                    o_len.ctypes.data, o_id.ctypes.data, o_seg.ctypes.data)
        for j, o in enumerate(ord_.tolist()):
            if 0 <= o < n:
                want = (int(off[o]), int(ln[o]), 1000 + o) if framed else (50 * o, 50, 1000 + o)
            else:
                want = (0, 0, -1)   # a zero-length record at offset 0
            assert (int(o_off[j]), int(o_len[j]), int(o_id[j]), int(o_seg[j])) == want + (-1,), (framed, j)


# ---------------------------------------------------------------------------------------------
# The stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snames,names", [(["D-BR"], ["BR-ID"]), (["D-NAME"], ["NAME"]), (["D-BIG", "D-NAME", "D-AMT"], ["ACCT-NO", "NAME", "AMT-01"])])
def test_host_program_under_the_sanitizers(tmp_path_factory, syn, dim, snames, names):  # noqa: F811
    """tests/native/keymap_host_main.cpp built with -fsanitize=address,undefined over exact-size heap buffers: a fixed
    source run and a framed run that cuts the source records inside and in front of the key fields, each joined INNER
    and LEFT with the SYN200 records, and an ordinal gather.  A subprocess of its own: nothing loaded into Python runs
    under a sanitizer."""
    pcb, pplan, pdata, prows = syn
    scb, splan, sdata, srows = dim
    n = 300
    exe = tmp_path_factory.getbasetemp() / "keymap_host_check"
    if not exe.exists():
        r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "native", "keymap_host_main.cpp")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    pt, st = K.compile_key_pairs(pplan, names, splan, snames)
    head = struct.pack("<6i3q4i4i", len(pplan.fields), len(splan.fields), 200, DIM_SIZE, len(names), 0, len(prows), n, 65536,
                       *(list(pt.fields)[:4]), *(list(st.fields)[:4]))
    case = tmp_path_factory.mktemp("km_case") / "case.bin"
    pf = (N.CbxField * len(pplan.fields))(*pplan.fields)
    sf = (N.CbxField * len(splan.fields))(*splan.fields)
    blob = sdata[:DIM_SIZE * n]
    case.write_bytes(head + bytes(pf) + bytes(sf) + bytes(pplan.options.lut) + bytes(splan.options.lut) + pdata + blob)
    r = subprocess.run([str(exe), str(case)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-4000:], r.stdout)
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    from oracle import reader_oracle as RO
    cuts = [(DIM_SIZE * i, (7 * i) % DIM_SIZE + 1) for i in range(n)]
    for back in range(1, DIM_SIZE + 1):
        cuts[n - back] = (len(blob) - back, back)
    vp = ReaderParameters(is_record_sequence=True, schema_policy="collapse_root")
    vcb = parse_copybook_for(DIM_COPYBOOK, vp)
    cut_rows = RO.var_len_rows(vcb, rdw_file([blob[o:o + ln] for o, ln in cuts]), vp)
    assert len(cut_rows) == n
    want = []
    for name, cb, rows in (("fixed", scb, srows[:n]), ("framed", vcb, cut_rows)):
        m, mp = map_model(cb, rows, snames, pplan, names)
        dups, most = duplicates_of(mp)
        want.append([name, "map", "values", str(len(mp)), "dup", str(dups), "max", str(most), "pins", "0", "first",
                     str(sum(f for f, _ in mp.values())), "rows", str(sum(c for _, c in mp.values()))])
        for how in ("inner", "left"):
            idx, match, mrows = expected_join(pcb, prows, np.ones(len(prows), bool), names, mp, how)
            want.append([name, how, "kept", str(len(idx)), "matched", str(int((match >= 0).sum())), "match",
                         str(int(match[match >= 0].sum())), "rows", str(int(mrows.sum()))])
    picks = [n - 1, n - 1, n // 2, 0]
    want.append(["ordinals", str(sum(cuts[i][0] for i in picks)), str(sum(cuts[i][1] for i in picks)),
                 str(sum(1000 + i for i in picks) - 2)])
    assert lines == want
    assert 0 < int(want[1][3]) < len(prows)
