"""Key-set filters (InSet / NotInSet), the parts that need no GPU: compile_key_values and compile_filters_with_sets with
every refusal, the new ABI structs' layout, and the host/device part of cobrix_amd/csrc/cbx_keyset.h (keyset_layout,
the value-side hash, insert with fingerprints, the record-side key, the membership test) run on the host
(tests/native/keyset_host.cpp) against a Python evaluator.

The evaluator (`expected_set_keep`) takes the oracle's rows, `row_value` of the key columns and Python set membership,
with None giving "not kept"; it never uses the code under test.  The GPU tests (test_gpu_keyset.py) use the same one.
"""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess
from decimal import Decimal

import numpy as np
import pytest

from cobrix_amd import filter as F
from cobrix_amd import keyset as K
from cobrix_amd import native as N
from cobrix_amd.reader import ReaderParameters
from cobrix_amd.synth import SYN200_COPYBOOK
from test_aggregate import _filter_table, _fi
from test_filter import (FUZZ_N, FUZZ_OPTIONS, LADDER_COPYBOOK, WIDE_COPYBOOK, ascii_records, fuzz_records, ladder_file,
                         ladder_params, narrow_file, narrow_params, py_keep, reader_plan, row_value)
from test_group import (EQUAL_COPYBOOK, EQUAL_SIZE, _hipcc, _key_candidates, _plan, equal_records, syn_plan,  # noqa: F401
                        syn_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")


# ---------------------------------------------------------------------------------------------
# The contract over decoded rows
# ---------------------------------------------------------------------------------------------
def expected_set_keep(cb, rows, filters, sets) -> np.ndarray:
    """keep[i]: the filters are true and, for every (names, values, negate) of `sets`, the row's key has no None and
    is (not) one of the values."""
    members = [(names, {tuple(v) if isinstance(v, (tuple, list)) else (v,) for v in values}, negate)
               for names, values, negate in sets]
    out = np.zeros(len(rows), dtype=bool)
    for i, r in enumerate(rows):
        keep = py_keep(cb, r, filters) if filters else True
        for names, vals, negate in members:
            if not keep:
                break
            key = tuple(row_value(cb, r, n) for n in names)
            keep = all(v is not None for v in key) and ((key in vals) != bool(negate))
        out[i] = keep
    return out


def distinct_keys(cb, rows, names):
    """The distinct key tuples without a None, in a fixed order."""
    keys = {tuple(row_value(cb, r, n) for n in names) for r in rows}
    return sorted((k for k in keys if all(v is not None for v in k)), key=repr)


def half(keys):
    """Every other key: a set that keeps some rows and drops some."""
    return keys[::2]


class FakeSet:
    """What compile_filters_with_sets reads of a KeySet."""

    def __init__(self, plan, names, has_null=False, closed=False):
        self.plan, self.names, self.has_null, self.closed = plan, list(names), has_null, closed


# ---------------------------------------------------------------------------------------------
# compile_key_values
# ---------------------------------------------------------------------------------------------
def _values(c: K.CompiledKeyValues):
    v = c.values.view(K._VALUE_DTYPE)
    return [(int(x["lo"]), int(x["hi"]), int(x["str_len"])) for x in v]


def test_compile_key_values_numeric_exactness(syn_plan):
    f = syn_plan.fields[_fi(syn_plan, "AMT-01")]
    assert f.out_type == N.O_DEC64 and f.out_scale == 2
    c = K.compile_key_values(syn_plan, ["AMT-01"], [Decimal("1.50"), -3, Decimal("0.001"), Decimal(10) ** f.out_precision, None,
                                                   (Decimal("-0.01"),)])
    m = 2 ** 64 - 1
    assert _values(c) == [(150, 0, 0), ((-300) & m, m, 0), ((-1) & m, m, 0)]
    assert (c.n_values, c.dropped, c.has_null, c.str_stride) == (3, 2, True, 0)
    br = syn_plan.fields[_fi(syn_plan, "BR-ID")]
    bits = 31 if br.out_type == N.O_I32 else 63
    c = K.compile_key_values(syn_plan, ["BR-ID"], [1 << bits, -(1 << bits), Decimal("2.0"), Decimal("2.5")])
    assert c.n_values == 2 and c.dropped == 2 and not c.has_null
    for bad in (1.5, True, "7", Decimal("NaN")):
        with pytest.raises(F.Unhandled):
            K.compile_key_values(syn_plan, ["BR-ID"], [bad])
    assert K.compile_key_values(syn_plan, ["BR-ID"], []).n_values == 0


def test_compile_key_values_strings_and_composites(syn_plan):
    name = syn_plan.fields[_fi(syn_plan, "NAME")]
    c = K.compile_key_values(syn_plan, ["BR-ID", "NAME"], [(5, "AB"), (6, "é"), (7, "x" * (name.size + 1)), (None, "Q"), (8, "")])
    assert c.str_stride == 3 * name.size and c.str_off[:2] == [0, 0]
    assert (c.n_values, c.dropped, c.has_null) == (3, 1, True)
    v = _values(c)
    assert v[0] == (5, 0, 0) and v[1] == (0, 0, 2) and v[3] == (0, 0, 2) and v[5] == (0, 0, 0)
    raw = bytes(c.str_bytes)
    assert raw[:2] == b"AB" and raw[c.str_stride:c.str_stride + 2] == "é".encode()
    with pytest.raises(F.Unhandled, match="str key values"):
        K.compile_key_values(syn_plan, ["NAME"], [5])
    with pytest.raises(ValueError, match="tuples of 2"):
        K.compile_key_values(syn_plan, ["BR-ID", "NAME"], [(5,)])
    c = K.compile_key_values(syn_plan, ["NAME", "BR-ID", "ACCT-NO"], [])
    assert c.str_off[:3] == [0, 3 * name.size, 3 * name.size] and c.table.n_keys == 3


def test_compile_key_values_every_refusal(syn_plan):
    """The refusals of compile_group_by, with its reasons."""
    plan = _plan(WIDE_COPYBOOK)
    for cols, word in ((["ITEM-NO"], "OCCURS"), (["RATE"], "COMP-1 / COMP-2 key"), (["NO-SUCH"], "not found"),
                       (["ITEMS"], "primitive"), (["ID", "ID"], "repeated"), ([], "1 to 4"),
                       (["ID", "BIG", "NAME", "RATE", "ID"], "1 to 4")):
        with pytest.raises(F.Unhandled, match=word):
            K.compile_key_values(plan, cols, [])
    long_plan = _plan("       01  R.\n           05  S32  PIC X(32).\n           05  S33  PIC X(33).\n")
    assert K.compile_key_values(long_plan, ["S32"], ["a"]).n_values == 1
    with pytest.raises(F.Unhandled, match="longer than 32"):
        K.compile_key_values(long_plan, ["S33"], [])
    from cobrix_amd.plan import build_plan
    from cobrix_amd.reader import parse_copybook_for
    cb = parse_copybook_for(WIDE_COPYBOOK, ReaderParameters(variable_size_occurs=True))
    walk = build_plan(cb, walk=True, variable_size_occurs=True, string_views=1)
    with pytest.raises(F.Unhandled, match="data-dependent"):
        K.compile_key_values(walk, ["NAME"], [])
    from test_decode_fuzz import ASCII_COPYBOOK
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    with pytest.raises(F.Unhandled, match="UTF-16"):
        K.compile_key_values(aplan, ["N2"], [])


# ---------------------------------------------------------------------------------------------
# compile_filters_with_sets
# ---------------------------------------------------------------------------------------------
def test_compile_filters_with_sets(syn_plan):
    a, b = FakeSet(syn_plan, ["BR-ID"]), FakeSet(syn_plan, ["BR-ID", "NAME"])
    lt = F.LessThan("BR-ID", 7)
    table, sets, negate, un = F.compile_filters_with_sets(syn_plan, [F.NotInSet(a), F.Not(F.Not(F.InSet(a)))])
    assert not un and table is None and sets == [a, a] and negate == [1, 0]
    table, sets, negate, un = F.compile_filters_with_sets(syn_plan, [lt, F.InSet(b), F.Not(F.InSet(a)), F.Not(F.NotInSet(a))])
    assert not un and table.n_terms == 1 and sets == [b, a, a] and negate == [0, 1, 0]
    # only sets: no table
    table, sets, negate, un = F.compile_filters_with_sets(syn_plan, [F.NotInSet(a)])
    assert table is None and sets == [a] and negate == [1] and not un
    # a top-level And is split, its parts are AND-ed
    table, sets, negate, un = F.compile_filters_with_sets(syn_plan, [F.And(F.InSet(a), F.And(lt, F.Not(F.InSet(a))))])
    assert table.n_terms == 1 and sets == [a, a] and negate == [0, 1] and not un
    # no sets: exactly compile_filters
    t0, u0 = F.compile_filters(syn_plan, [lt, F.IsNull("NO-SUCH")])
    t1, s1, n1, u1 = F.compile_filters_with_sets(syn_plan, [lt, F.IsNull("NO-SUCH")])
    assert bytes(t0) == bytes(t1) and s1 == [] and n1 == [] and list(u0) == list(u1) and u0.reasons == u1.reasons
    assert F.compile_filters_with_sets(syn_plan, None) == (None, [], [], [])


def test_compile_filters_with_sets_every_refusal(syn_plan):
    a, b = FakeSet(syn_plan, ["BR-ID"]), FakeSet(syn_plan, ["BR-ID", "NAME"])
    lt = F.LessThan("BR-ID", 7)
    cases = [(F.Or(F.InSet(a), lt), "under Or"), (F.Not(F.And(F.InSet(a), lt)), "under Or"),
             (F.NotInSet(b), "single-column"), (F.Not(F.InSet(b)), "single-column"),
             (F.NotInSet(FakeSet(syn_plan, ["BR-ID"], has_null=True)), "null"),
             (F.InSet(FakeSet(_plan(SYN200_COPYBOOK), ["BR-ID"])), "another reader's plan")]
    for flt, word in cases:
        table, sets, negate, un = F.compile_filters_with_sets(syn_plan, [lt, flt])
        assert list(un) == [flt] and word in un.reasons[0] and sets == [] and table.n_terms == 1, (flt, un.reasons)
    # InSet over values that held a null is fine (the tuple was dropped: it can never match)
    ok = F.InSet(FakeSet(syn_plan, ["BR-ID"], has_null=True))
    assert F.compile_filters_with_sets(syn_plan, [ok])[1] == [ok.key_set]
    # the fifth set
    five = [F.InSet(FakeSet(syn_plan, ["BR-ID"])) for _ in range(5)]
    table, sets, negate, un = F.compile_filters_with_sets(syn_plan, five)
    assert len(sets) == 4 and list(un) == [five[4]] and "more than 4" in un.reasons[0]
    with pytest.raises(ValueError, match="closed"):
        F.compile_filters_with_sets(syn_plan, [F.InSet(FakeSet(syn_plan, ["BR-ID"], closed=True))])


def test_compile_filters_unchanged_on_in_with_65_values(syn_plan):
    """compile_filters keeps its results: the set classes are not its business, In past the literal table is unhandled."""
    big = F.In("BR-ID", list(range(65)))
    table, un = F.compile_filters(syn_plan, [big, F.LessThan("BR-ID", 7)])
    assert list(un) == [big] and "table limits" in un.reasons[0] and table.n_terms == 1 and table.n_literals == 1
    table, un = F.compile_filters(syn_plan, [F.In("BR-ID", list(range(64)))])
    assert not un and table.n_literals == 64
    s = F.InSet(FakeSet(syn_plan, ["BR-ID"]))
    table, un = F.compile_filters(syn_plan, [s])
    assert table is None and list(un) == [s] and "not a pushed-down filter" in un.reasons[0]


# ---------------------------------------------------------------------------------------------
# ABI structs
# ---------------------------------------------------------------------------------------------
KEYSET_STRUCTS = {"cbx_key_value": N.CbxKeyValue, "cbx_keyset_info": N.CbxKeysetInfo}


def test_keyset_struct_layout_matches_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cobrix_hip.h"', "int main(void) {"]
    for cname, py in KEYSET_STRUCTS.items():
        src.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            src.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    src.append('printf("const CBX_ABI_VERSION %d\\n", (int)CBX_ABI_VERSION);')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    try:
        r = subprocess.run(["gcc", "-I", os.path.dirname(HDR), "-o", str(exe), str(c)], capture_output=True, text=True)
    except OSError as e:  # pragma: no cover
        pytest.skip(f"no C compiler: {e}")
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        cname, what, val = line.split()
        seen += 1
        if cname == "const":
            assert N.ABI_VERSION == int(val) == 25
        else:
            py = KEYSET_STRUCTS[cname]
            got = ctypes.sizeof(py) if what == "sizeof" else getattr(py, what).offset
            assert got == int(val), f"{cname}.{what}: ctypes {got} != C {val}"
    assert seen == 1 + sum(1 + len(py._fields_) for py in KEYSET_STRUCTS.values())
    assert set(N.KEYSET_SYMBOLS) <= set(N.EXPORTED_SYMBOLS)
    assert set(N.KEYSET_SYMBOLS) == {"cbx_key_set_create", "cbx_key_set_info", "cbx_key_set_destroy", "cbx_filter_records_keyed"}
    lib = N.load()
    assert all(hasattr(lib, s) for s in N.KEYSET_SYMBOLS)


# ---------------------------------------------------------------------------------------------
# The host/device part on the host
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("keyset_host") / "libcbx_keyset_host.so"
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-o", str(so), os.path.join(ROOT, "tests", "native", "keyset_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_keyset_create.argtypes = [P, i32, i32, P, P, P, i32, P, i64, ctypes.POINTER(P), ctypes.c_char_p, i32]
    lib.cbxh_keyset_info.argtypes = [P, P]
    lib.cbxh_keyset_info.restype = None
    lib.cbxh_keyset_destroy.argtypes = [P]
    lib.cbxh_keyset_destroy.restype = None
    lib.cbxh_keyset_value_hashes.argtypes = [P, P]
    lib.cbxh_keyset_value_hashes.restype = None
    lib.cbxh_keyset_record_hashes.argtypes = [P, P, P, i64, P, P, P, i64, i32, i32, i32, P, P]
    lib.cbxh_keyset_record_hashes.restype = None
    lib.cbxh_keyset_keep.argtypes = [P, i32, i32, P, P, P, i64, P, P, P, i64, i32, i32, i32, P, P, i32, P, ctypes.c_char_p, i32]
    return lib


class HostError(Exception):
    def __init__(self, rc, reason):
        super().__init__(f"{rc}: {reason}")
        self.rc, self.reason = rc, reason


class HostSet:
    """A key set of the host shim over `names` of `plan`."""

    def __init__(self, lib, plan, names, values, walk=False, raw=None):
        self.lib, self.plan = lib, plan
        c = raw if raw is not None else K.compile_key_values(plan, names, values)
        self.compiled = c
        fields = (N.CbxField * len(plan.fields))(*plan.fields)
        off = (ctypes.c_int32 * 4)(*(list(c.str_off) + [0] * 4)[:4])
        err = ctypes.create_string_buffer(256)
        h = ctypes.c_void_p()
        rc = lib.cbxh_keyset_create(ctypes.addressof(fields), len(plan.fields), int(walk), ctypes.addressof(c.table),
                                    c.values.ctypes.data if c.values.size else None,
                                    c.str_bytes.ctypes.data if c.str_bytes.size else None, c.str_stride,
                                    ctypes.addressof(off), c.n_values, ctypes.byref(h), err, 256)
        if rc != 0:
            raise HostError(rc, err.value.decode())
        self.handle = h

    def info(self) -> N.CbxKeysetInfo:
        out = N.CbxKeysetInfo()
        self.lib.cbxh_keyset_info(self.handle, ctypes.addressof(out))
        return out

    def value_hashes(self) -> np.ndarray:
        out = np.zeros(max(1, self.compiled.n_values), dtype=np.uint64)
        self.lib.cbxh_keyset_value_hashes(self.handle, out.ctypes.data)
        return out[:self.compiled.n_values]

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.cbxh_keyset_destroy(self.handle)
            self.handle = None


def _source(data: bytes, stride, framing, segment=-1):
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    if framing is None:
        return buf, (buf.ctypes.data, len(data), None, None, None, len(data) // stride, stride), ()
    off = np.ascontiguousarray(framing[0], dtype=np.int64)
    ln = np.ascontiguousarray(framing[1], dtype=np.int32)
    seg = np.ascontiguousarray(framing[2], dtype=np.int32) if framing[2] is not None else None
    return buf, (buf.ctypes.data, len(data), off.ctypes.data, ln.ctypes.data, seg.ctypes.data if seg is not None else None,
                 len(off), 0), (off, ln, seg)


def host_record_hashes(hs: HostSet, data: bytes, stride=0, framing=None, start_off=0):
    buf, src, alive = _source(data, stride, framing)
    n = src[5]
    hashes, nulls = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint8)
    hs.lib.cbxh_keyset_record_hashes(hs.handle, ctypes.addressof(hs.plan.options.lut), *src, start_off, -1,
                                     hashes.ctypes.data, nulls.ctypes.data)
    return hashes[:n], nulls[:n].astype(bool)


def host_set_keep(lib, plan, data: bytes, sets, negate, filters=(), stride=0, framing=None, start_off=0) -> np.ndarray:
    """keep[i] of the host shim: the compiled filters, then every HostSet of `sets`."""
    fields = (N.CbxField * len(plan.fields))(*plan.fields)
    flt = _filter_table(plan, filters)
    buf, src, alive = _source(data, stride, framing)
    n = src[5]
    keep = np.zeros(max(1, n), dtype=np.uint8)
    handles = (ctypes.c_void_p * max(1, len(sets)))(*[s.handle for s in sets])
    neg = (ctypes.c_int32 * max(1, len(sets)))(*negate)
    err = ctypes.create_string_buffer(256)
    rc = lib.cbxh_keyset_keep(ctypes.addressof(fields), len(plan.fields), 0, ctypes.addressof(flt) if flt is not None else None,
                              ctypes.addressof(plan.options.lut), *src, start_off, -1, ctypes.addressof(handles),
                              ctypes.addressof(neg), len(sets), keep.ctypes.data, err, 256)
    if rc != 0:
        raise HostError(rc, err.value.decode())
    return keep[:n].astype(bool)


def check_hashes(lib, cb, plan, rows, data, names, stride=0, framing=None, start_off=0):
    """The value-side hash of a row's key equals the record-side hash of the row's record, the record-side null flag is
    the evaluator's; returns the number of non-null rows."""
    keys = distinct_keys(cb, rows, names)
    hs = HostSet(lib, plan, names, keys)
    assert hs.compiled.n_values == len(keys) and hs.compiled.dropped == 0
    vh = dict(zip(keys, hs.value_hashes().tolist()))
    rh, nulls = host_record_hashes(hs, data, stride, framing, start_off)
    assert len(rh) == len(rows)
    seen = 0
    for i, r in enumerate(rows):
        key = tuple(row_value(cb, r, n) for n in names)
        null = any(v is None for v in key)
        assert bool(nulls[i]) == null, (names, i, key)
        if not null:
            assert int(rh[i]) == vh[key], (names, i, key)
            seen += 1
    info = hs.info()
    assert info.n_distinct == len(keys) and info.n_values == len(keys)
    return seen


def check_keep(lib, cb, plan, rows, data, specs, filters=(), permute=True, **src):
    """specs: (names, values, negate).  The host shim's keep flags equal the evaluator's; returns them."""
    exp = expected_set_keep(cb, rows, filters, specs)
    sets = [HostSet(lib, plan, names, values) for names, values, _ in specs]
    got = host_set_keep(lib, plan, data, sets, [int(ng) for _, _, ng in specs], filters, **src)
    assert np.array_equal(got, exp), (specs[0][0], np.flatnonzero(got != exp)[:8])
    if permute:   # the value order does not matter
        sets2 = [HostSet(lib, plan, names, list(reversed(list(values))), ) for names, values, _ in specs]
        assert np.array_equal(host_set_keep(lib, plan, data, sets2, [int(ng) for _, _, ng in specs], filters, **src), exp)
    return exp


@pytest.mark.parametrize("names", [["BR-ID"], ["ZD-01"], ["AMT-01"], ["NAME"], ["BR-ID", "NAME"], ["ZD-01", "AMT-01", "NAME", "ACCT-NO"]])
def test_host_syn200(host_shim, syn_plan, syn_rows, names):
    """2,000 SYN200 records, a fifth of the numeric fields malformed: the hashes agree, IN / NOT IN equal the evaluator."""
    cb, data, rows = syn_rows
    assert check_hashes(host_shim, cb, syn_plan, rows, data, names, stride=200) > 100
    keys = distinct_keys(cb, rows, names)
    absent = [tuple(99999 if not isinstance(v, str) else "~none~" for v in keys[0])]
    vals = half(keys) + absent
    for filters in ([], [F.IsNotNull("QTY-01")]):
        exp = check_keep(host_shim, cb, syn_plan, rows, data, [(names, vals, 0)], filters, stride=200)
        assert 0 < exp.sum() < len(rows)
        if len(names) == 1:
            exp2 = check_keep(host_shim, cb, syn_plan, rows, data, [(names, vals, 1)], filters, stride=200)
            assert not (exp & exp2).any()
            if names == ["ZD-01"] and not filters:   # null keys are kept by neither form
                assert (exp | exp2).sum() < len(rows)


def test_host_two_sets_and_a_filter(host_shim, syn_plan, syn_rows):
    cb, data, rows = syn_rows
    a, b = distinct_keys(cb, rows, ["BR-ID"]), distinct_keys(cb, rows, ["NAME"])
    specs = [(["BR-ID"], a[: 2 * len(a) // 3], 0), (["NAME"], half(b), 1)]
    for filters in ([], [F.GreaterThan("AMT-01", Decimal("0"))]):
        exp = check_keep(host_shim, cb, syn_plan, rows, data, specs, filters, stride=200)
        assert 0 < exp.sum() < len(rows)


@pytest.mark.parametrize("start,end", [(0, 0), (3, 2)])
@pytest.mark.parametrize("code_page,trim", FUZZ_OPTIONS)
def test_host_every_key_kind_ebcdic(host_shim, code_page, trim, start, end):
    from oracle import reader_oracle as RO
    from test_decode_fuzz import FUZZ_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim,
                         start_offset=start, end_offset=end)
    cb, plan = reader_plan(FUZZ_COPYBOOK, p)
    data = fuzz_records(cb, FUZZ_N, 31, start, end)
    rows = RO.fixed_len_rows(cb, data, p)
    stride = cb.record_size + start + end
    by_kind = _key_candidates(plan, cb)
    assert {k for k, _ in by_kind} >= {N.K_STRING, N.K_BCD, N.K_BINARY, N.K_ZONED}
    for cols in by_kind.values():
        for names in ([cols[0]], cols[-2:]):
            check_hashes(host_shim, cb, plan, rows, data, names, stride=stride, start_off=start)
            keys = distinct_keys(cb, rows, names)
            check_keep(host_shim, cb, plan, rows, data, [(names, half(keys), 0)], permute=False, stride=stride, start_off=start)
            if len(names) == 1:
                check_keep(host_shim, cb, plan, rows, data, [(names, half(keys), 1)], permute=False, stride=stride, start_off=start)


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_host_every_key_kind_ascii(host_shim, charset):
    from oracle import reader_oracle as RO
    from test_decode_fuzz import ASCII_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
    cb, plan = reader_plan(ASCII_COPYBOOK, p)
    data = ascii_records(cb, FUZZ_N, 32)
    rows = RO.fixed_len_rows(cb, data, p)
    by_kind = _key_candidates(plan, cb)
    assert {k for k, _ in by_kind} >= {N.K_STRING if charset else N.K_STRING_ASCII, N.K_ASCII_NUM}
    for cols in by_kind.values():
        names = cols[:1]
        check_hashes(host_shim, cb, plan, rows, data, names, stride=cb.record_size)
        keys = distinct_keys(cb, rows, names)
        for neg in (0, 1):
            check_keep(host_shim, cb, plan, rows, data, [(names, half(keys), neg)], permute=False, stride=cb.record_size)


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_width_ladder_cut_at_every_length(host_shim, trim):
    """One record per length: a string key starting past the record's end is NULL (kept by neither form), one that
    starts at its end is "" (a value like any other); a numeric key the record ends inside is NULL."""
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    raw, off, ln = ladder_file(seed=34, every_length=True)
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == len(off)
    framing = (off, ln, None)
    for names in (["X05"], ["X32"], ["X01"], ["X12"], ["P05"], ["Z07"], ["X03", "P03"]):
        check_hashes(host_shim, cb, plan, rows, raw, names, framing=framing)
        keys = distinct_keys(cb, rows, names)
        check_keep(host_shim, cb, plan, rows, raw, [(names, half(keys), 0)], framing=framing)
        if len(names) == 1:
            check_keep(host_shim, cb, plan, rows, raw, [(names, half(keys), 1)], framing=framing)
    # "" is a member when given, NULL never is: NOT IN of the empty set keeps exactly the non-null rows
    vals = [row_value(cb, r, "X05") for r in rows]
    assert None in vals and "" in vals
    exp = check_keep(host_shim, cb, plan, rows, raw, [(["X05"], [""], 0)], framing=framing)
    assert exp.sum() == vals.count("")
    exp = check_keep(host_shim, cb, plan, rows, raw, [(["X05"], [], 1)], framing=framing)
    assert exp.sum() == len(vals) - vals.count(None)


def test_host_segment_redefines(host_shim):
    """RDW_NARROW with its redefine map: a key in the inactive redefine is NULL."""
    from cobrix_amd.synth import RDW_NARROW_COPYBOOK
    from oracle import oracle as O
    from oracle import reader_oracle as RO
    p = narrow_params()
    cb, plan = reader_plan(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(300, 21)
    off, ln = O.frame_rdw(raw)
    recs = RO.var_len_records(cb, raw, p)
    rows = RO.var_len_rows(cb, raw, p)
    groups = [g.name.upper() for g in plan.segment_groups]
    seg = np.array([groups.index(r.active_segment.upper()) if r.active_segment is not None else -1 for r in recs],
                   dtype=np.int32)
    framing = (off, ln, seg)
    for names in (["SEGMENT-ID"], ["TAXPAYER-TYPE"], ["TAXPAYER-NUM"], ["SEGMENT-ID", "TAXPAYER-TYPE"]):
        keys = distinct_keys(cb, rows, names)
        exp = check_keep(host_shim, cb, plan, rows, raw, [(names, half(keys), 0)], framing=framing)
        assert exp.any()
        if len(names) == 1:
            check_keep(host_shim, cb, plan, rows, raw, [(names, half(keys), 1)], framing=framing)
    none = sum(row_value(cb, r, "TAXPAYER-TYPE") is None for r in rows)
    exp = check_keep(host_shim, cb, plan, rows, raw, [(["TAXPAYER-TYPE"], [], 1)], framing=framing)
    assert none > 0 and exp.sum() == len(rows) - none


@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
def test_host_equal_values_of_different_bytes_are_one_member(host_shim, trim):
    """The copybook of test_group.py: the sign nibbles of a COMP-3 zero, overpunch spellings, padding and code-page twins."""
    from oracle import reader_oracle as RO
    p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=trim)
    cb, plan = reader_plan(EQUAL_COPYBOOK, p)
    data = equal_records(plan)
    rows = RO.fixed_len_rows(cb, data, p)
    for names in (["KB"], ["KP"], ["KZ"], ["KX4"], ["KX3"], ["KB", "KP", "KX4", "KX3"], ["KZ", "KX3"]):
        check_hashes(host_shim, cb, plan, rows, data, names, stride=EQUAL_SIZE)
        keys = distinct_keys(cb, rows, names)
        for vals in (half(keys), keys[:1], keys):
            check_keep(host_shim, cb, plan, rows, data, [(names, vals, 0)], permute=False, stride=EQUAL_SIZE)
            if len(names) == 1:
                check_keep(host_shim, cb, plan, rows, data, [(names, vals, 1)], permute=False, stride=EQUAL_SIZE)


def test_host_wrap_around_duplicates_and_the_empty_set(host_shim, syn_plan, syn_rows):
    cb, data, rows = syn_rows
    # 8 values whose home slot is the last of the 16: the probe sequences wrap to slot 0 and reach 8 slots
    cands = list(range(1, 4000))
    hs = HostSet(host_shim, syn_plan, ["BR-ID"], cands)
    home = [v for v, h in zip(cands, hs.value_hashes().tolist()) if h & 15 == 15]
    assert len(home) >= 8
    present = {row_value(cb, r, "BR-ID") for r in rows}
    pick = [v for v in home if v in present][:4] + [v for v in home if v not in present]
    pick = pick[:8]
    wrap = HostSet(host_shim, syn_plan, ["BR-ID"], pick)
    info = wrap.info()
    assert (info.capacity, info.n_distinct) == (16, 8) and info.max_probe >= 8
    for neg in (0, 1):
        check_keep(host_shim, cb, syn_plan, rows, data, [(["BR-ID"], pick, neg)], stride=200)
    # 1,000 copies of one value
    dup = HostSet(host_shim, syn_plan, ["BR-ID", "NAME"], [(7, "SAME")] * 1000)
    info = dup.info()
    assert (info.n_values, info.n_distinct, info.capacity) == (1000, 1, 2048)
    # the empty set
    empty = HostSet(host_shim, syn_plan, ["ZD-01"], [])
    assert (empty.info().n_values, empty.info().n_distinct, empty.info().capacity, empty.info().max_probe) == (0, 0, 2, 0)
    exp = check_keep(host_shim, cb, syn_plan, rows, data, [(["ZD-01"], [], 0)], stride=200)
    assert not exp.any()
    exp = check_keep(host_shim, cb, syn_plan, rows, data, [(["ZD-01"], [], 1)], stride=200)
    nulls = sum(row_value(cb, r, "ZD-01") is None for r in rows)
    assert nulls > 0 and exp.sum() == len(rows) - nulls


def test_keyset_layout_refusals(host_shim, syn_plan):
    name = syn_plan.fields[_fi(syn_plan, "NAME")]

    def raw(names, values, **change):
        c = K.compile_key_values(syn_plan, names, values)
        for k, v in change.items():
            setattr(c, k, v)
        return c

    def status(c, walk=False, plan=syn_plan):
        try:
            HostSet(host_shim, plan, None, None, walk=walk, raw=c)
        except HostError as e:
            return e.rc, e.reason
        return 0, ""

    assert status(raw(["BR-ID", "NAME"], [(1, "A")]))[0] == 0
    c = raw(["NAME"], ["AB"])
    c.values.view(K._VALUE_DTYPE)["str_len"][0] = 3 * name.size + 1
    rc, err = status(c)
    assert rc == N.CBX_E_ARGUMENT and "str_len" in err
    c = raw(["NAME"], ["AB"])
    c.values.view(K._VALUE_DTYPE)["str_len"][0] = -1
    assert status(c)[0] == N.CBX_E_ARGUMENT
    for change, word in (({"n_values": -1}, "negative"), ({"str_stride": 3 * name.size + 1}, "str_stride"),
                         ({"str_off": [3, 0, 0, 0]}, "str_off"), ({"n_values": 1 << 40}, "workspace")):
        rc, err = status(raw(["NAME"], ["AB"], **change))
        assert rc == N.CBX_E_ARGUMENT and word in err, (change, rc, err)
    for fields, n_keys, word in (([_fi(syn_plan, "BR-ID")] * 2, 2, "repeated"), ([99], 1, "out of range"), ([], 0, "1 to 4"),
                                 ([0] * 4, 5, "1 to 4")):
        c = raw(["BR-ID"], [])
        c.table.n_keys = n_keys
        for i, fi in enumerate(fields):
            c.table.fields[i] = fi
        rc, err = status(c)
        assert rc == N.CBX_E_ARGUMENT and word in err, (fields, rc, err)
    wide = _plan(WIDE_COPYBOOK)
    for col, walk, word in (("ITEM-NO", False, "OCCURS"), ("RATE", False, "COMP-1 / COMP-2 key"), ("NAME", True, "data-dependent")):
        c = raw(["BR-ID"], [])
        c.table.fields[0] = _fi(wide, col)
        rc, err = status(c, walk=walk, plan=wide)
        assert rc == N.CBX_E_UNSUPPORTED and word in err, (col, rc, err)


# ---------------------------------------------------------------------------------------------
# The stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [["BR-ID"], ["NAME"], ["ZD-01", "NAME", "AMT-01"]])
def test_host_program_under_the_sanitizers(tmp_path_factory, syn_plan, syn_rows, names):
    """tests/native/keyset_host_main.cpp built with -fsanitize=address,undefined over exact-size heap buffers: the fixed
    run and a framed run that cuts the records inside and in front of the key fields.  A subprocess of its own: nothing
    loaded into Python runs under a sanitizer."""
    cb, data, rows = syn_rows
    n = 500
    exe = tmp_path_factory.getbasetemp() / "keyset_host_check"
    if not exe.exists():
        r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "native", "keyset_host_main.cpp")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    keys = distinct_keys(cb, rows[:n], names)
    vals = half(keys) + half(keys)[:5]          # with duplicates
    c = K.compile_key_values(syn_plan, names, vals)
    head = struct.pack("<4i2q4i4i", len(syn_plan.fields), 200, len(names), c.str_stride, n, c.n_values,
                       *(list(c.table.fields)[:4]), *((list(c.str_off) + [0] * 4)[:4]))
    case = tmp_path_factory.mktemp("ks_case") / "case.bin"
    fields = (N.CbxField * len(syn_plan.fields))(*syn_plan.fields)
    case.write_bytes(head + bytes(fields) + bytes(syn_plan.options.lut) + data[:200 * n] + c.values.tobytes() + c.str_bytes.tobytes())
    r = subprocess.run([str(exe), str(case)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-4000:], r.stdout)
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert lines[0][:3] == ["set", "distinct", str(len(half(keys)))]
    # the framed run's records, cut as the program cuts them, through the oracle's variable-length reader
    from cobrix_amd.reader import parse_copybook_for
    from cobrix_amd.synth import rdw_file
    from oracle import reader_oracle as RO
    blob = data[:200 * n]
    cuts = [(200 * i, (7 * i) % 200 + 1) for i in range(n)]
    for back in range(1, 201):
        cuts[n - back] = (len(blob) - back, back)
    vp = ReaderParameters(is_record_sequence=True, schema_policy="collapse_root")
    vcb = parse_copybook_for(SYN200_COPYBOOK, vp)
    cut_rows = RO.var_len_rows(vcb, rdw_file([blob[o:o + ln] for o, ln in cuts]), vp)
    assert len(cut_rows) == n
    forms = (0, 1) if len(names) == 1 else (0,)
    want = [["fixed", "not_in" if neg else "in", "kept", str(expected_set_keep(cb, rows[:n], [], [(names, vals, neg)]).sum())]
            for neg in forms]
    want += [["framed", "not_in" if neg else "in", "kept", str(expected_set_keep(vcb, cut_rows, [], [(names, vals, neg)]).sum())]
             for neg in forms]
    assert lines[1:] == want
    assert 0 < int(want[-1][3]) < n
