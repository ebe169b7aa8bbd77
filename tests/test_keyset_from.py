"""Key sets built from a second file's records (cbx_key_set_create_from_records), the parts that need no GPU: the new
ABI struct's layout, compile_key_pairs with every refusal, and the host/device part of cobrix_amd/csrc/cbx_keyset_from.h
(the compatibility rules and bounds, find-or-claim on bare slot words, the conversion rule) run on the host
(tests/native/keyset_from_host.cpp) in front of the key-set shim, against a Python model.

The model (`model_of`) takes the oracle's rows only: `distinct_keys` of the source rows the source filters keep, then
the drop rules written here from the contract (`can_hold`), then `expected_set_keep` over the probe rows.  It never
uses the code under test.  The GPU tests (test_gpu_keyset_from.py) use the same one, and the dimension copybook below.
"""
from __future__ import annotations

import ctypes
import decimal
import os
import random
import struct
import subprocess
from dataclasses import dataclass
from decimal import Decimal
from typing import Any, List

import numpy as np
import pytest

from cobrix_amd import filter as F
from cobrix_amd import keyset as K
from cobrix_amd import native as N
from cobrix_amd.reader import ReaderParameters, parse_copybook_for
from cobrix_amd.synth import SYN200_COPYBOOK, rdw_file, syn200
from test_aggregate import _filter_table, _fi
from test_filter import (FUZZ_N, FUZZ_OPTIONS, LADDER_COPYBOOK, WIDE_COPYBOOK, ascii_records, fuzz_records, ladder_file,
                         ladder_params, narrow_file, narrow_params, py_keep, reader_plan, row_value)
from test_group import EQUAL_COPYBOOK, EQUAL_SIZE, _hipcc, _key_candidates, _plan, equal_records
from test_keyset import HostError, _source, distinct_keys, expected_set_keep, host_set_keep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")


# ---------------------------------------------------------------------------------------------
# The contract over decoded rows
# ---------------------------------------------------------------------------------------------
def can_hold(f: N.CbxField, v) -> bool:
    """Can probe column f ever hold key value v?  (The issue's drop rules: |v| < 10^precision for a decimal column, the
    signed 32- / 64-bit range for an integer one, at most the field's size in characters and 3 x that in UTF-8 bytes.)"""
    if isinstance(v, str):
        return len(v) <= f.size and len(v.encode("utf-8")) <= 3 * f.size
    dec = f.out_type in (N.O_DEC64, N.O_DEC128)
    with decimal.localcontext() as ctx:
        ctx.prec = 100
        u = Decimal(v).scaleb(f.out_scale if dec else 0)
        assert u == u.to_integral_value(), (v, f.out_scale)   # (equal scales: nothing is rescaled)
        u = int(u)
    if dec:
        return abs(u) < 10 ** f.out_precision
    bits = 31 if f.out_type == N.O_I32 else 63
    return -(1 << bits) <= u < (1 << bits)


@dataclass
class Model:
    n_rows: int
    n_null_rows: int
    n_source_keys: int
    n_dropped: int
    values: List[Any]          # the members: tuples

    def counts(self):
        return self.n_rows, self.n_null_rows, self.n_source_keys, self.n_dropped


def model_of(scb, srows, source_names, pplan, names, filters=()) -> Model:
    kept = [r for r in srows if py_keep(scb, r, filters)] if filters else list(srows)
    nulls = sum(any(row_value(scb, r, c) is None for c in source_names) for r in kept)
    keys = distinct_keys(scb, kept, source_names)
    fields = [pplan.fields[_fi(pplan, c)] for c in names]
    values = [k for k in keys if all(can_hold(f, v) for f, v in zip(fields, k))]
    return Model(len(kept), nulls, len(keys), len(keys) - len(values), values)


def counts_of(info: N.CbxKeysetSourceInfo):
    return info.n_rows, info.n_null_rows, info.n_source_keys, info.n_dropped


# ---------------------------------------------------------------------------------------------
# A dimension file whose keys are encoded differently from SYN200's
# ---------------------------------------------------------------------------------------------
DIM_COPYBOOK = """
       01  DIM-REC.
           05  D-BR      PIC S9(5) COMP-3.
           05  D-ACCT    PIC S9(18).
           05  D-AMT     PIC S9(7)V99 COMP-3.
           05  D-NAME    PIC X(24).
           05  D-BIG     PIC S9(20) COMP-3.
           05  D-RATE    PIC S9(5)V999 COMP-3.
"""
DIM_SIZE = 3 + 18 + 5 + 24 + 11 + 5
DIM_PAIRS = {"D-BR": "BR-ID", "D-ACCT": "ACCT-NO", "D-AMT": "AMT-01", "D-NAME": "NAME", "D-BIG": "ACCT-NO"}


def _bcd(v: int, size: int) -> bytes:
    nib = [int(c) for c in str(abs(v)).rjust(2 * size - 1, "0")] + [0xD if v < 0 else (0xC, 0xF)[abs(v) % 2]]
    return bytes((nib[2 * j] << 4) | nib[2 * j + 1] for j in range(size))


def _zoned(v: int, size: int) -> bytes:
    b = bytearray(0xF0 | int(c) for c in str(abs(v)).rjust(size, "0"))
    b[-1] = ((0xD if v < 0 else 0xC) << 4) | (b[-1] & 0x0F)
    return bytes(b)


def dim_records(n: int, seed: int, pool_cb, pool_rows, malformed_rate: float = 0.2, match: float = 0.5, tall: float = 0.1) -> bytes:
    """n DIM records.  With probability `match` a record takes its key fields from the paired SYN200 columns of one
    random row of the pool (each where the DIM field can spell the value), else fresh values of its own; `tall` of the fresh
    D-BIG values lie beyond 63 bits and of the fresh names are longer than 18 characters; `malformed_rate` of the
    numeric fields are malformed (null).  Names are cp037 with padding on either side."""
    rng = random.Random(seed)
    out = bytearray()

    row = None

    def pooled(col):
        return row_value(pool_cb, row, col) if row is not None else None

    for _ in range(n):
        row = pool_rows[rng.randrange(len(pool_rows))] if pool_rows and rng.random() < match else None
        br = pooled("BR-ID")
        br = br if br is not None else rng.randrange(-99999, 100000)
        acct = pooled("ACCT-NO")
        if acct is None or abs(acct) >= 10 ** 18:
            acct = rng.randrange(-(10 ** 18) + 1, 10 ** 18)
        amt = pooled("AMT-01")
        amt = int(Decimal(amt).scaleb(2)) if amt is not None else None
        if amt is None or abs(amt) >= 10 ** 9:
            amt = rng.randrange(-(10 ** 9) + 1, 10 ** 9)
        name = pooled("NAME")
        if name is None:
            name = "".join(rng.choice("ABCXYZ019") for _ in range(rng.randrange(19, 25) if rng.random() < tall else rng.randrange(0, 5)))
        big = pooled("ACCT-NO")
        if big is None:
            big = rng.randrange(2 ** 63, 10 ** 20) * rng.choice((1, -1)) if rng.random() < tall else rng.randrange(-50, 50)
        rate = rng.randrange(-(10 ** 8) + 1, 10 ** 8)
        lead = rng.randrange(0, 24 - len(name) + 1) if rng.random() < 0.3 else 0
        text = (" " * lead + name).ljust(24).encode("cp037")
        parts = [_bcd(br, 3), _zoned(acct, 18), _bcd(amt, 5), text, _bcd(big, 11), _bcd(rate, 5)]
        for k in (0, 1, 2, 4, 5):
            if rng.random() < malformed_rate:
                bad = bytearray(parts[k])
                bad[rng.randrange(len(bad) - 1) if len(bad) > 1 else 0] = 0x5B if k == 1 else 0xAB
                parts[k] = bytes(bad)
        out += b"".join(parts)
    assert len(out) == n * DIM_SIZE
    return bytes(out)


DIM_PARAMS = ReaderParameters(schema_policy="collapse_root")
AMT_01_OFFSET = 4 + 2 + 8 + 4


def probe_records(n: int = 321, seed: int = 11) -> bytes:
    """n SYN200 records, a fifth of the numeric fields malformed; every third record's AMT-01 (13 random digits in the
    generator) is a value of at most 9 digits, which D-AMT (S9(7)V99) can spell too."""
    data = bytearray(syn200(n, seed=seed, malformed_rate=0.2).numpy().tobytes())
    rng = random.Random(seed)
    for i in range(0, n, 3):
        data[200 * i + AMT_01_OFFSET:200 * i + AMT_01_OFFSET + 8] = _bcd(rng.randrange(-(10 ** 9) + 1, 10 ** 9), 8)
    return bytes(data)


@pytest.fixture(scope="module")
def syn():
    """(copybook, plan, data of 321 SYN200 records a fifth malformed, oracle rows) -- the probe side."""
    from oracle import reader_oracle as RO
    cb, plan = reader_plan(SYN200_COPYBOOK, DIM_PARAMS)
    data = probe_records()
    return cb, plan, data, RO.fixed_len_rows(cb, data, DIM_PARAMS)


@pytest.fixture(scope="module")
def dim(syn):
    """(copybook, plan, data of 321 DIM records drawn from the probe rows, oracle rows) -- the source side."""
    from oracle import reader_oracle as RO
    cb, plan = reader_plan(DIM_COPYBOOK, DIM_PARAMS)
    assert cb.record_size == DIM_SIZE
    data = dim_records(321, 7, syn[0], syn[3])
    return cb, plan, data, RO.fixed_len_rows(cb, data, DIM_PARAMS)


# ---------------------------------------------------------------------------------------------
# compile_key_pairs
# ---------------------------------------------------------------------------------------------
def test_compile_key_pairs_accepts_different_encodings(syn, dim):
    _, splan = dim[0], dim[1]
    pplan = syn[1]
    for s, p in DIM_PAIRS.items():
        pt, st = K.compile_key_pairs(pplan, [p], splan, [s])
        assert pt.n_keys == st.n_keys == 1 and pt.fields[0] == _fi(pplan, p) and st.fields[0] == _fi(splan, s)
    pt, st = K.compile_key_pairs(pplan, ["BR-ID", "NAME", "AMT-01", "ACCT-NO"], splan, ["D-BR", "D-NAME", "D-AMT", "D-BIG"])
    assert pt.n_keys == st.n_keys == 4
    # an integral column is scale 0, whatever its encoding and output type
    assert splan.fields[_fi(splan, "D-BIG")].out_type == N.O_DEC128 and pplan.fields[_fi(pplan, "ACCT-NO")].out_type == N.O_I64


def test_compile_key_pairs_every_refusal(syn, dim):
    pplan, splan = syn[1], dim[1]
    for names, snames, word in ((["BR-ID", "NAME"], ["D-BR"], "2 probe key columns against 1 source key columns"),
                                (["NAME"], ["D-BR"], "key 0: a string column against a numeric one"),
                                (["BR-ID", "BR-ID"], ["D-BR", "D-NAME"], "probe: BR-ID: key column repeated"),
                                (["ACCT-NO", "BR-ID"], ["D-BIG", "D-NAME"], "key 1: a string column against a numeric one"),
                                (["AMT-01"], ["D-RATE"], "key 0: scales 2 and 3 differ"),
                                (["BR-ID"], ["D-AMT"], "key 0: scales 0 and 2 differ"),
                                (["FX-RATE"], ["D-BR"], "probe: FX-RATE: COMP-1 / COMP-2 key"),
                                (["NO-SUCH"], ["D-BR"], "probe: "), (["BR-ID"], ["NO-SUCH"], "source: "),
                                ([], [], "probe: GROUP BY takes 1 to 4"), (["BR-ID"], [], "source: GROUP BY takes 1 to 4")):
        with pytest.raises(F.Unhandled) as e:
            K.compile_key_pairs(pplan, names, splan, snames)
        assert word in str(e.value), (names, snames, str(e.value))
    # each refusal of compile_group_by on each side
    wide = _plan(WIDE_COPYBOOK)
    long_plan = _plan("       01  R.\n           05  S32  PIC X(32).\n           05  S33  PIC X(33).\n")
    from cobrix_amd.plan import build_plan
    from test_decode_fuzz import ASCII_COPYBOOK
    walk = build_plan(parse_copybook_for(WIDE_COPYBOOK, ReaderParameters(variable_size_occurs=True)), walk=True,
                      variable_size_occurs=True, string_views=1)
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    for plan, col, word in ((wide, "ITEM-NO", "OCCURS"), (wide, "RATE", "COMP-1 / COMP-2 key"), (long_plan, "S33", "longer than 32"),
                            (walk, "NAME", "data-dependent"), (aplan, "N2", "UTF-16"), (wide, "ITEMS", "primitive")):
        with pytest.raises(F.Unhandled, match="^probe: .*" + word):
            K.compile_key_pairs(plan, [col], pplan, ["BR-ID"])
        with pytest.raises(F.Unhandled, match="^source: .*" + word):
            K.compile_key_pairs(pplan, ["BR-ID"], plan, [col])
    assert K.compile_key_pairs(long_plan, ["S32"], pplan, ["NAME"])[0].n_keys == 1


# ---------------------------------------------------------------------------------------------
# ABI struct
# ---------------------------------------------------------------------------------------------
KEYSET_FROM_STRUCTS = {"cbx_keyset_source_info": N.CbxKeysetSourceInfo}


def test_keyset_from_struct_layout_matches_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cobrix_hip.h"', "int main(void) {"]
    for cname, py in KEYSET_FROM_STRUCTS.items():
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
            py = KEYSET_FROM_STRUCTS[cname]
            got = ctypes.sizeof(py) if what == "sizeof" else getattr(py, what).offset
            assert got == int(val), f"{cname}.{what}: ctypes {got} != C {val}"
    assert seen == 1 + sum(1 + len(py._fields_) for py in KEYSET_FROM_STRUCTS.values())
    assert N.KEYSET_FROM_SYMBOLS == ("cbx_key_set_create_from_records",) and set(N.KEYSET_FROM_SYMBOLS) <= set(N.EXPORTED_SYMBOLS)
    lib = N.load()
    assert all(hasattr(lib, s) for s in N.KEYSET_FROM_SYMBOLS)
    assert hasattr(K.KeySet, "from_records") and callable(K.compile_key_pairs)


# ---------------------------------------------------------------------------------------------
# The host/device part on the host
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("keyset_from_host") / "libcbx_keyset_from_host.so"
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(so),
                        os.path.join(ROOT, "tests", "native", "keyset_from_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(str(so))
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.cbxh_keyset_from_records.argtypes = [P, i32, i32, P, P, i32, i32, P, P, P, P, i64, P, P, P, i64, i32, i32, i32, i64,
                                             ctypes.POINTER(P), P, ctypes.c_char_p, i32]
    lib.cbxh_keyset_info.argtypes = [P, P]
    lib.cbxh_keyset_info.restype = None
    lib.cbxh_keyset_destroy.argtypes = [P]
    lib.cbxh_keyset_destroy.restype = None
    lib.cbxh_keyset_keep.argtypes = [P, i32, i32, P, P, P, i64, P, P, P, i64, i32, i32, i32, P, P, i32, P, ctypes.c_char_p, i32]
    return lib


class HostFromSet:
    """A set of `pplan` over `names` the host shim builds from the `source_names` keys of a source's records; what
    test_keyset.host_set_keep takes as a set."""

    def __init__(self, lib, pplan, names, splan, source_names, data: bytes, filters=(), stride=0, framing=None, start_off=0,
                 max_values=65536, tables=None, p_walk=False, s_walk=False):
        self.lib, self.plan = lib, pplan
        if tables is None:
            pt, st = K.compile_key_pairs(pplan, names, splan, source_names)
        else:
            pt, st = tables
        pf = (N.CbxField * len(pplan.fields))(*pplan.fields)
        sf = (N.CbxField * len(splan.fields))(*splan.fields)
        flt = _filter_table(splan, filters)
        buf, src, alive = _source(data, stride, framing)
        self.source_info = N.CbxKeysetSourceInfo()
        err = ctypes.create_string_buffer(256)
        h = ctypes.c_void_p()
        self.handle = None
        rc = lib.cbxh_keyset_from_records(ctypes.addressof(pf), len(pplan.fields), int(p_walk), ctypes.addressof(pt),
                                          ctypes.addressof(sf), len(splan.fields), int(s_walk), ctypes.addressof(st),
                                          ctypes.addressof(flt) if flt is not None else None, ctypes.addressof(splan.options.lut),
                                          *src, start_off, -1, max_values, ctypes.byref(h), ctypes.addressof(self.source_info),
                                          err, 256)
        if rc != 0:
            raise HostError(rc, err.value.decode())
        self.handle = h

    def info(self) -> N.CbxKeysetInfo:
        out = N.CbxKeysetInfo()
        self.lib.cbxh_keyset_info(self.handle, ctypes.addressof(out))
        return out

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.cbxh_keyset_destroy(self.handle)
            self.handle = None


def check_from(lib, probe, names, source, source_names, filters=(), probe_src=None, source_src=None) -> np.ndarray:
    """probe / source: (copybook, plan, data, rows).  The counts of the host shim's build equal the model's, and the
    keep flags over the probe records equal expected_set_keep with the model's values, for IN and (one column) NOT IN.
    Returns the IN flags."""
    pcb, pplan, pdata, prows = probe
    scb, splan, sdata, srows = source
    probe_src = probe_src or dict(stride=len(pdata) // len(prows))
    source_src = source_src or dict(stride=len(sdata) // len(srows))
    m = model_of(scb, srows, source_names, pplan, names, filters)
    hs = HostFromSet(lib, pplan, names, splan, source_names, sdata, filters, **source_src)
    assert counts_of(hs.source_info) == m.counts(), (names, source_names, counts_of(hs.source_info), m.counts())
    info = hs.info()
    assert (info.n_values, info.n_distinct) == (len(m.values), len(m.values))
    set_cap = 2
    while set_cap < 2 * len(m.values):
        set_cap <<= 1
    assert info.capacity == set_cap
    cap = 2
    while cap < 2 * 65536:
        cap <<= 1
    assert hs.source_info.source_capacity == cap and not hs.source_info.overflow
    first = None
    for neg in ((0, 1) if len(names) == 1 else (0,)):
        exp = expected_set_keep(pcb, prows, [], [(names, m.values, neg)])
        got = host_set_keep(lib, pplan, pdata, [hs], [neg], **probe_src)
        assert np.array_equal(got, exp), (names, neg, np.flatnonzero(got != exp)[:8])
        first = exp if first is None else first
    return first


@pytest.mark.parametrize("snames,names", [(["D-BR"], ["BR-ID"]), (["D-ACCT"], ["ACCT-NO"]), (["D-AMT"], ["AMT-01"]),
                                          (["D-NAME"], ["NAME"]), (["D-BIG"], ["ACCT-NO"]),
                                          (["D-BR", "D-NAME", "D-AMT", "D-BIG"], ["BR-ID", "NAME", "AMT-01", "ACCT-NO"])])
def test_host_dimension_against_syn200(host_shim, syn, dim, snames, names):
    """Keys spelt differently on the two sides (COMP-3 / binary, zoned / binary, X(24) / X(18), S9(20) / int64) join on
    the decoded value; nulls are counted and never join; what the probe column cannot hold is dropped and counted."""
    for filters in ([], [F.IsNotNull("D-RATE")], [F.GreaterThan("D-BR", 0), F.LessThan("D-AMT", Decimal("5000000.00"))]):
        exp = check_from(host_shim, syn, names, dim, snames, filters)
        assert 0 < exp.sum() < len(exp), (snames, filters)
    m = model_of(dim[0], dim[3], snames, syn[1], names)
    assert m.n_null_rows > 0 or snames == ["D-NAME"]   # (a string of a whole record is never null)
    if snames in (["D-NAME"], ["D-BIG"]):
        assert m.n_dropped > 0
    # the source keys of the same file under its own columns: every non-null probe row joins
    exp = check_from(host_shim, dim, snames, dim, snames)
    assert exp.sum() == len(dim[3]) - m.n_null_rows


def test_host_record_counts_and_no_rows(host_shim, syn, dim):
    scb, splan, sdata, srows = dim
    for n in (0, 1, 63, 64, 65):
        part = (scb, splan, sdata[:DIM_SIZE * n], srows[:n])
        if n:
            check_from(host_shim, syn, ["BR-ID"], part, ["D-BR"])
        else:
            hs = HostFromSet(host_shim, syn[1], ["BR-ID"], splan, ["D-BR"], b"", stride=DIM_SIZE)
            assert counts_of(hs.source_info) == (0, 0, 0, 0) and hs.info().n_values == 0
            assert not host_set_keep(host_shim, syn[1], syn[2], [hs], [0], stride=200).any()
    # a source filter that keeps no row
    hs = HostFromSet(host_shim, syn[1], ["BR-ID"], splan, ["D-BR"], sdata, [F.GreaterThan("D-BR", 10 ** 6)], stride=DIM_SIZE)
    assert counts_of(hs.source_info) == (0, 0, 0, 0) and hs.info().n_distinct == 0


def test_host_max_values_exact_and_one_less(host_shim, syn, dim):
    scb, splan, sdata, srows = dim
    m = model_of(scb, srows, ["D-ACCT"], syn[1], ["ACCT-NO"])
    hs = HostFromSet(host_shim, syn[1], ["ACCT-NO"], splan, ["D-ACCT"], sdata, stride=DIM_SIZE, max_values=m.n_source_keys)
    cap = 2
    while cap < 2 * m.n_source_keys:
        cap <<= 1
    assert counts_of(hs.source_info) == m.counts() and hs.source_info.source_capacity == cap
    with pytest.raises(HostError) as e:
        HostFromSet(host_shim, syn[1], ["ACCT-NO"], splan, ["D-ACCT"], sdata, stride=DIM_SIZE, max_values=m.n_source_keys - 1)
    assert e.value.rc == N.CBX_E_CAPACITY and "max_values" in e.value.reason
    for bad, word in ((0, "at least 1"), (1 << 40, "workspace")):
        with pytest.raises(HostError) as e:
            HostFromSet(host_shim, syn[1], ["ACCT-NO"], splan, ["D-ACCT"], sdata, stride=DIM_SIZE, max_values=bad)
        assert e.value.rc == N.CBX_E_ARGUMENT and word in e.value.reason


def _tables(pplan, names, splan, snames):
    pt, st = N.CbxGroupBy(), N.CbxGroupBy()
    for t, plan, cols in ((pt, pplan, names), (st, splan, snames)):
        t.n_keys = len(cols)
        for i, c in enumerate(cols):
            t.fields[i] = _fi(plan, c)
    return pt, st


def test_host_build_refusals(host_shim, syn, dim):
    """keyset_from_build: the C side's compatibility rules with their wording, each side's group_build refusals prefixed."""
    pplan, splan = syn[1], dim[1]
    wide = _plan(WIDE_COPYBOOK)

    def status(pp, names, sp, snames, **kw):
        try:
            HostFromSet(host_shim, pp, names, sp, snames, b"", stride=1, tables=_tables(pp, names, sp, snames), **kw)
        except HostError as e:
            return e.rc, e.reason
        return 0, ""

    assert status(pplan, ["BR-ID"], splan, ["D-BR"])[0] == 0
    for names, snames, rc, word in ((["BR-ID", "NAME"], ["D-BR"], N.CBX_E_ARGUMENT, "2 probe keys against 1 source keys"),
                                    (["NAME"], ["D-BR"], N.CBX_E_ARGUMENT, "key 0: a string column against a numeric one"),
                                    (["BR-ID", "ACCT-NO"], ["D-BR", "D-NAME"], N.CBX_E_ARGUMENT, "key 1: a string column"),
                                    (["AMT-01"], ["D-RATE"], N.CBX_E_UNSUPPORTED, "key 0: scales 2 and 3 differ"),
                                    (["BR-ID", "BR-ID"], ["D-BR", "D-ACCT"], N.CBX_E_ARGUMENT, "probe: cbx_group_by: key 1: field repeated"),
                                    (["BR-ID", "ACCT-NO"], ["D-BR", "D-BR"], N.CBX_E_ARGUMENT, "source: cbx_group_by: key 1: field repeated"),
                                    (["FX-RATE"], ["D-BR"], N.CBX_E_UNSUPPORTED, "probe: cbx_group_by: key 0: COMP-1 / COMP-2 key"),
                                    ([], [], N.CBX_E_ARGUMENT, "probe: cbx_group_by: 1 to 4")):
        got, err = status(pplan, names, splan, snames)
        assert got == rc and word in err, (names, snames, got, err)
    for col, word in (("ITEM-NO", "OCCURS"), ("RATE", "COMP-1 / COMP-2 key")):
        got, err = status(wide, [col], splan, ["D-BR"])
        assert got == N.CBX_E_UNSUPPORTED and err.startswith("probe: ") and word in err
        got, err = status(pplan, ["BR-ID"], wide, [col])
        assert got == N.CBX_E_UNSUPPORTED and err.startswith("source: ") and word in err
    got, err = status(wide, ["NAME"], splan, ["D-NAME"], p_walk=True)
    assert got == N.CBX_E_UNSUPPORTED and err.startswith("probe: ") and "data-dependent" in err
    got, err = status(pplan, ["NAME"], wide, ["NAME"], s_walk=True)
    assert got == N.CBX_E_UNSUPPORTED and err.startswith("source: ") and "data-dependent" in err
    long_plan = _plan("       01  R.\n           05  S32  PIC X(32).\n           05  S33  PIC X(33).\n")
    got, err = status(pplan, ["NAME"], long_plan, ["S33"])
    assert got == N.CBX_E_UNSUPPORTED and err.startswith("source: ") and "longer than 32" in err
    from test_decode_fuzz import ASCII_COPYBOOK
    _, aplan = reader_plan(ASCII_COPYBOOK, ReaderParameters(is_ebcdic=False))
    got, err = status(aplan, ["N2"], splan, ["D-NAME"])
    assert got == N.CBX_E_UNSUPPORTED and err.startswith("probe: ") and "UTF-16" in err


def _mixed(cb, plan, p, a: bytes, b: bytes, size: int, n_a: int):
    """The first n_a records of a followed by b's from there on: a probe file that shares some keys with a."""
    from oracle import reader_oracle as RO
    data = a[:size * n_a] + b[size * n_a:]
    return cb, plan, data, RO.fixed_len_rows(cb, data, p)


@pytest.mark.parametrize("start,end", [(0, 0), (3, 2)])
@pytest.mark.parametrize("code_page,trim", FUZZ_OPTIONS)
def test_host_every_key_kind_ebcdic(host_shim, code_page, trim, start, end):
    """The decoder fuzz copybook as source and as probe: every accepted key kind on both sides."""
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
            exp = check_from(host_shim, probe, names, source, names, probe_src=dict(stride=stride, start_off=start),
                             source_src=dict(stride=stride, start_off=start))
            some += 0 < exp.sum() < len(exp)
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
    by_kind = _key_candidates(plan, cb)
    assert {k for k, _ in by_kind} >= {N.K_STRING if charset else N.K_STRING_ASCII, N.K_ASCII_NUM}
    for cols in by_kind.values():
        exp = check_from(host_shim, probe, cols[:1], source, cols[:1])
        assert exp.any()


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_width_ladder_cut_by_short_records(host_shim, trim):
    """Strings of every width class cut by short records on the source side (a key past the record's end is null, one
    that starts at its end is ""), probed by whole and cut records of another file."""
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    sraw, soff, sln = ladder_file(seed=34, every_length=True)
    praw, poff, pln = ladder_file(n=300, seed=35)
    source = (cb, plan, sraw, RO.var_len_rows(cb, sraw, p))
    probe = (cb, plan, praw, RO.var_len_rows(cb, praw, p))
    assert len(source[3]) == len(soff) and len(probe[3]) == len(poff)
    some = 0
    for names in (["X05"], ["X32"], ["X01"], ["X12"], ["P05"], ["Z07"], ["X03", "P03"], ["X02", "X01", "Z01", "P01"]):
        exp = check_from(host_shim, probe, names, source, names, probe_src=dict(framing=(poff, pln, None)),
                         source_src=dict(framing=(soff, sln, None)))
        some += 0 < exp.sum() < len(exp)
        if names == ["X01"]:
            assert exp.any()
    assert some >= 2
    m = model_of(cb, source[3], ["X05"], plan, ["X05"])
    assert m.n_null_rows > 0 and ("",) in m.values
    # a wider source string against a narrower probe column: what does not fit is dropped
    m = model_of(cb, source[3], ["X12"], plan, ["X05"])
    exp = check_from(host_shim, probe, ["X05"], source, ["X12"], probe_src=dict(framing=(poff, pln, None)),
                     source_src=dict(framing=(soff, sln, None)))
    assert m.n_dropped > 0 and exp.any()


def test_host_segment_redefines(host_shim):
    """RDW_NARROW with its redefine map as the source: a key inside an inactive redefine is null (counted, no member)."""
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
    for names in (["SEGMENT-ID"], ["TAXPAYER-TYPE"], ["TAXPAYER-NUM"], ["SEGMENT-ID", "TAXPAYER-TYPE"]):
        for filters in ([], [F.EqualTo("SEGMENT-ID", "C")]):
            exp = check_from(host_shim, probe, names, source, names, filters, probe_src=psrc, source_src=ssrc)
            assert exp.any(), names
    m = model_of(cb, source[3], ["TAXPAYER-NUM"], plan, ["TAXPAYER-NUM"])
    assert m.n_null_rows > 100 and 0 < m.n_source_keys < m.n_rows - m.n_null_rows + 1


@pytest.mark.parametrize("trim", ["none", "left", "right", "both"])
def test_host_equal_values_of_different_bytes_collapse_to_one_source_key(host_shim, trim):
    """The copybook of test_group.py: the sign nibbles of a COMP-3 zero, overpunch spellings, padding and code-page twins
    are one source key each (n_source_keys is the model's), whichever record claimed the slot."""
    from oracle import reader_oracle as RO
    p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=trim)
    cb, plan = reader_plan(EQUAL_COPYBOOK, p)
    data = equal_records(plan)
    rows = RO.fixed_len_rows(cb, data, p)
    whole = (cb, plan, data, rows)
    third = (cb, plan, data[:EQUAL_SIZE * 64], rows[:64])
    for names in (["KB"], ["KP"], ["KZ"], ["KX4"], ["KX3"], ["KB", "KP", "KX4", "KX3"], ["KZ", "KX3"]):
        m = model_of(cb, rows, names, plan, names)
        assert m.n_source_keys < m.n_rows - m.n_null_rows and m.n_dropped == 0
        if len(names) == 1:
            assert m.n_source_keys <= 8
        check_from(host_shim, whole, names, whole, names)
        check_from(host_shim, whole, names, third, names)
    # KP (S9(20) COMP-3) against KB-sized columns: +-10^19 cannot be an int16 / int32 value's column ... but KB is
    # integral like KP, so the pair is accepted and the wide values are dropped
    m = model_of(cb, rows, ["KP"], plan, ["KB"])
    exp = check_from(host_shim, whole, ["KB"], whole, ["KP"])
    assert m.n_dropped == 2 and exp.any() and not exp.all()


# ---------------------------------------------------------------------------------------------
# The stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snames,names", [(["D-BR"], ["BR-ID"]), (["D-NAME"], ["NAME"]), (["D-BIG", "D-NAME", "D-AMT"], ["ACCT-NO", "NAME", "AMT-01"])])
def test_host_program_under_the_sanitizers(tmp_path_factory, syn, dim, snames, names):
    """tests/native/keyset_from_host_main.cpp built with -fsanitize=address,undefined over exact-size heap buffers: a
    fixed source run and a framed run that cuts the source records inside and in front of the key fields, each probed
    with the SYN200 records, and a build with max_values one too small.  A subprocess of its own: nothing loaded into
    Python runs under a sanitizer."""
    pcb, pplan, pdata, prows = syn
    scb, splan, sdata, srows = dim
    n = 300
    exe = tmp_path_factory.getbasetemp() / "keyset_from_host_check"
    if not exe.exists():
        r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "tests", "native"), "-o", str(exe),
                            os.path.join(ROOT, "tests", "native", "keyset_from_host_main.cpp")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    pt, st = K.compile_key_pairs(pplan, names, splan, snames)
    head = struct.pack("<6i3q4i4i", len(pplan.fields), len(splan.fields), 200, DIM_SIZE, len(names), 0, len(prows), n, 65536,
                       *(list(pt.fields)[:4]), *(list(st.fields)[:4]))
    case = tmp_path_factory.mktemp("ksf_case") / "case.bin"
    pf = (N.CbxField * len(pplan.fields))(*pplan.fields)
    sf = (N.CbxField * len(splan.fields))(*splan.fields)
    blob = sdata[:DIM_SIZE * n]
    case.write_bytes(head + bytes(pf) + bytes(sf) + bytes(pplan.options.lut) + bytes(splan.options.lut) + pdata + blob)
    r = subprocess.run([str(exe), str(case)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-4000:], r.stdout)
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    # the framed run's records, cut as the program cuts them, through the oracle's variable-length reader
    from oracle import reader_oracle as RO
    cuts = [(DIM_SIZE * i, (7 * i) % DIM_SIZE + 1) for i in range(n)]
    for back in range(1, DIM_SIZE + 1):
        cuts[n - back] = (len(blob) - back, back)
    vp = ReaderParameters(is_record_sequence=True, schema_policy="collapse_root")
    vcb = parse_copybook_for(DIM_COPYBOOK, vp)
    cut_rows = RO.var_len_rows(vcb, rdw_file([blob[o:o + ln] for o, ln in cuts]), vp)
    assert len(cut_rows) == n
    forms = (0, 1) if len(names) == 1 else (0,)
    want = []
    for name, cb, rows in (("fixed", scb, srows[:n]), ("framed", vcb, cut_rows)):
        m = model_of(cb, rows, snames, pplan, names)
        want.append([name, "source", "rows", str(m.n_rows), "nulls", str(m.n_null_rows), "keys", str(m.n_source_keys), "dropped",
                     str(m.n_dropped), "distinct", str(len(m.values))])
        want += [[name, "not_in" if neg else "in", "kept", str(expected_set_keep(pcb, prows, [], [(names, m.values, neg)]).sum())]
                 for neg in forms]
    want.append(["overflow", str(N.CBX_E_CAPACITY), "1"])
    assert lines == want
    assert 0 < int(want[1][3]) < len(prows)
