"""GPU: the deferred-value pass (cbx_kernels.hip fixup_kernel<kind>) against the oracle.

The pass compacts the set bits of a span of S = kFixSpan tiles of one deferral sequence into an LDS
list of L = kFixList entries and decodes the list with the byte-loop decoder of the sequence's kind.
The cases sit on its edges: record counts around a tile and around a span, no deferral at all, single
deferrals on word / span borders, every value deferred (a span then takes 16 fills of the list), a
seeded 1 % mix, the decoder kinds that always defer, an OCCURS field (several sequences of one field),
a non-zero record start offset and the variable-length path.

Run on an MI355X: python -u -m pytest tests/test_gpu_fixup.py -m gpu -x -v
"""
from __future__ import annotations

import functools
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from parity import compare_batch  # noqa: E402

from cobrix_amd.reader import (FixedLenNestedReader, ReaderParameters, VarLenNestedReader,  # noqa: E402
                               parse_copybook_for)
from oracle import oracle as O  # noqa: E402

S = 1024   # kFixSpan: tiles of 64 records per workgroup span
L = 4096   # kFixList: entries of the LDS list
COUNTS = [1, 63, 64, 65, 64 * S - 1, 64 * S, 64 * S + 1, 2 * 64 * S + 70]
JIT = [-1, 1]   # the table-driven kernel / the copybook-specialised kernel forced


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_constants_mirror_the_kernel():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cobrix_amd", "csrc", "cbx_kernels.hip")).read()
    threads = int(re.search(r"constexpr int kFixThreads = (\d+);", src).group(1))
    words = int(re.search(r"#define CBX_FIX_WORDS (\d+)", src).group(1))
    assert threads * words == S
    assert int(re.search(r"constexpr int kFixList = (\d+);", src).group(1)) == L
    assert 64 * S > L   # a fully deferred span needs more than one fill


def _kernel_kind(rd) -> int:
    import ctypes
    from cobrix_amd import native as N
    k = ctypes.c_int32(-1)
    N.check(N.load().cbx_plan_kernel_kind(rd.native.handle, ctypes.byref(k)))
    return k.value


# ------------------------------------------------------------------------------------------------
# Zoned fields of the SWAR fast path: a value defers exactly when its bytes leave the fast form
# (F-zone digits, overpunch in the last byte), so the test decides which values reach the pass.
# ------------------------------------------------------------------------------------------------
ZONED_COPYBOOK = """
       01  R.
           05  ZU    PIC 9(5).
           05  ZS    PIC S9(7).
           05  ZG    OCCURS 3.
              10  ZO    PIC S9(3).
           05  ZD    PIC S9(5)V99.
           05  TAG   PIC X(4).
"""
# (offset, size, signed) of the 6 numeric values of a record; TAG at 28..31
ZONED_VALUES = [(0, 5, False), (5, 7, True), (12, 3, True), (15, 3, True), (18, 3, True), (21, 7, True)]
ZONED_SIZE = 32
START = 3   # record_start_offset of the fixed-length cases


def _clean_zoned(rng, n: int) -> np.ndarray:
    rec = np.empty((n, ZONED_SIZE), dtype=np.uint8)
    rec[:, :28] = 0xF0 + rng.integers(0, 10, (n, 28), dtype=np.uint8)
    for off, size, signed in ZONED_VALUES:
        if signed:   # overpunch in the last byte: C / D / F zone
            zone = rng.choice(np.array([0xC0, 0xD0, 0xF0], dtype=np.uint8), n)
            rec[:, off + size - 1] = zone | (rec[:, off + size - 1] & 0x0F)
    rec[:, 28:] = np.frombuffer(b"\xC1\xC2\xF1\x40", dtype=np.uint8)
    return rec


def _defer_form(rec_row: np.ndarray, off: int, size: int, form: int) -> None:
    """Rewrite one clean value into a form the fast path leaves to the pass."""
    mid = off + size // 2
    last = off + size - 1
    if form == 0:
        rec_row[off] = 0x60                                  # separate leading '-'
    elif form == 1:
        rec_row[last] = 0x4E                                 # separate trailing '+'
    elif form == 2:
        rec_row[off] = 0x40                                  # leading space
    elif form == 3:
        rec_row[mid] = 0x40                                  # embedded space
    elif form == 4:
        rec_row[mid] = 0x4B                                  # explicit dot
    elif form == 5:
        rec_row[off] = 0x00                                  # NUL
    elif form == 6:
        rec_row[mid] = 0xAB                                  # a byte outside the allowed set
    else:
        rec_row[off] = 0xD0 | (rec_row[off] & 0x0F)          # overpunch in the first byte
        rec_row[last] = 0xF0 | (rec_row[last] & 0x0F)


def _zoned_mask(pattern: str, n: int, rng) -> np.ndarray:
    nv = len(ZONED_VALUES)
    m = np.zeros((n, nv), dtype=bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "single":
        # record 0, the last record, bit 0 / bit 63 of a word, the first / last word of a span
        recs = [0, 63, 64, 127, 64 * (S - 1), 64 * S - 1, 64 * S, 64 * S + 63, 64 * (2 * S - 1), 2 * 64 * S - 1,
                2 * 64 * S, n - 1]
        for i, r in enumerate(x for x in recs if 0 <= x < n):
            m[r, i % nv] = True
    elif pattern == "mix":
        m = rng.random((n, nv)) < 0.01
        if n >= 2:   # a tile with a deferred and a clean value of one field, whatever the draw
            m[n // 2, 1] = True
            m[n // 2 - 1, 1] = False
    return m


@functools.lru_cache(maxsize=None)
def _zoned_case(n: int, pattern: str):
    """(file bytes, oracle result, deferred mask) -- shared by the kernel kinds, never modified."""
    rng = np.random.default_rng(1000 * COUNTS.index(n) + ["none", "single", "all", "mix"].index(pattern))
    rec = _clean_zoned(rng, n)
    mask = _zoned_mask(pattern, n, rng)
    forms = rng.integers(0, 8, mask.shape)
    for r, v in zip(*np.nonzero(mask)):
        off, size, _ = ZONED_VALUES[v]
        _defer_form(rec[r], off, size, int(forms[r, v]))
    data = np.empty((n, START + ZONED_SIZE), dtype=np.uint8)
    data[:, :START] = 0xEE
    data[:, START:] = rec
    data = data.tobytes()
    cb = parse_copybook_for(ZONED_COPYBOOK, ReaderParameters(start_offset=START))
    res = O.decode_fixed(cb, data, record_size=ZONED_SIZE, start_offset=START, end_offset=0)
    return data, res, mask


def _decode_fixed(copybook: str, data: bytes, jit: int, **kw):
    rd = FixedLenNestedReader(copybook, ReaderParameters(jit_min_records=jit, **kw))
    batch = rd.decode(data)
    assert _kernel_kind(rd) == (1 if jit == 1 else 0)
    return rd, batch


def _seen_by(rd, res):
    """The shared oracle result for this reader: compare_batch finds a column's oracle node by the
    identity of the reader's copybook statement, and the event stream names nodes by their number in
    walk order -- the same for every parse of one copybook text."""
    ast = O.OracleAst(rd.copybook)
    assert len(ast.stmts) == len(res.ast.stmts)
    return O.OracleResult(ast, res.events, res.heap, res.n_rec)


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("pattern", ["none", "single", "all", "mix"])
@pytest.mark.parametrize("n", COUNTS)
def test_zoned_deferral_patterns(n, pattern, jit):
    """(a) no deferral: the pass leaves values and validity as the decode kernel wrote them; (b) single
    deferrals on the borders of words and spans; (c) every value deferred: spans of more than L values
    refill the list; (d) a seeded 1 % mix with clean and deferred values of a field in one tile (a
    dropped validity OR or a misplaced index shows as a wrong neighbour).  Fixed-length records behind a
    3-byte record start offset."""
    data, res, mask = _zoned_case(n, pattern)
    if pattern == "mix" and n >= 2:
        t = (n // 2) // 64
        col = mask[64 * t:64 * (t + 1), 1]
        assert col.any() and not col.all()
    if pattern == "all" and n >= 64 * S - 1:
        assert mask[:64 * S, 0].sum() > L
    rd, batch = _decode_fixed(ZONED_COPYBOOK, data, jit, start_offset=START)
    errs = compare_batch(batch, _seen_by(rd, res))
    assert not errs, errs[:8]


# ------------------------------------------------------------------------------------------------
# Kinds whose every value is deferred (byte-loop decoders only): one instantiation of the pass each.
# ------------------------------------------------------------------------------------------------
GENERIC_COPYBOOK = """
       01  R.
           05  ZW    PIC 9(20).
           05  PW    PIC S9(33) COMP-3.
           05  BP    PIC SPPP9 COMP.
           05  BW    PIC 9(20) COMP.
"""
DISPLAY_FORMS_COPYBOOK = """
       01  R.
           05  ZL    PIC S9(7) SIGN LEADING SEPARATE.
           05  ZT    PIC S9(5)V99 SIGN TRAILING SEPARATE.
           05  ZX    PIC S9(3).99.
           05  ZP    PIC SPPP9(5).
           05  ZQ    PIC S9(5)PPP.
           05  ZV    PIC 9(10)V9(6).
"""
ASCII_COPYBOOK = """
       01  R.
           05  A1    PIC S9(4).
           05  A2    PIC S9(17).
           05  A3    PIC S9(5)V99.
           05  A4    PIC S9(3).99.
           05  A5    PIC S9(7) SIGN LEADING SEPARATE.
           05  A6    PIC SPPP9(3).
"""


@functools.lru_cache(maxsize=None)
def _fuzz_case(name: str, n: int):
    """Records of random field bytes (the decoder fuzz's generators), repeated from a pool."""
    from test_decode_fuzz import _random_ascii_bytes, _random_bytes
    from cobrix_amd import copybook as cbk
    text, kw = {"generic": (GENERIC_COPYBOOK, {}), "display": (DISPLAY_FORMS_COPYBOOK, {}),
                "ascii": (ASCII_COPYBOOK, {"is_ebcdic": False})}[name]
    cb = parse_copybook_for(text, ReaderParameters(**kw))
    leaves = list(O._iter_leaves(cb.ast))
    rng = np.random.default_rng(len(name) + 31 * COUNTS.index(n))
    gen = (lambda p: _random_ascii_bytes(rng, p, p.data_size, True)) if name == "ascii" else \
        (lambda p: _random_bytes(rng, p, p.data_size))
    pool = [b"".join(gen(p) for p in leaves) for _ in range(min(n, 1021))]
    assert len(pool[0]) == cb.record_size <= 48
    order = rng.integers(0, len(pool), n)
    data = b"".join(pool[i] for i in order)
    return text, kw, data, O.decode_fixed(cb, data)


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["generic", "display", "ascii"])
def test_always_deferred_kinds(name, n, jit):
    """generic: zoned of more than 18 digits (16-byte decimals), COMP-3 wider than 16 bytes, a P-scaled
    and an odd-width binary -- the BCD, binary and zoned instantiations in one plan; display: separate
    signs, explicit dot, P-scaled zoned, a 16-digit decimal; ascii: an ASCII-numeric file.  Every value
    of the byte-loop-only fields is deferred, so each span of 64 * S records refills the list."""
    text, kw, data, res = _fuzz_case(name, n)
    rd, batch = _decode_fixed(text, data, jit, **kw)
    errs = compare_batch(batch, _seen_by(rd, res))
    assert not errs, errs[:8]


# ------------------------------------------------------------------------------------------------
# Variable-length records (rec_off non-null): deferred zoned values in both segment redefines.
# ------------------------------------------------------------------------------------------------
VAR_COPYBOOK = """
       01  REC.
           05  SEGMENT-ID   PIC X(1).
           05  SEG-A.
              10  A1        PIC S9(7).
              10  A2        PIC 9(5).
           05  SEG-B REDEFINES SEG-A.
              10  B1        PIC 9(4).
              10  B2        PIC S9(9).
"""
VAR_SEGMENTS = {"A": "SEG-A", "B": "SEG-B"}


@pytest.mark.parametrize("jit", JIT)
def test_var_length_deferred_in_both_segments(jit):
    n = 64 * 3 + 5
    rng = np.random.default_rng(77)
    body = bytearray()
    payloads, segs = [], []
    deferred = {"SEG_A": 0, "SEG_B": 0}
    for i in range(n):
        is_a = bool(rng.random() < 0.5)
        fields = [(1, 7), (8, 5)] if is_a else [(1, 4), (5, 9)]
        p = np.empty(14, dtype=np.uint8)
        p[0] = 0xC1 if is_a else 0xC2
        p[1:] = 0xF0 + rng.integers(0, 10, 13, dtype=np.uint8)
        if rng.random() < 0.3:
            off, size = fields[int(rng.integers(0, 2))]
            _defer_form(p, off, size, int(rng.integers(0, 8)))
            deferred["SEG_A" if is_a else "SEG_B"] += 1
        p = bytes(p[:13 if is_a else 14])
        payloads.append(p)
        segs.append("SEG_A" if is_a else "SEG_B")
        body += bytes([0, 0, len(p) & 0xFF, len(p) >> 8]) + p
    assert deferred["SEG_A"] > 5 and deferred["SEG_B"] > 5
    raw = bytes(body)
    params = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID", segment_id_redefine_map=VAR_SEGMENTS,
                              jit_min_records=jit)
    rd = VarLenNestedReader(VAR_COPYBOOK, params)
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    off, ln = rd.frame(t, len(raw))
    eo, el = O.frame_rdw(raw)
    assert np.array_equal(off.cpu().numpy(), eo) and np.array_equal(ln.cpu().numpy(), el)
    batch = rd.decode_device(t, len(raw), off, ln)
    res = O.decode_records(rd.copybook, payloads, active_segments=segs)
    errs = compare_batch(batch, res)
    assert not errs, errs[:8]
