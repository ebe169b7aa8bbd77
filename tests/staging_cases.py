"""Inputs of the staging-path tests (tests/test_gpu_staging.py): the decoder fuzz copybooks cut into
slices small enough for every staging path of the decode kernel, two small copybooks for the geometry
sweeps, and seeded fixed-length / RDW files over them.

The contiguous staging takes records of at most 252 bytes and the span staging records of at most 256;
FUZZ_COPYBOOK (517 bytes) and the fuzz's ASCII_COPYBOOK (292 bytes) reach neither.  A slice holds
consecutive 05-level fields of one of them, at most SLICE_BYTES bytes, so that every decoder shape of
the fuzz runs through every loop.  tests/test_staging_cases.py pins this module: a slicing bug would
silently drop coverage.
"""
from __future__ import annotations

import functools
import re
from typing import Dict, List, Tuple

import numpy as np

from cobrix_amd import copybook as cbk
from oracle import oracle as O
from test_decode_fuzz import ASCII_COPYBOOK, FUZZ_COPYBOOK, _random_ascii_bytes, _random_bytes

SLICE_BYTES = 60
HEADER = "       01  R.\n"

MIX = HEADER + """\
           05  MS    PIC X(3).
           05  MZ    PIC S9(3).
           05  MP    PIC S9(5) COMP-3.
           05  MH    PIC S9(4) COMP.
           05  MW    PIC S9(9) COMP.
           05  MD    PIC 9(1).
"""
TINY = HEADER + """\
           05  TH    PIC S9(4) COMP.
           05  TP    PIC 9(3) COMP-3.
"""


def field_lines(text: str) -> List[str]:
    """The 05-level lines of a flat copybook, in order."""
    lines = [ln for ln in text.split("\n") if re.match(r"\s+05\s", ln)]
    assert lines and all(ln.rstrip().endswith(".") for ln in lines)
    return lines


def parse(text: str, ascii: bool = False, **kw) -> cbk.Copybook:
    return cbk.parse_copybook(text, data_encoding=cbk.ASCII if ascii else cbk.EBCDIC, **kw)


def slices(text: str, ascii: bool = False, limit: int = SLICE_BYTES) -> List[str]:
    """The copybook's 05-level lines cut greedily, in order, into sub-copybooks of at most `limit`
    payload bytes."""
    out: List[str] = []
    cur: List[str] = []
    size = 0
    for ln in field_lines(text):
        n = parse(HEADER + ln + "\n", ascii).record_size
        assert 0 < n <= limit, ln
        if cur and size + n > limit:
            out.append(HEADER + "\n".join(cur) + "\n")
            cur, size = [], 0
        cur.append(ln)
        size += n
    out.append(HEADER + "\n".join(cur) + "\n")
    return out


@functools.lru_cache(maxsize=None)
def fuzz_slices() -> Tuple[str, ...]:
    return tuple(slices(FUZZ_COPYBOOK))


@functools.lru_cache(maxsize=None)
def ascii_slices() -> Tuple[str, ...]:
    return tuple(slices(ASCII_COPYBOOK, ascii=True))


# The slices as the GPU tests name them: id -> (source, index, bytes, plain stride, padded stride).
# plain: the smallest 4 * odd at or above the size (rows staged as they lie); padded: the smallest multiple
# of 16 (rows padded to an odd dword pitch).  Written out so that the GPU tables read as literals;
# tests/test_staging_cases.py checks them against the slices.
SLICE_TABLE = {
    "f0": ("fuzz", 0, 57, 60, 64), "f1": ("fuzz", 1, 38, 44, 48), "f2": ("fuzz", 2, 47, 52, 48),
    "f3": ("fuzz", 3, 57, 60, 64), "f4": ("fuzz", 4, 54, 60, 64), "f5": ("fuzz", 5, 52, 52, 64),
    "f6": ("fuzz", 6, 59, 60, 64), "f7": ("fuzz", 7, 59, 60, 64), "f8": ("fuzz", 8, 59, 60, 64),
    "f9": ("fuzz", 9, 35, 36, 48),
    "a0": ("ascii", 0, 60, 60, 64), "a1": ("ascii", 1, 57, 60, 64), "a2": ("ascii", 2, 58, 60, 64),
    "a3": ("ascii", 3, 53, 60, 64), "a4": ("ascii", 4, 26, 28, 32), "a5": ("ascii", 5, 38, 44, 48),
}


def slice_text(sid: str) -> str:
    source, index = SLICE_TABLE[sid][:2]
    return (fuzz_slices() if source == "fuzz" else ascii_slices())[index]


def leaves(cb: cbk.Copybook) -> List[cbk.Primitive]:
    return list(O._iter_leaves(cb.ast))


def payloads(cb: cbk.Copybook, n: int, seed: int, ascii: bool = False) -> np.ndarray:
    """(n, record_size) random field bytes of the decoder fuzz's generators: a pool of at most 1021
    distinct records, drawn n times."""
    rng = np.random.default_rng(seed)
    lv = leaves(cb)
    gen = (lambda p: _random_ascii_bytes(rng, p, p.data_size, True)) if ascii else \
        (lambda p: _random_bytes(rng, p, p.data_size))
    pool = np.frombuffer(b"".join(gen(p) for _ in range(min(n, 1021)) for p in lv), dtype=np.uint8)
    pool = pool.reshape(-1, cb.record_size)
    return pool[rng.integers(0, len(pool), n)] if n > len(pool) else pool


def fixed_file(cb: cbk.Copybook, n: int, seed: int, start: int = 0, end: int = 0, ascii: bool = False) -> bytes:
    """n fixed-length records of stride start + record_size + end: the payloads of `payloads` (the same
    for every start / end of a seed), random bytes in the start and end padding."""
    body = payloads(cb, n, seed, ascii)
    rng = np.random.default_rng(seed + 7919 * (start + 1) + 104729 * end)
    rec = rng.integers(0, 256, (n, start + cb.record_size + end), dtype=np.uint8)
    rec[:, start:start + cb.record_size] = body
    return rec.tobytes()


def rdw_file(cb: cbk.Copybook, n: int, seed: int, ascii: bool = False, long_every: int = 0) -> Tuple[bytes, List[bytes]]:
    """(RDW file, payload list): 30 % whole records, the others cut at a uniform length in
    1..record_size.  long_every = k > 0: record 0 of every k-th tile of 64 is the whole record followed by
    random bytes, 300-3000 bytes in all."""
    body = payloads(cb, n, seed, ascii)
    rng = np.random.default_rng(seed + 15485863)
    size = cb.record_size
    recs: List[bytes] = []
    for i in range(n):
        b = body[i].tobytes()
        if long_every and i % (64 * long_every) == 0:
            b += rng.integers(0, 256, int(rng.integers(300, 3001)) - size, dtype=np.uint8).tobytes()
        elif rng.random() >= 0.3:
            b = b[:int(rng.integers(1, size + 1))]
        recs.append(b)
    raw = b"".join(bytes([0, 0, len(r) & 0xFF, len(r) >> 8]) + r for r in recs)
    return raw, recs


def field_events(res: "O.OracleResult") -> Dict[str, list]:
    """Per leaf name: the leaf's value events (record, slot, null flag, value words, heap bytes of a
    string) in record order -- what a decode says about the field, free of node numbers and heap
    positions."""
    cols = O.columns(res)
    out: Dict[str, list] = {}
    for p in leaves(res.ast.cb):
        c = cols.get(res.ast.node_of(p))
        rows = []
        if c is not None:
            for k in np.argsort(c["rec"], kind="stable"):
                valid = bool(c["valid"][k])
                lo, hi = int(c["lo"][k]), int(c["hi"][k])
                if valid and p.is_string:
                    rows.append((int(c["rec"][k]), int(c["slot"][k]), True, res.heap[lo:lo + hi]))
                else:
                    rows.append((int(c["rec"][k]), int(c["slot"][k]), valid, (lo, hi) if valid else None))
        out[p.name] = rows
    return out
