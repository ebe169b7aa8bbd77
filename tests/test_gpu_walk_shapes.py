"""GPU: every decoder shape, string composition, record source, validity form and layout shape through the
record walk (cbx_walk.h, walk_launch, jit_walk_source / jit_chain_source), against the oracle.

The walk is the one decode path whose field offsets depend on the data; it has its own primitive decoder
(walk_prim_f), numeric fast paths (walk_numeric) and tile staging.  Every case decodes the same bytes as
the oracle (RO.var_len_rows / RO.fixed_len_rows, never another GPU path), on the table-driven walk and on
the copybook-specialised one, and asserts the kernel kind and the launch the library reports
(cbx_plan_walk_info) against the values written here: a dispatch change that moves a case to another
path fails it instead of silently taking its coverage away.  Inputs: walk_cases.py (pinned on the CPU by
test_walk_cases.py).

  A  decoder slices behind / inside an ODO array (RDW) and inside one at a fixed stride
  B  dense strings: 2- and 3-byte code-page entries through the register path and its wave-wide fallback
  C  record source: no staging (HBM), tiles straddling stage_cap at four pointer offsets
  D  validity words: global atomics by the environment and by size
  E  the selection source (cbx_decode_selected) with a segment redefine
  F  random layouts over RDW and over VarOccursRecordExtractor framing
  G  the nesting limit

The EBCDIC slices rotate through the decoder fuzz's (code page, trim, float format) triples; the slices
that the options change -- f0 (the strings) and f9 (COMP-1 / COMP-2) -- run under all three.  The ASCII
slices rotate through "" and windows-1252, a0 (the string) runs under both.

Run on an MI355X: python -u -m pytest tests/test_gpu_walk_shapes.py -m gpu -x -v --durations=0
"""
from __future__ import annotations

import dataclasses
import functools
import random
import struct
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import staging_cases as S  # noqa: E402
import walk_cases as W  # noqa: E402

from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader  # noqa: E402
from cobrix_amd.synth import WALK_NESTED_COPYBOOK, walk_nested_record  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_gpu_filter import FUZZ_GPU_OPTIONS  # noqa: E402

KERNELS = ("table", "jit")
JIT_MIN = {"table": -1, "jit": 1}
KIND = {"table": 2, "jit": 3}
ASCII_CHARSETS = ("", "windows-1252")
TILES = 6            # tiles of 64 records in walk_cases.N_REC = 321


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@dataclass(frozen=True)
class Case:
    id: str
    src: Tuple               # ("slice", sid, how) | ("dense", page) | ("random", seed) | (name,) of SPECIAL
    option: object = None    # slice: options triple / charset; dense: trim
    framing: str = "rdw"     # rdw: RDW headers; fixed: fixed-length records; b2b: VarOccursRecordExtractor
    kernel: str = "table"
    env: Tuple = ()          # environment of the call
    shift: int = 0           # data pointer & 15 (rdw)
    via: str = "device"      # device: frame + decode_device; read: select + cbx_decode_selected


# ------------------------------------------------------------------------------------------------
# inputs and expected rows: built once per (source, option, framing), shared by the kernels and the
# environments, never modified
# ------------------------------------------------------------------------------------------------
WIDE = """
       01  R.
         05  N-PAD  PIC 9(1).
         05  PAD    PIC X(1) OCCURS 0 TO 3 TIMES DEPENDING ON N-PAD.
         05  BIG    OCCURS 120 TIMES.
           10  W0   PIC 9(1).
           10  W1   PIC S9(3) COMP-3.
           10  W2   PIC X(2).
           10  W3   PIC 9(2).
           10  W4   PIC S9(4) COMP.
           10  W5   PIC X(1).
           10  W6   PIC 9(1) COMP-3.
           10  W7   PIC 9(3).
           10  W8   PIC X(3).
           10  W9   PIC S9(2).
         05  TAIL   PIC S9(7) COMP-3.
"""
WIDE_REC = 1 + 120 * 19 + 4     # without PAD


def _wide_records(n: int):
    rnd = random.Random(41)
    al = bytes(range(0xF0, 0xFA)) * 3 + b"\x40\xc1\xd2\x00\x0c\x1d"
    recs = []
    for _ in range(n):
        k = rnd.choice([0, 1, 2, 3, 7])
        b = bytes([0xF0 + k]) + bytes(rnd.choice(al) for _ in range((k if k <= 3 else 3) + WIDE_REC - 1))
        recs.append(b if rnd.random() < 0.7 else b[:rnd.randint(1, len(b))])
    return recs


def _deep(levels: int) -> str:
    """`levels` nested groups (the record's included), the innermost holding a dependee and an ODO array of
    primitives: the walk's frame stack is levels + 2 deep (the root's frame, one per group, the array's)."""
    out = ["       01  R."]
    for k in range(2, levels + 1):
        out.append(f"        {k:02d}  G{k}.")
    out.append(f"         {levels + 1:02d} N PIC 9(1).")
    out.append(f"         {levels + 1:02d} V PIC S9(3) COMP-3 OCCURS 0 TO 3 TIMES DEPENDING ON N.")
    out.append("        02  AFTER PIC X(3).")
    assert max(map(len, out)) <= 72
    return "\n".join(out) + "\n"


def _deep_records(n: int):
    rnd = random.Random(43)
    recs = []
    for _ in range(n):
        k = rnd.choice([0, 1, 2, 3, 5])
        b = bytes([0xF0 + k]) + b"".join(bytes([rnd.randrange(10) << 4 | rnd.randrange(10), rnd.randrange(10) << 4 | 0x0C])
                                       for _ in range(k if k <= 3 else 3)) + rnd.choice(["abc", "X  ", "   "]).encode("cp037")
        recs.append(b)
    return recs


def _segsel_layout():
    """The inside wrapper of slice f1 with a segment id in front and two segment redefines behind."""
    body = W.wrap("f1", "inside")
    a = W.Node("A-PART", children=[W.count_node("NA", "zoned", 3),
                                   W.Node("AV", "PIC S9(3) COMP-3", 2, lambda rng: bytes([int(rng.integers(0, 10)) << 4 | 5, 0x1C]),
                                          occurs=(0, 3), dep="NA")], seg="A")
    b = W.Node("B-PART", children=[W.count_node("NB", "zoned", 2),
                                   W.Node("BV", "PIC X(4)", 4, lambda rng: bytes(rng.choice([0x40, 0xC1, 0x82, 0xF7], 4).astype("uint8")),
                                          occurs=(0, 2), dep="NB")], redefines="A-PART", seg="B")
    return [W.Node("SEG", "PIC X(1)", 1, count="seg")] + body + [a, b]


@functools.lru_cache(maxsize=None)
def _input(src: Tuple, option, framing: str, shift: int = 0):
    """(copybook text, reader parameters without jit_min_records, file bytes, the records as generated)."""
    kind = src[0]
    if kind == "slice":
        _, sid, how = src
        body, recs = W.wrapped_records(sid, how)
        return W.copybook_text(body), W.wrapper_parameters(sid, how, option), (b"".join(recs) if how == "fixed" else W.rdw(recs)), recs
    if kind == "dense":
        body, recs = W.dense_records(src[1], src[2])
        return W.copybook_text(body), W.dense_parameters(src[1], option), W.rdw(recs), recs
    if kind == "random":
        lay = W.random_layout(src[1])
        recs = lay.records(W.N_REC, framed=framing == "rdw")
        p = ReaderParameters(is_record_sequence=framing == "rdw", **lay.options)
        return lay.text, p, (W.rdw(recs) if framing == "rdw" else b"".join(recs)), recs
    if kind == "straddle":
        return _straddle_input(shift)
    if kind == "wide":
        recs = _wide_records(130)
        return WIDE, ReaderParameters(is_record_sequence=True, variable_size_occurs=True, ebcdic_code_page="cp037"), W.rdw(recs), recs
    if kind == "nested":
        rnd = random.Random(5)
        recs = [walk_nested_record(rnd, True) for _ in range(W.N_REC)]
        return WALK_NESTED_COPYBOOK, ReaderParameters(is_record_sequence=True, variable_size_occurs=True), W.rdw(recs), recs
    if kind == "deep":
        recs = _deep_records(W.N_REC)
        p = ReaderParameters(is_record_sequence=framing == "rdw", variable_size_occurs=True, ebcdic_code_page="cp037")
        return _deep(src[1]), p, (W.rdw(recs) if framing == "rdw" else b"".join(recs)), recs
    assert kind == "segsel"
    body = _segsel_layout()
    recs = W.records(body, W.N_REC, 77)
    p = ReaderParameters(is_record_sequence=True, variable_size_occurs=True, ebcdic_code_page="cp037", generate_record_id=True,
                         segment_field="SEG", segment_id_redefine_map={"A": "A_PART", "B": "B_PART"})
    return W.copybook_text(body), p, W.rdw(recs), recs


STRADDLE_CAP = 3472          # stage_cap of the behind wrapper of f1: (64 * (46 + 8) + 31) & ~15
STRADDLE_DELTAS = (-2, -1, 0, 1, 2, 2, 1, 0, -1, -2)


def _straddle_input(shift: int):
    """The behind wrapper of f1, 10 tiles and one record: the last record of tile t lengthened with trailing
    bytes so that the tile's span (payload bytes + the headers between them + the first payload's address
    & 15 at this pointer offset) is STRADDLE_CAP + STRADDLE_DELTAS[t]."""
    body, _ = W.wrapped_records("f1", "behind")
    recs = W.records(body, 64 * len(STRADDLE_DELTAS) + 1, 4242)
    rnd = random.Random(shift)
    pos = 0
    for t, d in enumerate(STRADDLE_DELTAS):
        tile = recs[64 * t:64 * t + 64]
        lo = pos + 4
        mis = (shift + lo) & 15
        have = sum(len(r) + 4 for r in tile) - 4 + mis
        need = STRADDLE_CAP + d - have
        assert need > 0
        recs[64 * t + 63] = tile[63] + bytes(rnd.randrange(256) for _ in range(need))
        pos += sum(len(r) + 4 for r in recs[64 * t:64 * t + 64])
    return W.copybook_text(body), W.wrapper_parameters("f1", "behind"), W.rdw(recs), recs


@functools.lru_cache(maxsize=None)
def _expected(src: Tuple, option, framing: str, shift: int, via: str):
    text, p, data, _ = _input(src, option, framing, shift)
    from cobrix_amd.reader import parse_copybook_for
    cb = parse_copybook_for(text, p)
    if framing == "fixed":
        return _bits(RO.fixed_len_rows(cb, data, p))
    return _bits(RO.var_len_rows(cb, data, p, file_id=1 if via == "read" else 0))


def _bits(x):
    """Rows with every float as its bit pattern: the random bytes of COMP-1 / COMP-2 make NaNs."""
    if isinstance(x, np.floating):
        return (x.dtype.name, x.tobytes())
    if isinstance(x, float):
        return ("float", struct.pack("<d", x))
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    return x


def _device(data: bytes, shift: int, extra: int = 16):
    """The file on the GPU, `shift` bytes past a 16-byte boundary: a batch cut out of a larger tensor."""
    buf = torch.zeros(shift + len(data) + extra, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf[shift:]


INFO_FIELDS = [n for n, _ in N.CbxWalkInfo._fields_]


def run_case(c: Case, setenv):
    """Decode the case; (rows with floats as bits, reader, walk info as a dict, framing as (off, len) lists or None)."""
    for k, v in c.env:
        setenv(k, v)
    text, p, data, _ = _input(c.src, c.option, c.framing, c.shift)
    p = dataclasses.replace(p, jit_min_records=JIT_MIN[c.kernel])
    framing = None
    if c.framing == "fixed":
        rd = FixedLenNestedReader(text, p)
        assert rd.walk
        batch = rd.decode_device(_device(data, c.shift), len(data))
    else:
        rd = VarLenNestedReader(text, p)
        assert rd.walk
        if c.via == "read":
            batch = rd.read(data, file_id=1)
        elif c.framing == "b2b":
            t = rd._device_file(data)
            off, ln, vb = rd.frame_file(t, len(data))
            framing = (off.cpu().tolist(), ln.cpu().tolist())
            batch = rd.decode_device(t, vb, off, ln)
        else:
            t = _device(data, c.shift)
            off, ln = rd.frame(t, len(data))
            framing = (off.cpu().tolist(), ln.cpu().tolist(), t.data_ptr())
            batch = rd.decode_device(t, len(data), off, ln)
    rows = _bits(batch.to_rows())
    wi = N.walk_info(rd.native.handle)
    return rows, rd, {n: int(getattr(wi, n)) for n in INFO_FIELDS}, framing


def _kernel_kind(rd) -> int:
    import ctypes
    k = ctypes.c_int32()
    N.check(N.load().cbx_plan_kernel_kind(rd.native.handle, ctypes.byref(k)))
    return k.value


def _frame_kind(rd) -> int:
    import ctypes
    k = ctypes.c_int32()
    N.check(N.load().cbx_plan_frame_kind(rd.native.handle, ctypes.byref(k)))
    return k.value


def expect(depth: int, stage_cap: int, n_vslots: int, n_sslots: int, kernel: str, vlds: int = 1, tiles: int = TILES):
    """A case's cbx_walk_info from its table row: the frame stack is 800 bytes a level on the table walk
    (32 of the wave's + three rows of 64 ints) and in registers on the specialised one; the words are
    8 bytes a validity slot and 4 a string slot, rounded to 16, in LDS when vlds."""
    stack = 800 * depth if kernel == "table" else 0
    words = (8 * n_vslots + 4 * n_sslots + 15) & ~15 if vlds else 0
    return dict(kind=KIND[kernel], stage_cap=stage_cap, vlds=vlds, wave_lds=stack + stage_cap + words, depth=depth,
                stack_lds=stack, n_vslots=n_vslots, n_sslots=n_sslots, grid=(tiles + 3) // 4, n_tiles=tiles)


def check(c: Case, want: Dict[str, int], monkeypatch):
    rows, rd, info, framing = run_case(c, monkeypatch.setenv)
    print(c.id, info)
    exp = _expected(c.src, c.option, c.framing, c.shift, c.via)
    assert len(rows) == len(exp)
    bad = [i for i, (a, b) in enumerate(zip(rows, exp)) if a != b]
    assert not bad, (len(bad), bad[:5], rows[bad[0]], exp[bad[0]])
    assert _kernel_kind(rd) == KIND[c.kernel]
    assert info == want and set(want) == set(INFO_FIELDS), info
    return rows, rd, info, framing


def _ids(cases):
    assert len({c.id for c in cases}) == len(cases)
    return [pytest.param(c, id=c.id) for c in cases]


# ------------------------------------------------------------------------------------------------
# A. decoder slices.  Per slice: (depth, stage_cap, validity slots, string slots) of the behind, inside
# and fixed wrappers.  behind: depth 3 (root, record, PAD's elements); inside: 4 (+ the element's frame);
# fixed: 6 (OUTER's two frames more).
# ------------------------------------------------------------------------------------------------
SLICE_INFO: Dict[str, Tuple[Tuple[int, int, int, int], ...]] = {
    "f0": ((3, 4688, 15, 6), (4, 8144, 21, 6), (6, 8192, 42, 12)),
    "f1": ((3, 3472, 8, 3), (4, 5712, 7, 0), (6, 8192, 14, 0)),
    "f2": ((3, 4048, 9, 3), (4, 6864, 9, 0), (6, 8192, 18, 0)),
    "f3": ((3, 4688, 10, 3), (4, 8144, 11, 0), (6, 8192, 22, 0)),
    "f4": ((3, 4496, 13, 3), (4, 7760, 17, 0), (6, 8192, 34, 0)),
    "f5": ((3, 4368, 17, 3), (4, 7504, 25, 0), (6, 8192, 50, 0)),
    "f6": ((3, 4816, 15, 3), (4, 8192, 21, 0), (6, 8192, 42, 0)),
    "f7": ((3, 4816, 15, 3), (4, 8192, 21, 0), (6, 8192, 42, 0)),
    "f8": ((3, 4816, 14, 3), (4, 8192, 19, 0), (6, 8192, 38, 0)),
    "f9": ((3, 3280, 10, 3), (4, 5328, 11, 0), (6, 8192, 22, 0)),
    "a0": ((3, 4880, 13, 7), (4, 8192, 17, 8), (6, 8192, 34, 16)),
    "a1": ((3, 4688, 10, 3), (4, 8144, 11, 0), (6, 8192, 22, 0)),
    "a2": ((3, 4752, 10, 3), (4, 8192, 11, 0), (6, 8192, 22, 0)),
    "a3": ((3, 4432, 11, 3), (4, 7632, 13, 0), (6, 8192, 26, 0)),
    "a4": ((3, 2704, 9, 3), (4, 4176, 9, 0), (6, 7568, 18, 0)),
    "a5": ((3, 3472, 7, 3), (4, 5712, 5, 0), (6, 8192, 10, 0)),
}
# Every behind and inside tile is staged (records of at most 68 / 123 bytes: 64 of them with their headers
# stay below the cap).  The fixed wrappers' records (2 * (1 + 2 * slice) + 4 bytes, 110-246) make tiles of
# 7040-15744 bytes: only a4's (110 bytes, cap 7568) is staged, the other fifteen read HBM at a fixed stride.


def _slice_options(sid: str):
    source, index = S.SLICE_TABLE[sid][:2]
    if source == "ascii":
        return list(ASCII_CHARSETS) if sid == "a0" else [ASCII_CHARSETS[index % 2]]
    return list(FUZZ_GPU_OPTIONS) if sid in ("f0", "f9") else [FUZZ_GPU_OPTIONS[index % 3]]


def _tag(option) -> str:
    return (option or "default") if isinstance(option, str) else "-".join(option)


def _slice_cases(hows, env=()):
    out = []
    for sid in S.SLICE_TABLE:
        for option in _slice_options(sid):
            for how in hows:
                for k in KERNELS:
                    suffix = "-nostage" if env else ""
                    out.append(Case(f"{sid}-{how}-{_tag(option)}-{k}{suffix}", ("slice", sid, how), option,
                                    "fixed" if how == "fixed" else "rdw", k, env))
    return out


def _slice_want(c: Case):
    depth, cap, nv, ns = SLICE_INFO[c.src[1]][W.WRAPPERS.index(c.src[2])]
    return expect(depth, 0 if c.env else cap, nv, ns, c.kernel)


@pytest.mark.parametrize("c", _ids(_slice_cases(("behind", "inside", "fixed"))))
def test_decoder_slices(c, monkeypatch):
    """Every decoder shape of the fuzz at a data-dependent offset (behind), as an element of an OCCURS of
    groups (inside: slot > 0) and at a fixed stride (fixed: rec_off == nullptr)."""
    check(c, _slice_want(c), monkeypatch)


# ------------------------------------------------------------------------------------------------
# B. dense strings
# ------------------------------------------------------------------------------------------------
# place -> (depth, stage_cap, validity slots, string slots).  behind: records of at most 123 bytes, every tile
# staged; inside: up to 235 bytes, a tile of whole records (15 KiB) reads HBM
DENSE_INFO = {"behind": (3, 8192, 20, 17), "inside": (4, 8192, 31, 28)}


def _dense_cases():
    return [Case(f"{page}-{place}-{trim}-{k}", ("dense", page, place), trim, kernel=k) for page in W.DENSE_PAGES
            for place in W.DENSE_PLACES for trim in W.TRIMS for k in KERNELS]


@pytest.mark.parametrize("c", _ids(_dense_cases()))
def test_dense_strings(c, monkeypatch):
    """PIC X(1..13, 24) of bytes that are half 2- and 3-byte code-page entries: the register path composes
    them across its lo / hi registers, and a wave where one lane's value exceeds 12 UTF-8 bytes takes the
    generic path as a whole.  From the oracle's rows: the input holds waves in which some lane, but not
    every lane, exceeds 12 bytes in a field of at most 12, and waves in which none does."""
    rows, *_ = check(c, expect(*DENSE_INFO[c.src[2]], c.kernel), monkeypatch)
    exp = _expected(c.src, c.option, c.framing, c.shift, c.via)
    mixed = none = 0
    for name in [f"X{n:02d}" for n in range(5, 13)]:
        for e in range(1 if c.src[2] == "behind" else 2):
            for t in range(0, len(exp), 64):
                vals = [r["R"][name] if c.src[2] == "behind" else (r["R"]["ELS"][e][name] if len(r["R"]["ELS"]) > e else None)
                        for r in exp[t:t + 64]]
                over = [len(v.encode("utf-8")) > 12 for v in vals if v is not None]
                mixed += 0 < sum(over) < len(over)
                none += len(over) > 0 and not any(over)
    assert mixed >= 3 and none >= 1, (mixed, none)


# ------------------------------------------------------------------------------------------------
# C. record source
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", _ids(_slice_cases(("behind",), (("CBX_WALK_NO_STAGE", "1"),))))
def test_no_stage_reads_records_from_hbm(c, monkeypatch):
    """Every behind case with CBX_WALK_NO_STAGE=1: the records read through the typed global pointer,
    the same rows, stage_cap 0 reported."""
    _, _, info, _ = check(c, _slice_want(c), monkeypatch)
    assert info["stage_cap"] == 0


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shift", [0, 1, 9, 15])
def test_tiles_straddling_the_stage(shift, kernel, monkeypatch):
    """Consecutive tiles with spans of stage_cap - 2 .. stage_cap + 2 at data-pointer offsets 0, 1, 9 and 15:
    a tile is staged exactly when hi - lo + ((pointer + lo) & 15) <= stage_cap."""
    c = Case(f"straddle-{shift}-{kernel}", ("straddle",), kernel=kernel, shift=shift)
    depth, cap, nv, ns = SLICE_INFO["f1"][0]
    assert cap == STRADDLE_CAP
    tiles = len(STRADDLE_DELTAS) + 1
    _, _, info, (off, ln, ptr) = check(c, expect(depth, cap, nv, ns, kernel, tiles=tiles), monkeypatch)
    recs = _input(c.src, None, "rdw", shift)[3]
    assert ln == [len(r) for r in recs] and ptr % 16 == shift
    spans = []
    for t in range(0, len(off), 64):
        lo = min(off[t:t + 64])
        hi = max(o + n for o, n in zip(off[t:t + 64], ln[t:t + 64]))
        spans.append(hi - lo + ((ptr + lo) & 15))
    assert spans[:-1] == [cap + d for d in STRADDLE_DELTAS]
    staged = [s <= info["stage_cap"] for s in spans]
    assert staged.count(True) == 7 and staged.count(False) == 4    # six tiles at or below the cap and the last; four above


# ------------------------------------------------------------------------------------------------
# D. validity words
# ------------------------------------------------------------------------------------------------
NESTED_INFO = (6, 6352, 38, 17)
WIDE_INFO = (4, 8192, 1207, 363)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("which", ["inside", "nested"])
def test_global_atomics_by_environment(which, kernel, monkeypatch):
    env = (("CBX_WALK_GLOBAL_ATOMICS", "1"),)
    if which == "inside":
        c = Case(f"atomics-f4-inside-{kernel}", ("slice", "f4", "inside"), FUZZ_GPU_OPTIONS[1], kernel=kernel, env=env)
        depth, cap, nv, ns = SLICE_INFO["f4"][1]
    else:
        c = Case(f"atomics-nested-{kernel}", ("nested",), kernel=kernel, env=env)
        depth, cap, nv, ns = NESTED_INFO
    check(c, expect(depth, cap, nv, ns, kernel, vlds=0), monkeypatch)


@pytest.mark.parametrize("kernel", KERNELS)
def test_global_atomics_by_size(kernel, monkeypatch):
    """OCCURS 120 of a 10-field group behind an ODO: more than 8 KiB of words a wave, so vlds == 0 without
    the variable set; the records (2285 bytes) are wider than the stage, so every tile reads HBM."""
    c = Case(f"wide-{kernel}", ("wide",), kernel=kernel)
    depth, cap, nv, ns = WIDE_INFO
    assert 8 * nv + 4 * ns > 8192 and cap == 8192
    check(c, expect(depth, cap, nv, ns, kernel, vlds=0, tiles=3), monkeypatch)


# ------------------------------------------------------------------------------------------------
# E. selection source
# ------------------------------------------------------------------------------------------------
SEGSEL_INFO = (4, 6352, 20, 3)


@pytest.mark.parametrize("kernel", KERNELS)
def test_selection_source_with_segment_redefine(kernel, monkeypatch):
    """A whole-file read: select, then cbx_decode_selected -- the walk takes Record_Id and the active
    segment from the selection (rec_id, rec_seg), not from the segment map."""
    c = Case(f"segsel-{kernel}", ("segsel",), kernel=kernel, via="read")
    rows, *_ = check(c, expect(*SEGSEL_INFO, kernel), monkeypatch)
    assert [r["Record_Id"] for r in rows] == list(range(W.N_REC))


# ------------------------------------------------------------------------------------------------
# F. random layouts: seed -> (depth, stage_cap, validity slots, string slots)
# ------------------------------------------------------------------------------------------------
RANDOM_INFO: Dict[int, Tuple[int, int, int, int]] = {
    0: (8, 8192, 91, 19), 1: (4, 2384, 19, 7), 2: (5, 8192, 19, 9), 3: (4, 5584, 17, 3), 4: (5, 5712, 36, 11),
    5: (8, 8192, 73, 12), 6: (8, 8192, 234, 65), 7: (8, 8192, 135, 17), 8: (8, 8192, 81, 21), 9: (6, 8192, 32, 0),
    10: (8, 8192, 97, 17), 11: (8, 8192, 78, 18), 12: (8, 8192, 76, 10), 13: (3, 2384, 11, 2), 14: (4, 5776, 17, 5),
    15: (4, 6800, 25, 7), 16: (6, 8192, 67, 6), 17: (4, 6608, 27, 6), 18: (8, 8192, 103, 6), 19: (6, 5584, 21, 3),
    20: (7, 8192, 95, 8), 21: (8, 8192, 108, 51), 22: (4, 8192, 45, 12), 23: (6, 8192, 63, 19),
}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("seed", W.SEEDS)
def test_random_layout_rdw(seed, kernel, monkeypatch):
    c = Case(f"random-{seed}-rdw-{kernel}", ("random", seed), kernel=kernel)
    check(c, expect(*RANDOM_INFO[seed], kernel), monkeypatch)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("chunk", ["32", None])
@pytest.mark.parametrize("seed", W.SEEDS)
def test_random_layout_var_occurs_framing(seed, chunk, kernel, monkeypatch):
    """Back to back: VarOccursRecordExtractor framing on the GPU (walk_length / jit_chain_source; 32-byte
    chunks make every chain cross many speculated entries) must find the generator's lengths."""
    env = (("CBX_CHAIN_CHUNK", chunk),) if chunk else ()
    c = Case(f"random-{seed}-b2b-{chunk}-{kernel}", ("random", seed), framing="b2b", kernel=kernel, env=env)
    _, rd, _, (off, ln) = check(c, expect(*RANDOM_INFO[seed], kernel), monkeypatch)
    assert _frame_kind(rd) == (1 if kernel == "jit" else 0)
    recs = _input(c.src, None, "b2b")[3]
    assert ln == [len(r) for r in recs]
    assert off == [sum(ln[:i]) for i in range(len(ln))]


# ------------------------------------------------------------------------------------------------
# G. limits
# ------------------------------------------------------------------------------------------------
DEEP_OK = 14          # nested groups whose frame stack is kWalkDepth = 16 deep
DEEP_INFO = (16, 1168, 6, 1)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("framing", ["rdw", "b2b"])
def test_deepest_accepted_nesting_decodes(framing, kernel, monkeypatch):
    c = Case(f"deep-{framing}-{kernel}", ("deep", DEEP_OK), framing=framing, kernel=kernel)
    _, _, info, fr = check(c, expect(*DEEP_INFO, kernel), monkeypatch)
    assert info["depth"] == 16
    if framing == "b2b":
        assert fr[1] == [len(r) for r in _input(c.src, None, "b2b")[3]]


def test_one_level_deeper_is_refused():
    text, p, *_ = _input(("deep", DEEP_OK + 1), None, "rdw")
    with pytest.raises(N.CbxError, match="the copybook nests 17 levels, above 16") as e:
        VarLenNestedReader(text, p)
    assert e.value.code == N.CBX_E_UNSUPPORTED


def test_walk_info_needs_a_walk():
    """CBX_E_STATE when the plan's last decode call was not a record walk (here: none yet, then a staged decode)."""
    text = S.MIX
    rd = FixedLenNestedReader(text, ReaderParameters(ebcdic_code_page="cp037", jit_min_records=-1))
    assert not rd.walk
    for _ in range(2):
        with pytest.raises(N.CbxError) as e:
            N.walk_info(rd.native.handle)
        assert e.value.code == N.CBX_E_STATE
        rd.decode(S.fixed_file(rd.copybook, 10, 1))
