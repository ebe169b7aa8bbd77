"""GPU: every decoder shape and every tile geometry through every staging loop of the decode kernel.

The decode kernel stages a tile's records into LDS in one of three ways (cbx_capi.hip launch()):
contiguous (contig_loop, coop_loop; plain rows or rows padded to an odd dword pitch), span (span_loop:
variable-length records, the specialised kernel) and windowed (stage_window; fields wider than a window
read from HBM through the global window).  Every case decodes through the readers, compares the whole
batch with the oracle and asserts the launch the library reports (cbx_plan_launch_info) against the
values written here: a dispatch change that moves a case to another path fails it instead of silently
taking its coverage away.

  A  every shape, fixed length: the slices of the decoder fuzz's two copybooks (staging_cases.py)
  B  every geometry: a 16-byte and a 4-byte copybook at every contiguous stride, pointer offset and
     record counts around a tile and a run of tiles
  C  a wave's second run of tiles (the prefetch chain across loop iterations)
  D  every shape, variable length: span staging, its overflow to record windows, 16-byte windows
  E  the string slices in the string-view and Arrow Utf8 layouts, with the Utf8 count pass

Run on an MI355X: python -u -m pytest tests/test_gpu_staging.py -m gpu -x -v
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field
from typing import Dict

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import staging_cases as S  # noqa: E402
from parity import compare_batch  # noqa: E402

from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.reader import (FixedLenNestedReader, ReaderParameters, VarLenNestedReader,  # noqa: E402
                               parse_copybook_for)
from oracle import oracle as O  # noqa: E402

N_REC = 1089        # two full runs of 8 tiles + a tile of one record
TILES = 18          # tiles of 64 records in N_REC


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------
# The launch each slice is expected to report, written out (the strides are in S.SLICE_TABLE):
#   kp plain / kp padded: 16-byte chunks per lane at the plain / padded contiguous stride
#   coop: the specialised contiguous kernel, as dispatched, runs cooperative tiles
#   windows16 / global16: windows of the windowed op set at window_bytes = 16 / whether fields wider
#       than 16 bytes sit in its global window (f1 and a5 hold such fields only: one window, the global)
#   span kp: chunks per lane of the span staging
# ------------------------------------------------------------------------------------------------
SLICE_LAUNCH = {
    #      kp plain, kp padded, coop, windows16, global16, span kp
    "f0": (4, 5, 1, 5, 0, 5),
    "f1": (3, 4, 1, 1, 1, 3),
    "f2": (4, 4, 1, 2, 1, 4),
    "f3": (4, 5, 1, 2, 1, 5),
    "f4": (4, 5, 1, 5, 0, 4),
    "f5": (4, 5, 1, 4, 0, 4),
    "f6": (4, 5, 1, 5, 0, 5),
    "f7": (4, 5, 1, 5, 0, 5),
    "f8": (4, 5, 1, 4, 1, 5),
    "f9": (3, 4, 1, 3, 1, 3),
    "a0": (4, 5, 1, 4, 1, 5),
    "a1": (4, 5, 1, 3, 1, 5),
    "a2": (4, 5, 1, 2, 1, 5),
    "a3": (4, 5, 1, 3, 1, 4),
    "a4": (2, 3, 1, 2, 0, 3),
    "a5": (3, 4, 0, 1, 1, 3),   # a single field: nothing to split between two waves
}

# stride in dwords -> (kp, padded rows) of the contiguous staging, stride_dw 1..63
SWEEP = {
    1: (1, 0), 2: (1, 0), 3: (1, 0), 4: (2, 1), 5: (2, 0), 6: (2, 0), 7: (2, 0), 8: (3, 1), 9: (3, 0),
    10: (3, 0), 11: (3, 0), 12: (4, 1), 13: (4, 0), 14: (4, 0), 15: (4, 0), 16: (5, 1), 17: (5, 0),
    18: (5, 0), 19: (5, 0), 20: (6, 1), 21: (6, 0), 22: (6, 0), 23: (6, 0), 24: (7, 1), 25: (7, 0),
    26: (7, 0), 27: (7, 0), 28: (8, 1), 29: (8, 0), 30: (8, 0), 31: (8, 0), 32: (9, 1), 33: (9, 0),
    34: (9, 0), 35: (9, 0), 36: (10, 1), 37: (10, 0), 38: (10, 0), 39: (10, 0), 40: (11, 1), 41: (11, 0),
    42: (11, 0), 43: (11, 0), 44: (12, 1), 45: (12, 0), 46: (12, 0), 47: (12, 0), 48: (13, 1), 49: (13, 0),
    50: (13, 0), 51: (13, 0), 52: (14, 1), 53: (14, 0), 54: (14, 0), 55: (14, 0), 56: (15, 1), 57: (15, 0),
    58: (15, 0), 59: (15, 0), 60: (16, 1), 61: (16, 0), 62: (16, 0), 63: (16, 0),
}

EBCDIC_KW = dict(ebcdic_code_page="cp037", string_trimming_policy="both", floating_point_format="IBM")
VARIANT_KW = {"": {}, "ieee": dict(floating_point_format="IEEE754"), "le": dict(floating_point_format="IBM_LE")}
LAYOUT_KW = {"large": {}, "views": dict(string_views=True), "utf8": dict(string_utf8=True)}
KERNEL_JIT = {"table": -1, "spec": 1, "nocoop": 1}   # jit_min_records; nocoop: CBX_NO_COOP=1 as well


@dataclass(frozen=True)
class Case:
    id: str
    cb: str                      # a slice of S.SLICE_TABLE, "MIX" or "TINY"
    expect: Dict[str, int] = field(hash=False, compare=False, default_factory=dict)
    kernel: str = "table"        # table / spec / nocoop
    start: int = 0               # record start offset
    end: int = 0                 # record end offset
    shift: int = 0               # data pointer & 15
    n: int = N_REC
    window: int = 0              # ReaderParameters.window_bytes
    layout: str = "large"
    variant: str = ""            # floating-point format of the float slice
    var: str = ""                # "": fixed length; "rdw": RDW records; "long": with overflowing tiles
    max_blocks: int = 0          # CBX_MAX_BLOCKS_PER_CU


def _source(c: Case):
    """(copybook text, reader keywords, ASCII data) of a case."""
    if c.cb in ("MIX", "TINY"):
        return getattr(S, c.cb), dict(EBCDIC_KW), False
    if S.SLICE_TABLE[c.cb][0] == "ascii":
        return S.slice_text(c.cb), dict(is_ebcdic=False), True
    return S.slice_text(c.cb), {**EBCDIC_KW, **VARIANT_KW[c.variant]}, False


def _seed(cb: str) -> int:
    return zlib.crc32(cb.encode()) % 100000


@functools.lru_cache(maxsize=None)
def _fixed_input(cb: str, variant: str, n: int, start: int, end: int):
    """(file bytes, oracle result) -- shared by the kernels, pointer offsets and layouts; never modified."""
    text, kw, ascii = _source(Case("", cb, variant=variant))
    book = parse_copybook_for(text, ReaderParameters(start_offset=start, end_offset=end, **kw))
    data = S.fixed_file(book, n, _seed(cb), start, end, ascii)
    return data, O.decode_fixed(book, data, record_size=book.record_size, start_offset=start, end_offset=end)


@functools.lru_cache(maxsize=None)
def _var_input(cb: str, long_every: int):
    text, kw, ascii = _source(Case("", cb))
    book = parse_copybook_for(text, ReaderParameters(is_record_sequence=True, **kw))
    raw, recs = S.rdw_file(book, N_REC, _seed(cb) + 1, ascii, long_every)
    return raw, O.decode_records(book, recs)


def _seen_by(rd, res):
    """The shared oracle result for this reader: compare_batch finds a column's oracle node by the identity
    of the reader's copybook statement; the events name nodes by their number in walk order."""
    ast = O.OracleAst(rd.copybook)
    assert len(ast.stmts) == len(res.ast.stmts)
    return O.OracleResult(ast, res.events, res.heap, res.n_rec)


def _device(data: bytes, shift: int):
    """The file on the GPU, `shift` bytes past a 16-byte boundary."""
    buf = torch.zeros(shift + len(data) + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf[shift:shift + len(data)]


INFO_FIELDS = [n for n, _ in N.CbxLaunchInfo._fields_ if n != "reserved"]


def run_case(c: Case, setenv):
    """Decode the case; (launch info as a dict, mismatches against the oracle)."""
    if c.kernel == "nocoop":
        setenv("CBX_NO_COOP", "1")
    if c.max_blocks:
        setenv("CBX_MAX_BLOCKS_PER_CU", str(c.max_blocks))
    text, kw, _ = _source(c)
    kw.update(LAYOUT_KW[c.layout], jit_min_records=KERNEL_JIT[c.kernel], window_bytes=c.window)
    if c.var:
        raw, res = _var_input(c.cb, 5 if c.var == "long" else 0)
        rd = VarLenNestedReader(text, ReaderParameters(is_record_sequence=True, **kw))
        t = _device(raw, c.shift)
        off, ln = rd.frame(t, len(raw))
        batch = rd.decode_device(t, len(raw), off, ln)
    else:
        data, res = _fixed_input(c.cb, c.variant, c.n, c.start, c.end)
        rd = FixedLenNestedReader(text, ReaderParameters(start_offset=c.start, end_offset=c.end, **kw))
        assert rd.get_record_size() * c.n == len(data)
        batch = rd.decode_device(_device(data, c.shift), len(data))
    li = N.launch_info(rd.native.handle)
    info = {n: int(getattr(li, n)) for n in INFO_FIELDS}
    return info, compare_batch(batch, _seen_by(rd, res))


def check(c: Case, monkeypatch):
    info, errs = run_case(c, monkeypatch.setenv)
    print(c.id, info)
    assert not errs, errs[:8]
    want = dict(c.expect)
    if "grid" not in want:
        want["grid"] = want["blocks_needed"]     # small batches: every tile's workgroup is launched
    assert {k: info[k] for k in want} == want, info
    assert set(want) == set(INFO_FIELDS)


# ------------------------------------------------------------------------------------------------
# expectation rows
# ------------------------------------------------------------------------------------------------
def _blocks(tiles: int, coop: int) -> int:
    return tiles if coop else (tiles + 1) // 2   # a workgroup per tile / a wave of a two-wave workgroup per tile


def contig(kernel: str, kp: int, padded: int, coop_as_dispatched: int, shift: int = 0, tiles: int = TILES, count: int = 0):
    coop = 1 if kernel == "spec" and coop_as_dispatched else 0
    return dict(kind=0 if kernel == "table" else 1, staging=1, coop=coop, kp=kp, padded_rows=padded, n_windows=1,
                global_window=0, count_kernel=count, base_shift=shift, blocks_needed=_blocks(tiles, coop))


def windowed(kernel: str, shift: int = 0, n_windows: int = 1, global_window: int = 0, count: int = 0):
    return dict(kind=0 if kernel == "table" else 1, staging=0, coop=0, kp=0, padded_rows=0, n_windows=n_windows,
                global_window=global_window, count_kernel=count, base_shift=shift, blocks_needed=_blocks(TILES, 0))


def span(kp: int, count: int = 0):
    return dict(kind=1, staging=2, coop=0, kp=kp, padded_rows=0, n_windows=1, global_window=0, count_kernel=count,
                base_shift=0, blocks_needed=_blocks(TILES, 0))


def _ids(cases):
    assert len({c.id for c in cases}) == len(cases)
    return [pytest.param(c, id=c.id) for c in cases]


# ------------------------------------------------------------------------------------------------
# A. every shape, fixed length
# ------------------------------------------------------------------------------------------------
def _shape_cases():
    out = []
    for sid, (_, _, size, plain, padded) in S.SLICE_TABLE.items():
        kp_plain, kp_padded, coop, win16, glob16, _ = SLICE_LAUNCH[sid]
        for v in (["", "ieee", "le"] if sid == "f9" else [""]):
            tag = sid + ("-" + v if v else "")
            for rows, stride, kp, pad in (("plain", plain, kp_plain, 0), ("padded", padded, kp_padded, 1)):
                for k in ("table", "spec", "nocoop"):
                    out.append(Case(f"{tag}-{rows}-{k}", sid, contig(k, kp, pad, coop), k, end=stride - size, variant=v))
            # ContigSpan::mis_dw 1, 3 (padded rows) and 2 (plain rows)
            for shift, rows, stride, kp, pad in ((4, "padded", padded, kp_padded, 1), (12, "padded", padded, kp_padded, 1),
                                                 (8, "plain", plain, kp_plain, 0)):
                out.append(Case(f"{tag}-{rows}-ptr{shift}", sid, contig("table", kp, pad, coop, shift), end=stride - size,
                                shift=shift, variant=v))
            # windowed by stride: start offsets 1, 2, 3 with stride % 4 = 1, 2, 3 -- every field alignment
            for start in (1, 2, 3):
                end = -size % 4
                assert (start + size + end) % 4 == start
                for k in (("table", "spec") if start == 1 else ("table",)):
                    out.append(Case(f"{tag}-win-start{start}-{k}", sid, windowed(k), k, start=start, end=end, variant=v))
            # windows cut at 16 bytes, a pointer 9 bytes past a 16-byte boundary
            for k in ("table", "spec"):
                out.append(Case(f"{tag}-win16-{k}", sid, windowed(k, 9, win16, glob16), k, start=1, end=-size % 4, shift=9,
                                window=16, variant=v))
    return out


SHAPE_CASES = _shape_cases()


@pytest.mark.parametrize("c", _ids(SHAPE_CASES))
def test_every_shape_fixed_length(c, monkeypatch):
    """A slice of the fuzz copybooks through the contiguous loops (plain and padded rows; table-driven,
    specialised as dispatched, specialised without cooperative tiles; data pointers 4, 8 and 12 bytes past a
    16-byte boundary) and through the windowed staging (strides of every residue mod 4; 16-byte windows
    with the wider fields in the global window; a0's PIC N(12) is the string read there behind a record
    start offset).  The slices f1, f3 and a1-a5 hold byte-loop-only fields (wide zoned, ASCII numbers):
    the deferred-value pass decodes them from HBM, so they check the dispatch and that pass, while the
    staged image is observed through the other nine slices."""
    check(c, monkeypatch)


def test_shape_table_covers_both_specialised_loops_and_cut_windows():
    spec = [c for c in SHAPE_CASES if c.kernel == "spec" and c.expect["staging"] == 1]
    assert {c.expect["coop"] for c in spec} == {0, 1}            # coop_loop and contig_loop without the knob
    assert {c.cb for c in spec if not c.expect["coop"]} == {"a5"}
    cut = [c for c in SHAPE_CASES if c.window == 16]
    # every slice with a field of at most 16 bytes is cut into several windows; f1 and a5 have none
    assert {c.cb for c in cut if c.expect["n_windows"] == 1} == {"f1", "a5"}
    assert all(c.expect["global_window"] == 1 for c in cut if c.expect["n_windows"] == 1)
    assert {c.cb for c in cut if c.expect["global_window"]} == {"f1", "f2", "f3", "f8", "f9", "a0", "a1", "a2", "a3", "a5"}
    assert {c.shift for c in SHAPE_CASES if c.expect["staging"] == 1} == {0, 4, 8, 12}


# ------------------------------------------------------------------------------------------------
# B. every geometry, small copybooks
# ------------------------------------------------------------------------------------------------
def _geo(sdw: int, kernel: str, shift: int = 0, n: int = N_REC, tag: str = "") -> Case:
    cb, size = ("TINY", 4) if sdw < 4 else ("MIX", 16)
    kp, pad = SWEEP[sdw]
    return Case(f"{cb}-dw{sdw}-{kernel}{tag}", cb, contig(kernel, kp, pad, 1, shift, (n + 63) // 64), kernel,
                end=4 * sdw - size, shift=shift, n=n)


SWEEP_CASES = [_geo(sdw, "table") for sdw in range(1, 64)] + \
              [_geo(sdw, "spec") for sdw in [2, 3] + [d for k in range(2, 17) for d in (4 * (k - 1), 4 * (k - 1) + 1)]]
POINTER_CASES = [_geo(sdw, k, shift, tag=f"-ptr{shift}") for sdw in (5, 8, 63) for k in ("table", "spec")
                 for shift in (0, 4, 8, 12)]
COUNT_CASES = [_geo(sdw, k, n=n, tag=f"-n{n}") for sdw in (8, 13) for k in ("table", "spec")
               for n in (1, 63, 64, 65, 511, 512, 513)]


@pytest.mark.parametrize("c", _ids(SWEEP_CASES))
def test_stride_sweep(c, monkeypatch):
    """Every contiguous stride: 4..252 bytes on the table-driven kernel, and one padded and one plain row
    layout per prefetch depth on the specialised one."""
    check(c, monkeypatch)


@pytest.mark.parametrize("c", _ids(POINTER_CASES))
def test_pointer_offsets(c, monkeypatch):
    """ContigSpan::mis_dw 0..3 at a plain stride, a padded stride and the widest stride."""
    check(c, monkeypatch)


@pytest.mark.parametrize("c", _ids(COUNT_CASES))
def test_record_counts(c, monkeypatch):
    """Record counts around a tile (64) and around a run of 8 tiles (512), padded and plain rows."""
    check(c, monkeypatch)


def test_geometry_tables_cover_every_depth():
    geo = SWEEP_CASES + POINTER_CASES + COUNT_CASES
    for kernel, kind in (("table", 0), ("spec", 1)):
        assert {c.expect["kp"] for c in geo if c.kernel == kernel and c.expect["kind"] == kind} == set(range(1, 17))
    for pad in (0, 1):
        assert {c.expect["kp"] for c in geo if c.expect["padded_rows"] == pad} >= set(range(2, 17))
    assert sorted(4 * sdw for sdw in SWEEP) == list(range(4, 253, 4))
    assert {c.end + (4 if c.cb == "TINY" else 16) for c in SWEEP_CASES if c.kernel == "table"} == set(range(4, 253, 4))


# ------------------------------------------------------------------------------------------------
# C. a wave's second run of tiles
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["table", "spec", "nocoop"])
def test_second_run_of_tiles(kernel, monkeypatch):
    """One resident workgroup per CU and two runs of 8 tiles per wave of it, plus a tile of one record and
    a last tile of 65 - 64: every wave's prefetch chain crosses a loop iteration (MIX at stride 20)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * (cus * 2 * 8 * 64) + 65
    tiles = (n + 63) // 64
    want = contig(kernel, 2, 0, 1, tiles=tiles)
    want["grid"] = cus
    c = Case(f"MIX-dw5-{kernel}-second-run", "MIX", want, kernel, end=4, n=n, max_blocks=1)
    assert want["grid"] < want["blocks_needed"]
    check(c, monkeypatch)


# ------------------------------------------------------------------------------------------------
# D. every shape, variable length
# ------------------------------------------------------------------------------------------------
def _var_cases():
    out = []
    for sid in S.SLICE_TABLE:
        _, _, _, win16, glob16, span_kp = SLICE_LAUNCH[sid]
        out.append(Case(f"{sid}-span", sid, span(span_kp), "spec", var="rdw"))
        out.append(Case(f"{sid}-span-long", sid, span(span_kp), "spec", var="long"))
        out.append(Case(f"{sid}-rdw-win16", sid, windowed("table", 0, win16, glob16), "table", window=16, var="rdw"))
    return out


VAR_CASES = _var_cases()


@pytest.mark.parametrize("c", _ids(VAR_CASES))
def test_every_shape_variable_length(c, monkeypatch):
    """RDW records, 30 % whole and the others cut at every length: the span staging of the specialised
    kernel, and the table-driven kernel over 16-byte windows.  `long`: every fifth tile holds a record of
    300-3000 bytes; such a tile overflows the span staging and falls back to record windows.  The kernel
    decides that per tile on the device, so the fallback cannot be asserted, only its values.
    The files end with their last record, most of them 1-3 bytes into a dword: f6-span-long and
    a0-span-long are the cases whose last bytes then carry a value (contig_issue once lost them)."""
    check(c, monkeypatch)


# ------------------------------------------------------------------------------------------------
# E. string layouts
# ------------------------------------------------------------------------------------------------
def _string_cases():
    out = []
    for sid in ("f0", "a0"):
        _, _, size, plain, padded = S.SLICE_TABLE[sid]
        kp_plain, kp_padded, coop, _, _, span_kp = SLICE_LAUNCH[sid]
        for layout in ("views", "utf8"):
            u = layout == "utf8"
            for k in ("table", "spec"):
                cnt = 0 if not u else 1 if k == "spec" else 2   # the Utf8 count pass: specialised / table-driven
                out.append(Case(f"{sid}-{layout}-plain-{k}", sid, contig(k, kp_plain, 0, coop, count=cnt), k,
                                end=plain - size, layout=layout))
                out.append(Case(f"{sid}-{layout}-padded-{k}", sid, contig(k, kp_padded, 1, coop, count=cnt), k,
                                end=padded - size, layout=layout))
                out.append(Case(f"{sid}-{layout}-win-{k}", sid, windowed(k, count=2 if u else 0), k, start=1,
                                end=-size % 4, layout=layout))
            out.append(Case(f"{sid}-{layout}-span", sid, span(span_kp, 1 if u else 0), "spec", layout=layout, var="rdw"))
            out.append(Case(f"{sid}-{layout}-rdw-table", sid, windowed("table", count=2 if u else 0), "table",
                            layout=layout, var="rdw"))
    return out


STRING_CASES = _string_cases()


@pytest.mark.parametrize("c", _ids(STRING_CASES))
def test_string_layouts(c, monkeypatch):
    """The slices that hold strings (EBCDIC X / A fields; ASCII X and PIC N) in the string-view and Arrow
    Utf8 layouts through both contiguous row layouts, the windowed staging and the span staging.  The Utf8
    layout's count pass is the specialised kernel on contiguous and span staging with the specialised
    decode, the table-driven kernel's mode 1 otherwise."""
    check(c, monkeypatch)
