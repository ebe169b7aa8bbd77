"""Measure column projection: the projected plan on the staged decode kernels and on the direct kernel
(cbx_gather.h) against the unprojected decode of the same batch.

Workloads: SYN200 (fixed-length, the C2 batch) and rdw_narrow_large (RDW multisegment, the C4 batch), string
columns in the view layout (the one layout the direct kernel writes).
Projections: SYN200 -- a ladder of 1, 2, 4, 8, 16 and all fields taken in a fixed seeded order that mixes the
decoder kinds, and the 3-field query REC-ID, AMT-01, NAME; rdw_narrow_large -- COMPANY-ID alone, then with
COMPANY-NAME + PHONE-NUMBER.

Per case, in one process on one GPU, into preallocated columns, HIP events on the stream around each call:
  * the unprojected decode (the unchanged call),
  * the projected plan on the staged kernels (direct_decode = 0),
  * the projected plan on the direct kernel (direct_decode = 1) -- the two projected legs run alternately,
  * the bytes of column buffers each allocates, and the projection's byte share of the record.
Every figure is the median of --steps repetitions after --warmup.  One JSON line per case on stdout (and
appended to --out); the last line is the summary with two expectations checked (reported, not gates):
  (1) the staged 3-field read is faster than the unprojected decode,
  (2) direct beats staged at one field,
the crossover share per workload (where direct and staged take the same time, linear interpolation between
the measured shares), and `direct_max_share`: the largest measured share S at which direct won on every
workload measured -- every workload has a measured case at or below S, and at each of those direct took at
most 0.9 of the staged time (null: no such share; the reader's rule then never picks the direct kernel).
"""
from __future__ import annotations

import argparse
import ctypes
import dataclasses
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cobrix_amd import native as N  # noqa: E402
from cobrix_amd import synth  # noqa: E402
from cobrix_amd.plan import project_columns  # noqa: E402
from cobrix_amd.reader import (FixedLenNestedReader, ReaderParameters, VarLenNestedReader, _alloc_columns,  # noqa: E402
                               projection_share, string_capacity)

LADDER = (1, 2, 4, 8, 16)
LADDER_SEED = 20261019
WIN = 0.9    # direct must take at most this share of the staged time


def leaf_names(cb):
    def walk(g):
        for c in g.children:
            if hasattr(c, "children"):
                yield from walk(c)
            elif not c.is_filler:
                yield c.name
    return list(walk(cb.ast))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def medians(fns, steps, warmup):
    """Median ms of each fn, the fns run alternately (a, b, a, b, ...) after `warmup` rounds."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            ms[k].append(timed(fn))
    return [statistics.median(m) for m in ms]


def column_bytes(cols):
    return sum(v.numel() * v.element_size() for c in cols for v in c.values() if torch.is_tensor(v))


class Leg:
    """One reader's decode plan with its columns allocated once."""

    def __init__(self, work, columns, direct):
        p = work.params if columns is None else dataclasses.replace(work.params, direct_decode=direct)
        self.rd = work.make(p, columns)
        self.work = work
        self.native = self.rd.out_native
        self.cols, self.cs = _alloc_columns(self.rd.out_plan, work.n_rec, string_capacity(self.native, work.n_rec), work.dev)
        self.bytes = column_bytes(self.cols)

    def __call__(self):
        w, L, sp = self.work, self.work.L, ctypes.c_void_p(self.work.st.cuda_stream)
        if w.stride:
            N.check(L.cbx_decode_fixed(self.native.handle, w.data.data_ptr(), w.n_rec, w.stride, 0, 0, self.cs, sp))
        else:
            N.check(L.cbx_decode_var(self.native.handle, w.data.data_ptr(), w.n_bytes, w.off.data_ptr(), w.ln.data_ptr(),
                                     w.n_rec, 0, 0, self.cs, sp))

    def kind(self):
        k = ctypes.c_int32(-1)
        N.check(self.work.L.cbx_plan_kernel_kind(self.native.handle, ctypes.byref(k)))
        return k.value

    def check(self):
        N.check(self.work.L.cbx_plan_check(self.native.handle, ctypes.c_void_p(self.work.st.cuda_stream)))

    def close(self):
        self.rd.close()


class Work:
    """One batch resident in HBM."""

    def __init__(self, name, n_rec, dev):
        self.name, self.dev, self.L = name, dev, N.load()
        self.st = torch.cuda.current_stream()
        if name == "syn200":
            self.params = ReaderParameters(string_views=True)
            self.make = lambda p, cols: FixedLenNestedReader(synth.SYN200_COPYBOOK, p, columns=cols)
            self.data = synth.syn200(n_rec, seed=20261015, device=dev).view(-1)
            self.n_bytes, self.n_rec, self.stride = int(self.data.numel()), n_rec, synth.SYN200_RECORD_SIZE
            self.off = self.ln = None
            rd = self.make(self.params, None)
            names = leaf_names(rd.copybook)
            rd.close()
            order = random.Random(LADDER_SEED).sample(names, len(names))
            self.cases = [(f"ladder_{k}", order[:k]) for k in LADDER] + [(f"ladder_all_{len(names)}", order),
                                                                         ("query3", ["REC-ID", "AMT-01", "NAME"])]
        else:
            self.params = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID", generate_record_id=True,
                                           string_views=True,
                                           segment_id_redefine_map={k: v for k, v in synth.RDW_NARROW_SEGMENTS.items()})
            self.make = lambda p, cols: VarLenNestedReader(synth.RDW_NARROW_COPYBOOK, p, columns=cols)
            size = synth.rdw_narrow_large_size(n_rec, device=dev)
            buf = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
            self.data, _ = synth.rdw_narrow_large(n_rec, device=dev, out=buf)
            self.n_bytes, self.stride = size, 0
            rd = self.make(self.params, None)
            self.off, self.ln = rd.frame(self.data, size)
            rd.close()
            self.n_rec = int(self.off.numel())
            self.cases = [("company_id", ["COMPANY-ID"]), ("id_name_phone", ["COMPANY-ID", "COMPANY-NAME", "PHONE-NUMBER"])]


def run(work: Work, steps: int, warmup: int, emit):
    full = Leg(work, None, False)
    rows = []
    for case, cols in work.cases:
        staged, direct = Leg(work, cols, False), Leg(work, cols, True)
        full_ms, = medians([full], steps, warmup)
        staged_ms, direct_ms = medians([staged, direct], steps, warmup)
        for leg in (full, staged, direct):
            leg.check()
        cb = staged.rd.copybook
        row = {"workload": work.name, "case": case, "records": work.n_rec, "input_bytes": work.n_bytes, "columns": cols,
               "n_fields": len(project_columns(cb, cols)),
               "byte_share": round(projection_share(cb, project_columns(cb, cols)), 4),
               "unprojected_ms": round(full_ms, 4), "staged_ms": round(staged_ms, 4), "direct_ms": round(direct_ms, 4),
               "direct_over_staged": round(direct_ms / staged_ms, 4),
               "kernel_kind": {"unprojected": full.kind(), "staged": staged.kind(), "direct": direct.kind()},
               "column_bytes": {"unprojected": full.bytes, "staged": staged.bytes, "direct": direct.bytes}}
        emit(row)
        rows.append(row)
        staged.close()
        direct.close()
        del staged, direct
        torch.cuda.empty_cache()
    full.close()
    return rows


def crossover(rows):
    """Byte share at which direct and staged take the same time (None: direct is faster at every measured
    share; 0.0: at none)."""
    pts = sorted((r["byte_share"], r["direct_ms"] - r["staged_ms"]) for r in rows)
    if pts[0][1] >= 0:
        return 0.0
    for (s0, d0), (s1, d1) in zip(pts, pts[1:]):
        if d0 < 0 <= d1:
            return round(s0 + (s1 - s0) * (-d0) / (d1 - d0), 4)
    return None


def direct_max_share(all_rows):
    """The largest measured share S at which direct won on every workload measured: every workload has a
    measured case at or below S, and at each of those direct took at most WIN of the staged time."""
    best = None
    loads = {r["workload"] for r in all_rows}
    for s in sorted({r["byte_share"] for r in all_rows}):
        below = [r for r in all_rows if r["byte_share"] <= s]
        if {r["workload"] for r in below} == loads and all(r["direct_ms"] <= WIN * r["staged_ms"] for r in below):
            best = s
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="syn200,rdw_narrow_large")
    ap.add_argument("--records", type=int, default=0, help="records per batch (default: 50M SYN200 = the C2 batch, 37.5M RDW = the C4 batch)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_project.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    emit({"tool": "bench_project", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup})
    summary = {"case": "summary", "win_ratio": WIN}
    all_rows = []
    for name in args.workloads.split(","):
        n = args.records or {"syn200": 50_000_000, "rdw_narrow_large": 37_500_000}[name]
        work = Work(name, n, dev)
        rows = run(work, args.steps, args.warmup, emit)
        all_rows += rows
        one = min(rows, key=lambda r: (r["n_fields"], r["byte_share"]))
        summary[name] = {"direct_beats_staged_at_one_field": one["direct_ms"] < one["staged_ms"],
                         "one_field_case": one["case"], "crossover_share": crossover(rows)}
        q3 = [r for r in rows if r["case"] == "query3"]
        if q3:
            summary[name]["staged_3_field_faster_than_unprojected"] = q3[0]["staged_ms"] < q3[0]["unprojected_ms"]
        del work
        torch.cuda.empty_cache()
    summary["direct_max_share"] = direct_max_share(all_rows)
    emit(summary)


if __name__ == "__main__":
    main()
