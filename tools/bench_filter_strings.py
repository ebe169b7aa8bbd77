"""Measure the suffix / substring filter ops (StringContains, StringEndsWith) of the row-filter stage.

Workloads: SYN200 `NAME` (fixed-length, the C2 batch) and rdw_narrow_large `COMPANY-NAME` (RDW multisegment, the
C4 batch).  Cases per workload: StringContains with a 1-, 2- and 4-byte literal and StringEndsWith with a 1-byte
literal; the measured selectivity is reported.  Two comparisons in the same process on the same batch:
  * the test pass of StringStartsWith on the same field (the string term the stage had before);
  * the projected decode of that one string column over all rows (a reader with columns=[field]): the least any
    evaluation that is not pushed down can cost before it has compared a single value.
Per case: test / scan / emit pass times (HIP events recorded by the library, cbx_filter_pass_times), the whole
filter call, and filter + cbx_decode_selected of the projected column (events around both calls; the filter
call returns the surviving count to the host in between: that wait is part of the figure).
Every figure is the median of --steps repetitions after --warmup.  One JSON line per case on stdout (and
appended to --out); the last line is the summary: whether each test pass stays below the projected decode and
whether filter + selected decode beats it (reported, not gated).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd import synth  # noqa: E402
from cobrix_amd.reader import (FixedLenNestedReader, ReaderParameters, VarLenNestedReader, _alloc_columns,  # noqa: E402
                               string_capacity)

FIELD = {"syn200": "NAME", "rdw_narrow_large": "COMPANY-NAME"}


def cases(field):
    """Both fields hold cp037 letters and digits."""
    return [("starts_with_1", F.StringStartsWith(field, "A")), ("contains_1", F.StringContains(field, "A")),
            ("contains_2", F.StringContains(field, "AB")), ("contains_4", F.StringContains(field, "ABCD")),
            ("ends_with_1", F.StringEndsWith(field, "A")), ("not_contains_1", F.Not(F.StringContains(field, "A")))]


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


class Work:
    """One batch resident in HBM with a reader projected on the one string column."""

    def __init__(self, name, n_rec, dev):
        self.name, self.field = name, FIELD[name]
        L = self.L = N.load()
        if name == "syn200":
            self.rd = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters(string_views=True), columns=[self.field])
            self.data = synth.syn200(n_rec, seed=20261015, device=dev).view(-1)
            self.n_bytes, self.n_rec, self.stride = int(self.data.numel()), n_rec, synth.SYN200_RECORD_SIZE
            self.off = self.ln = None
        else:
            p = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID", string_views=True,
                                 segment_id_redefine_map={k: v for k, v in synth.RDW_NARROW_SEGMENTS.items()})
            self.rd = VarLenNestedReader(synth.RDW_NARROW_COPYBOOK, p, columns=[self.field])
            size = synth.rdw_narrow_large_size(n_rec, device=dev)
            buf = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
            self.data, _ = synth.rdw_narrow_large(n_rec, device=dev, out=buf)
            self.n_bytes, self.stride = size, 0
            self.off, self.ln = self.rd.frame(self.data, size)
            self.n_rec = int(self.off.numel())
        self.h = self.rd.native.handle            # the full plan: the filter stage
        self.ho = self.rd.out_native.handle       # the projected plan: the decode calls
        self.st = torch.cuda.current_stream()
        self.cols, self.cs = _alloc_columns(self.rd.out_plan, self.n_rec, string_capacity(self.rd.out_native, self.n_rec), dev)
        N.check(L.cbx_plan_set_profiling(self.h, 1))

    def projected_decode(self):
        L, sp = self.L, ctypes.c_void_p(self.st.cuda_stream)
        if self.stride:
            N.check(L.cbx_decode_fixed(self.ho, self.data.data_ptr(), self.n_rec, self.stride, 0, 0, self.cs, sp))
        else:
            N.check(L.cbx_decode_var(self.ho, self.data.data_ptr(), self.n_bytes, self.off.data_ptr(), self.ln.data_ptr(),
                                     self.n_rec, 0, 0, self.cs, sp))

    def filter(self, table):
        return self.rd._filter_records(table, self.data, self.n_bytes, self.n_rec, self.st, rec_off=self.off,
                                       rec_len=self.ln, stride=self.stride)

    def pass_times(self):
        t = [ctypes.c_float(0) for _ in range(3)]
        N.check(self.L.cbx_filter_pass_times(self.h, *[ctypes.byref(x) for x in t]))
        return [x.value for x in t]

    def drain_kernel_times(self):
        for h in (self.h, self.ho):
            n = ctypes.c_int32(0)
            N.check(self.L.cbx_plan_kernel_times(h, None, None, 0, ctypes.byref(n)))


def run(work: Work, steps: int, warmup: int, emit):
    dev = work.data.device
    proj_ms = median_ms(work.projected_decode, steps, warmup)
    N.check(work.L.cbx_plan_check(work.ho, ctypes.c_void_p(work.st.cuda_stream)))
    work.drain_kernel_times()
    emit({"workload": work.name, "case": "projected_decode", "column": work.field, "records": work.n_rec,
          "input_bytes": work.n_bytes, "decode_ms": round(proj_ms, 4)})
    results = []
    for kind, flt in cases(work.field):
        table, unhandled = F.compile_filters(work.rd.plan, [flt])
        assert table is not None and not unhandled, unhandled.reasons
        row = {"workload": work.name, "case": kind, "column": work.field,
               "literal_bytes": int(table.literals[0].str_len)}
        sel = work.filter(table)
        n_sel = sel["n"]
        row["selectivity"] = round(n_sel / work.n_rec, 5)
        passes = []

        def only_filter():
            work.filter(table)
            passes.append(work.pass_times())

        flt_ms = median_ms(only_filter, steps, warmup)
        test, scan, em = (statistics.median(p[k] for p in passes[-steps:]) for k in range(3))
        row["filter"] = {"filter_call_ms": round(flt_ms, 4), "test_ms": round(test, 4), "scan_ms": round(scan, 4),
                         "emit_ms": round(em, 4), "stage_ms": round(test + scan + em, 4)}
        cols, cs = _alloc_columns(work.rd.out_plan, n_sel, string_capacity(work.rd.out_native, n_sel), dev)

        def filter_and_decode():
            s = work.filter(table)
            N.check(work.L.cbx_decode_selected(work.ho, work.data.data_ptr(), work.n_bytes, ctypes.byref(s["struct"]), s["n"], 0,
                                               cs, ctypes.c_void_p(work.st.cuda_stream)))

        row["filter_plus_selected_decode_ms"] = round(median_ms(filter_and_decode, steps, warmup), 4)
        N.check(work.L.cbx_plan_check(work.ho, ctypes.c_void_p(work.st.cuda_stream)))
        work.drain_kernel_times()
        row["projected_decode_ms"] = round(proj_ms, 4)
        del cols, cs, sel
        emit(row)
        results.append(row)
    return proj_ms, results


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="syn200,rdw_narrow_large")
    ap.add_argument("--records", type=int, default=0, help="records per batch (default: 50M SYN200 = the C2 batch, 37.5M RDW = the C4 batch)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter_strings.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(s + "\n")

    emit({"tool": "bench_filter_strings", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
          "filter_max_op": N.load().cbx_filter_max_op()})
    summary = {"case": "summary"}
    for name in args.workloads.split(","):
        n = args.records or {"syn200": 50_000_000, "rdw_narrow_large": 37_500_000}[name]
        work = Work(name, n, dev)
        proj_ms, rows = run(work, args.steps, args.warmup, emit)
        starts = next(r for r in rows if r["case"] == "starts_with_1")["filter"]["test_ms"]
        summary[name] = {
            "projected_decode_ms": round(proj_ms, 4),
            "starts_with_test_ms": starts,
            "test_ms": {r["case"]: r["filter"]["test_ms"] for r in rows},
            "test_pass_below_projected_decode": {r["case"]: r["filter"]["test_ms"] < proj_ms for r in rows},
            "filter_first_beats_projected_decode": {r["case"]: r["filter_plus_selected_decode_ms"] < proj_ms for r in rows}}
        work.rd.close()
        del work
        torch.cuda.empty_cache()
    emit(summary)


if __name__ == "__main__":
    main()
