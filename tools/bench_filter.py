"""Measure the row-filter stage (cbx_filter_records) against the unfiltered decode of the same batch.

Workloads: SYN200 (fixed-length, the C2 batch) and rdw_narrow_large (RDW multisegment, the C4 batch).
Predicates per workload: one numeric term, one string term, one three-term conjunction, each at about
1 %, 10 %, 50 % and 100 % selectivity (set by the literal; the measured selectivity is reported).
rdw_narrow has no COMP-3 field and its binary TAXPAYER-NUM is null in the synthetic data, so its
"numeric" row is a second string term (COMPANY-ID, ten digits).

Per case, in one process on one GPU:
  * test / scan / emit pass times of the filter stage (HIP events recorded by the library on the call's
    stream, cbx_filter_pass_times) and the whole call (events around it, the host wait for the count included);
  * filter + cbx_decode_selected, events around both calls on the stream (the filter call returns the
    surviving count to the host in between: that wait is part of the figure);
  * the unfiltered cbx_decode_fixed / cbx_decode_var step into preallocated columns, the same way.
Every figure is the median of --steps repetitions after --warmup.  One JSON line per case on stdout
(and appended to --out); the last line is the summary with the two expectations checked:
  (1) the filter stage alone takes no longer than the unfiltered decode of the batch,
  (2) filter + selected decode beats the unfiltered decode at 1 % selectivity,
and the crossover selectivity above which filtering first is slower (linear interpolation between the
measured selectivities).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
from decimal import Decimal

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd import synth  # noqa: E402
from cobrix_amd.reader import (FixedLenNestedReader, ReaderParameters, VarLenNestedReader, _alloc_columns,  # noqa: E402
                               string_capacity)

SELECTIVITIES = (0.01, 0.10, 0.50, 1.00)


def syn200_cases():
    """SYN200: AMT-01 uniform in (-1e13, 1e13), ZD-01 in (-1e7, 1e7), BR-ID in [-9999, 9999]; NAME is 0..18
    cp037 letters / digits (first character uniform over 62, 1 / 19 empty)."""
    def amt(f):
        return Decimal(min(int(-10 ** 15 + 2 * 10 ** 15 * f), 10 ** 15 - 1)).scaleb(-2)

    def zd(f):
        return Decimal(min(int(-10 ** 9 + 2 * 10 ** 9 * f), 10 ** 9 - 1)).scaleb(-2)

    name = {0.01: F.StringStartsWith("NAME", "A"), 0.10: F.LessThan("NAME", "4"), 0.50: F.LessThan("NAME", "T"),
            1.00: F.GreaterThanOrEqual("NAME", "")}
    out = []
    for s in SELECTIVITIES:
        f3 = s ** (1.0 / 3.0)
        out.append(("comp3", s, [F.LessThan("AMT-01", amt(s))]))
        out.append(("string", s, [name[s]]))
        out.append(("conj3", s, [F.LessThan("AMT-01", amt(f3)), F.LessThan("ZD-01", zd(f3)),
                                 F.LessThan("BR-ID", int(-9999 + 19999 * f3) + 1)]))
    return out


def rdw_cases():
    """rdw_narrow: COMPANY-ID is ten uniform digits; 35 % of the records are segment C (COMPANY-NAME: letters / digits)."""
    cid = {0.01: "01", 0.10: "1", 0.50: "5", 1.00: ":"}
    nm = {0.01: F.StringStartsWith("COMPANY-ID", "37"), 0.10: F.StringStartsWith("COMPANY-ID", "4"),
          0.50: F.GreaterThanOrEqual("COMPANY-ID", "5"), 1.00: F.IsNotNull("COMPANY-ID")}
    conj = {0.01: ("03", "0"), 0.10: ("3", "0"), 0.50: (":", "0"), 1.00: (":", "")}
    out = []
    for s in SELECTIVITIES:
        out.append(("string_a", s, [F.LessThan("COMPANY-ID", cid[s])]))
        out.append(("string_b", s, [nm[s]]))
        a, b = conj[s]
        third = F.IsNotNull("SEGMENT-ID") if s == 1.00 else F.EqualTo("SEGMENT-ID", "C")
        out.append(("conj3", s, [third, F.LessThan("COMPANY-ID", a), F.Or(F.GreaterThanOrEqual("COMPANY-NAME", b), F.IsNull("COMPANY-NAME"))
                                 if s == 1.00 else F.GreaterThanOrEqual("COMPANY-NAME", b)]))
    return out


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
    """One batch resident in HBM with its reader; unfiltered decode columns allocated once."""

    def __init__(self, name, n_rec, dev):
        self.name = name
        L = self.L = N.load()
        if name == "syn200":
            self.rd = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters(string_views=True))
            self.data = synth.syn200(n_rec, seed=20261015, device=dev).view(-1)
            self.n_bytes, self.n_rec, self.stride = int(self.data.numel()), n_rec, synth.SYN200_RECORD_SIZE
            self.off = self.ln = None
            self.cases = syn200_cases()
        else:
            p = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID", generate_record_id=True, string_views=True,
                                 segment_id_redefine_map={k: v for k, v in synth.RDW_NARROW_SEGMENTS.items()})
            self.rd = VarLenNestedReader(synth.RDW_NARROW_COPYBOOK, p)
            size = synth.rdw_narrow_large_size(n_rec, device=dev)
            buf = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
            self.data, _ = synth.rdw_narrow_large(n_rec, device=dev, out=buf)
            self.n_bytes, self.stride = size, 0
            self.off, self.ln = self.rd.frame(self.data, size)
            self.n_rec = int(self.off.numel())
            self.cases = rdw_cases()
        self.h = self.rd.native.handle
        self.st = torch.cuda.current_stream()
        self.cols, self.cs = _alloc_columns(self.rd.plan, self.n_rec, string_capacity(self.rd.native, self.n_rec), dev)
        N.check(L.cbx_plan_set_profiling(self.h, 1))

    def unfiltered(self):
        L, sp = self.L, ctypes.c_void_p(self.st.cuda_stream)
        if self.stride:
            N.check(L.cbx_decode_fixed(self.h, self.data.data_ptr(), self.n_rec, self.stride, 0, 0, self.cs, sp))
        else:
            N.check(L.cbx_decode_var(self.h, self.data.data_ptr(), self.n_bytes, self.off.data_ptr(), self.ln.data_ptr(),
                                     self.n_rec, 0, 0, self.cs, sp))

    def filter(self, table):
        return self.rd._filter_records(table, self.data, self.n_bytes, self.n_rec, self.st, rec_off=self.off,
                                       rec_len=self.ln, stride=self.stride)

    def pass_times(self):
        t = [ctypes.c_float(0) for _ in range(3)]
        N.check(self.L.cbx_filter_pass_times(self.h, *[ctypes.byref(x) for x in t]))
        return [x.value for x in t]

    def drain_kernel_times(self):
        n = ctypes.c_int32(0)
        N.check(self.L.cbx_plan_kernel_times(self.h, None, None, 0, ctypes.byref(n)))


def run(work: Work, steps: int, warmup: int, emit):
    dev = work.data.device
    un_ms = median_ms(work.unfiltered, steps, warmup)
    work.drain_kernel_times()
    emit({"workload": work.name, "case": "unfiltered_decode", "records": work.n_rec, "input_bytes": work.n_bytes,
          "decode_ms": round(un_ms, 4)})
    results = []
    for kind, target, filters in work.cases:
        table, unhandled = F.compile_filters(work.rd.plan, filters)
        assert table is not None and not unhandled, unhandled.reasons
        row = {"workload": work.name, "case": kind, "target_selectivity": target, "terms": table.n_terms}
        sel = work.filter(table)
        row["selectivity"] = round(sel["n"] / work.n_rec, 5)
        passes = []

        def only_filter():
            work.filter(table)
            passes.append(work.pass_times())

        flt_ms = median_ms(only_filter, steps, warmup)
        test, scan, em = (statistics.median(p[k] for p in passes[-steps:]) for k in range(3))
        row["filter"] = {"filter_call_ms": round(flt_ms, 4), "test_ms": round(test, 4), "scan_ms": round(scan, 4),
                         "emit_ms": round(em, 4), "stage_ms": round(test + scan + em, 4)}
        # filter + selected decode into columns sized by the survivors
        n_sel = sel["n"]
        cols, cs = _alloc_columns(work.rd.plan, n_sel, string_capacity(work.rd.native, n_sel), dev)

        def filter_and_decode():
            s = work.filter(table)
            N.check(work.L.cbx_decode_selected(work.h, work.data.data_ptr(), work.n_bytes, ctypes.byref(s["struct"]), s["n"], 0,
                                               cs, ctypes.c_void_p(work.st.cuda_stream)))

        row["filter_plus_selected_decode_ms"] = round(median_ms(filter_and_decode, steps, warmup), 4)
        N.check(work.L.cbx_plan_check(work.h, ctypes.c_void_p(work.st.cuda_stream)))
        work.drain_kernel_times()
        row["unfiltered_decode_ms"] = round(un_ms, 4)
        del cols, cs, sel
        emit(row)
        results.append(row)
    return un_ms, results


def crossover(un_ms, rows):
    """Selectivity at which filter + selected decode equals the unfiltered decode, per predicate kind."""
    out = {}
    for kind in sorted({r["case"] for r in rows}):
        pts = sorted((r["selectivity"], r["filter_plus_selected_decode_ms"]) for r in rows if r["case"] == kind)
        x = None
        if pts[0][1] >= un_ms:
            x = 0.0
        for (s0, t0), (s1, t1) in zip(pts, pts[1:]):
            if t0 < un_ms <= t1:
                x = s0 + (s1 - s0) * (un_ms - t0) / (t1 - t0)
        out[kind] = round(x, 4) if x is not None else None   # None: filtering first is faster at every measured selectivity
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="syn200,rdw_narrow_large")
    ap.add_argument("--records", type=int, default=0, help="records per batch (default: 50M SYN200 = the C2 batch, 37.5M RDW = the C4 batch)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    emit({"tool": "bench_filter", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup})
    summary = {"case": "summary"}
    for name in args.workloads.split(","):
        n = args.records or {"syn200": 50_000_000, "rdw_narrow_large": 37_500_000}[name]
        work = Work(name, n, dev)
        un_ms, rows = run(work, args.steps, args.warmup, emit)
        path = lambda r: r["filter"]   # noqa: E731
        summary[name] = {
            "unfiltered_decode_ms": round(un_ms, 4),
            "filter_stage_ms_max": max(path(r)["stage_ms"] for r in rows),
            "filter_stage_no_longer_than_decode": all(path(r)["stage_ms"] <= un_ms for r in rows),
            "filter_first_wins_at_1pct": all(r["filter_plus_selected_decode_ms"] < un_ms for r in rows if r["target_selectivity"] == 0.01),
            "crossover_selectivity": crossover(un_ms, rows)}
        work.rd.close()
        del work
        torch.cuda.empty_cache()
    emit(summary)


if __name__ == "__main__":
    main()
