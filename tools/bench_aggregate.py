"""Measure aggregate pushdown (cbx_aggregate_records) against what a caller does without it.

Workloads: SYN200 (fixed-length, 50 M records: the C2 batch) and rdw_narrow_large (RDW multisegment, the C4
batch, framed once outside the timed region).  Requests per workload:
  count_star      COUNT(*) alone;
  one_field       COUNT, MIN, MAX and SUM of one field (SYN200: AMT-01, COMP-3; rdw_narrow has no COMP-3
                  field: TAXPAYER-NUM, binary);
  three_fields    the four functions of three numeric fields (SYN200: AMT-01 COMP-3, ZD-01 zoned, BR-ID
                  binary; rdw_narrow has one numeric field: TAXPAYER-NUM plus COUNT of COMPANY-NAME and
                  PHONE-NUMBER),
each without a filter and with a one-term filter (SYN200: AMT-02 < 0, about half the rows; rdw_narrow:
SEGMENT-ID = 'C').

Per case, in one process on one GPU, medians of --steps repetitions after --warmup:
  * aggregate:   the accumulate and combine pass times (HIP events recorded by the library on the call's
                 stream, cbx_aggregate_pass_times) and the whole call (events around it, the host wait for
                 the result included);
  * filter_test: the test pass of the row-filter stage over IS NOT NULL terms on the same fields
                 (cbx_filter_pass_times) -- it decodes the same fields from the same cache lines;
  * baseline:    the `columns=`-projected (and filtered) decode of the same fields followed by torch
                 reductions of the columns (validity unpacked, masked min / max / sum in int64 -- not exact
                 beyond 64 bits), the host wait for the values included.
--baseline-only runs the baseline alone and imports nothing of the aggregate stage, so the same file measures
the baseline on a revision that lacks it.  One JSON line per case on stdout (and appended to --out).
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
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader  # noqa: E402

REQUESTS = {
    "syn200": {"count_star": [], "one_field": [("AMT-01", True)],
               "three_fields": [("AMT-01", True), ("ZD-01", True), ("BR-ID", True)],
               "filter": lambda: [F.LessThan("AMT-02", 0)]},
    "rdw_narrow_large": {"count_star": [], "one_field": [("TAXPAYER-NUM", True)],
                         "three_fields": [("TAXPAYER-NUM", True), ("COMPANY-NAME", False), ("PHONE-NUMBER", False)],
                         "filter": lambda: [F.EqualTo("SEGMENT-ID", "C")]},
}


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
    """One batch resident in HBM, framed once."""

    def __init__(self, name, n_rec, dev):
        self.name, self.dev = name, dev
        if name == "syn200":
            self.text, self.params, self.var = synth.SYN200_COPYBOOK, ReaderParameters(string_views=True), False
            self.data = synth.syn200(n_rec, seed=20261015, device=dev).view(-1)
            self.n_bytes, self.n_rec = int(self.data.numel()), n_rec
            self.off = self.ln = None
        else:
            self.text, self.var = synth.RDW_NARROW_COPYBOOK, True
            self.params = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID", string_views=True,
                                           segment_id_redefine_map={k: v for k, v in synth.RDW_NARROW_SEGMENTS.items()})
            size = synth.rdw_narrow_large_size(n_rec, device=dev)
            buf = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
            self.data, _ = synth.rdw_narrow_large(n_rec, device=dev, out=buf)
            self.n_bytes = size
            rd = self.reader()
            self.off, self.ln = rd.frame(self.data, size)
            self.n_rec = int(self.off.numel())
            rd.close()

    def reader(self, columns=None):
        cls = VarLenNestedReader if self.var else FixedLenNestedReader
        return cls(self.text, self.params, columns=columns)


def baseline(work: Work, fields, filters, steps, warmup):
    """Projected (and filtered) decode of the fields, then torch reductions of the columns."""
    rd = work.reader(columns=[name for name, _ in fields])
    shifts = torch.arange(64, device=work.dev, dtype=torch.int64)
    plan = rd.out_plan
    cols = [(plan.fields[plan.field_of_node[id(rd.copybook.get_field_by_name(name))]].column, numeric) for name, numeric in fields]

    def run():
        if work.var:
            if filters:
                b = rd.decode_selected(work.data, work.n_bytes, rd.filter(work.data, work.n_bytes, (work.off, work.ln), filters))
            else:
                b = rd.decode_device(work.data, work.n_bytes, work.off, work.ln)
        else:
            b = rd.decode_device(work.data, work.n_bytes, filters=filters or None)
        n = b.n_rec
        out = [torch.tensor(n, device=work.dev)]
        for ci, numeric in cols:
            c = b.cols[ci]
            valid = ((c["validity"].unsqueeze(1) >> shifts) & 1).bool().view(-1)[:n]
            out.append(valid.sum())
            if numeric and n:
                v = c["values"][:n].to(torch.int64)
                big = torch.iinfo(torch.int64)
                out += [torch.where(valid, v, big.max).min(), torch.where(valid, v, big.min).max(), torch.where(valid, v, 0).sum()]
        return torch.stack(out).cpu()

    ms = median_ms(run, steps, warmup)
    rd.close()
    return ms


def aggregate_times(work: Work, fields, filters, steps, warmup):
    from cobrix_amd import aggregate as A
    rd = work.reader()
    N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 1))
    aggs = [A.CountStar()]
    for name, numeric in fields:
        aggs += [A.Count(name)] + ([A.Min(name), A.Max(name), A.Sum(name)] if numeric else [])
    passes = []

    def run():
        if work.var:
            r = rd.aggregate_device(work.data, work.n_bytes, (work.off, work.ln), aggs, filters or None)
        else:
            r = rd.aggregate_device(work.data, work.n_bytes, aggs, filters or None)
        passes.append(rd.aggregate_pass_times())
        return r

    call_ms = median_ms(run, steps, warmup)
    acc, comb = (statistics.median(p[k] for p in passes[-steps:]) for k in range(2))
    res = run()
    out = {"call_ms": round(call_ms, 4), "accumulate_ms": round(acc, 4), "combine_ms": round(comb, 4),
           "n_rows": res.n_rows, "selectivity": round(res.n_rows / max(1, work.n_rec), 5)}
    # the filter stage's test pass over the same fields (IS NOT NULL terms), with the same row filter
    if fields:
        table, un = F.compile_filters(rd.plan, [F.IsNotNull(name) for name, _ in fields] + list(filters))
        assert not un, un.reasons
        tests = []

        def flt():
            rd._filter_records(table, work.data, work.n_bytes, work.n_rec, torch.cuda.current_stream(), rec_off=work.off,
                               rec_len=work.ln, stride=0 if work.var else rd.get_record_size())
            t = [ctypes.c_float(0) for _ in range(3)]
            N.check(N.load().cbx_filter_pass_times(rd.native.handle, *[ctypes.byref(x) for x in t]))
            tests.append(t[0].value)

        median_ms(flt, steps, warmup)
        out["filter_test_pass_ms"] = round(statistics.median(tests[-steps:]), 4)
    rd.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="syn200,rdw_narrow_large")
    ap.add_argument("--records", type=int, default=0, help="records per batch (default: 50M SYN200, 37.5M RDW)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_aggregate.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    emit({"tool": "bench_aggregate", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
          "abi": N.ABI_VERSION, "baseline_only": args.baseline_only})
    for name in args.workloads.split(","):
        n = args.records or {"syn200": 50_000_000, "rdw_narrow_large": 37_500_000}[name]
        work = Work(name, n, dev)
        req = REQUESTS[name]
        for case in ("count_star", "one_field", "three_fields"):
            for filtered in (False, True):
                filters = req["filter"]() if filtered else []
                row = {"workload": name, "case": case, "filtered": filtered, "records": work.n_rec, "input_bytes": work.n_bytes}
                if case == "count_star" and not filtered:
                    row["baseline_ms"] = None      # the record count of an unfiltered batch needs no GPU work
                else:
                    row["baseline_ms"] = round(baseline(work, req[case], filters, args.steps, args.warmup), 4)
                if not args.baseline_only:
                    row["aggregate"] = aggregate_times(work, req[case], filters, args.steps, args.warmup)
                    if row["baseline_ms"]:
                        row["baseline_over_aggregate_call"] = round(row["baseline_ms"] / row["aggregate"]["call_ms"], 2)
                emit(row)
                torch.cuda.empty_cache()
        del work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
