"""Measure Top-N pushdown (cbx_top_n_records) against what a caller does without it.

Workloads: SYN200 (fixed-length, 50 M records: the C2 batch) and rdw_narrow_large (RDW multisegment, the C4
batch, framed once outside the timed region).  Cases:
  syn200 / amt_desc_100, amt_desc_10000   ORDER BY AMT-01 DESC LIMIT 100 / 10,000, each without a filter and
                                          with AMT-02 < 0 (about half the rows);
  syn200 / br_id_100                      ORDER BY BR-ID LIMIT 100 (20 k values: a large tie class);
  syn200 / name_100                       ORDER BY NAME LIMIT 100 (an 18-byte string key);
  rdw_narrow_large / company_id_100       ORDER BY COMPANY-ID LIMIT 100 (a 10-byte string key of framed records).

Per case, in one process on one GPU, medians of --steps repetitions after --warmup:
  * top_n:       the key / select / emit pass times (HIP events recorded by the library on the call's stream,
                 cbx_top_n_pass_times), the selection call (events around it, its host waits included), the
                 call plus the decode of the winners, and cbx_top_n_info of the last call;
  * filter_test: the test pass of the row-filter stage over an IS NOT NULL term on the first key (plus the row
                 filter): it decodes the same field from the same cache lines as the key pass;
  * baseline:    numeric keys only -- the `columns=`-projected (and filtered) decode of the key column,
                 torch.topk over it (nulls masked to the far end), the winners turned back into a selection
                 and decoded with the full plan.  torch has no string sort: a string key has no baseline here.
--baseline-only runs the baseline alone and touches nothing of the Top-N stage, so the same file measures the
baseline on a revision (or a library variant, CBX_LIB_VARIANT) that lacks it.  One JSON line per case on stdout
(and appended to --out).
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

# (case, [(column, descending)], limit, filtered, numeric first key)
CASES = {
    "syn200": [("amt_desc_100", [("AMT-01", True)], 100, False, True), ("amt_desc_100", [("AMT-01", True)], 100, True, True),
               ("amt_desc_10000", [("AMT-01", True)], 10000, False, True), ("amt_desc_10000", [("AMT-01", True)], 10000, True, True),
               ("br_id_100", [("BR-ID", False)], 100, False, True), ("name_100", [("NAME", False)], 100, False, False)],
    "rdw_narrow_large": [("company_id_100", [("COMPANY-ID", False)], 100, False, False)],
}
FILTERS = {"syn200": lambda: [F.LessThan("AMT-02", 0)], "rdw_narrow_large": lambda: [F.EqualTo("SEGMENT-ID", "C")]}


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


def baseline(work: Work, keys, limit, filters, steps, warmup):
    """Projected (and filtered) decode of the first key column, torch.topk, the winners as a selection, the full
    decode of that selection (fixed-length source, one numeric key)."""
    assert not work.var
    (name, desc), = keys
    rd_key = work.reader(columns=[name])
    rd_full = work.reader()
    stride = rd_full.get_record_size()
    st = torch.cuda.current_stream()
    shifts = torch.arange(64, device=work.dev, dtype=torch.int64)
    plan = rd_key.out_plan
    ci = plan.fields[plan.field_of_node[id(rd_key.copybook.get_field_by_name(name))]].column
    table = F.compile_filters(rd_key.plan, filters)[0] if filters else None

    def run():
        if table is not None:
            src = rd_key._filter_records(table, work.data, work.n_bytes, work.n_rec, st, stride=stride)
            b = rd_key._decode_selection(work.data, work.n_bytes, src, False, st)
        else:
            src = None
            b = rd_key.decode_device(work.data, work.n_bytes)
        n = b.n_rec
        c = b.cols[ci]
        valid = ((c["validity"].unsqueeze(1) >> shifts) & 1).bool().view(-1)[:n]
        v = c["values"][:n].to(torch.int64)
        big = torch.iinfo(torch.int64)
        # DESC NULLS LAST / ASC NULLS FIRST (Spark's defaults): nulls at the small end
        v = torch.where(valid, v, big.min)
        win = torch.sort(torch.topk(v, min(limit, n), largest=desc).indices).values
        sel, cs = rd_full._empty_selection(int(win.numel()), work.dev)
        k = int(win.numel())
        if src is not None:
            sel["rec_off"][:k] = src["rec_off"][win]
            sel["record_id"][:k] = src["record_id"][win]
        else:
            sel["rec_off"][:k] = win * stride
            sel["record_id"][:k] = win
        sel["rec_len"][:k] = stride
        sel["segment"][:k] = -1
        sel["n"], sel["struct"] = k, cs
        return rd_full._decode_selection(work.data, work.n_bytes, sel, False, st)

    ms = median_ms(run, steps, warmup)
    rd_key.close()
    rd_full.close()
    return ms


def top_n_times(work: Work, keys, limit, filters, steps, warmup):
    from cobrix_amd.topn import SortOrder
    rd = work.reader()
    N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 1))
    orders = [SortOrder(c, d) for c, d in keys]
    st = torch.cuda.current_stream()
    src = dict(rec_off=work.off, rec_len=work.ln) if work.var else dict(stride=rd.get_record_size())
    passes = []

    def select():
        sel = rd._top_n_records(orders, limit, filters or None, work.data, work.n_bytes, work.n_rec, st, **src)
        passes.append(rd.topn_pass_times())
        return sel

    def whole():
        return rd._decode_selection(work.data, work.n_bytes, select(), False, st)

    select_ms = median_ms(select, steps, warmup)
    key, sel_ms, emit = (statistics.median(p[k] for p in passes[-steps:]) for k in range(3))
    whole_ms = median_ms(whole, steps, warmup)
    info = rd.topn_info()
    out = {"select_call_ms": round(select_ms, 4), "call_and_decode_ms": round(whole_ms, 4), "key_ms": round(key, 4),
           "select_ms": round(sel_ms, 4), "emit_ms": round(emit, 4), "n_live": info.n_live, "levels_run": info.levels_run,
           "levels_total": info.levels_total, "ties_after_level0": info.ties_after_level0, "ties_max": info.ties_max,
           "grid": info.grid}
    # the filter stage's test pass over the first key (IS NOT NULL), with the same row filter
    table, un = F.compile_filters(rd.plan, [F.IsNotNull(keys[0][0])] + list(filters))
    assert not un, un.reasons
    tests = []

    def flt():
        rd._filter_records(table, work.data, work.n_bytes, work.n_rec, st, **src)
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
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topn.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    emit({"tool": "bench_topn", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
          "abi": N.ABI_VERSION, "baseline_only": args.baseline_only, "lib_variant": os.environ.get("CBX_LIB_VARIANT", "")})
    for name in args.workloads.split(","):
        n = args.records or {"syn200": 50_000_000, "rdw_narrow_large": 37_500_000}[name]
        work = Work(name, n, dev)
        for case, keys, limit, filtered, numeric in CASES[name]:
            if args.cases and case not in args.cases.split(","):
                continue
            filters = FILTERS[name]() if filtered else []
            row = {"workload": name, "case": case, "filtered": filtered, "limit": limit, "records": work.n_rec,
                   "input_bytes": work.n_bytes}
            row["baseline_ms"] = round(baseline(work, keys, limit, filters, args.steps, args.warmup), 4) \
                if numeric and not work.var else None
            if not args.baseline_only:
                row["top_n"] = top_n_times(work, keys, limit, filters, args.steps, args.warmup)
                if row["baseline_ms"]:
                    row["baseline_over_call_and_decode"] = round(row["baseline_ms"] / row["top_n"]["call_and_decode_ms"], 2)
            elif row["baseline_ms"] is None:
                continue
            emit(row)
            torch.cuda.empty_cache()
        del work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
