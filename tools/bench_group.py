"""Measure grouped aggregate pushdown (cbx_aggregate_grouped) against its two baselines.

Configurations (each without a filter and with a one-term filter: SYN200 AMT-02 < 0, rdw_narrow SEGMENT-ID = 'C'):
  syn200_br         50 M SYN200 records grouped by BR-ID (about 20 k groups), COUNT and SUM of AMT-01;
  narrow_segment    rdw_narrow_large grouped by SEGMENT-ID (a handful of groups), COUNT and SUM of TAXPAYER-NUM;
  narrow_taxpayer   the same grouped by TAXPAYER-TYPE;
  syn200_cust       a 1 M-record SYN200 slice grouped by CUST-KEY (nearly all distinct), COUNT and SUM of AMT-01.

Per configuration, in one process on one GPU, medians of --steps repetitions after --warmup:
  * grouped:   the init, accumulate and emit pass times (HIP events recorded by the library on the call's stream,
               cbx_group_pass_times) and the whole call (events around it: table compilation, the output arrays'
               allocation and both host waits included; the mapping of the arrays to Python values is not);
  * baseline (a), what a caller does without it: the `columns=`-projected (and filtered) decode of the key and value
               columns, then torch.unique(return_inverse=True) over the key column and scatter reductions
               (index_add_ of the valid flags and of the int64 values -- not exact beyond 64 bits), the host wait for
               the per-group values included;
  * baseline (b), the floor: the ungrouped cbx_aggregate_records over the same fields (key and value) and filter.
Ratios above 1 mean the grouped call is slower than that baseline.  One JSON line per configuration on stdout (and
appended to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_aggregate import Work, median_ms  # noqa: E402
from cobrix_amd import aggregate as A  # noqa: E402
from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402

CONFIGS = {
    "syn200_br": ("syn200", 50_000_000, "BR-ID", "AMT-01", 65536),
    "narrow_segment": ("rdw_narrow_large", 37_500_000, "SEGMENT-ID", "TAXPAYER-NUM", 1024),
    "narrow_taxpayer": ("rdw_narrow_large", 37_500_000, "TAXPAYER-TYPE", "TAXPAYER-NUM", 1024),
    "syn200_cust": ("syn200", 1_000_000, "CUST-KEY", "AMT-01", 1 << 20),
}
FILTERS = {"syn200": lambda: [F.LessThan("AMT-02", 0)], "rdw_narrow_large": lambda: [F.EqualTo("SEGMENT-ID", "C")]}


def grouped_times(work: Work, key, value, filters, max_groups, steps, warmup):
    rd = work.reader()
    N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 1))
    aggs = [A.CountStar(), A.Count(value), A.Sum(value)]
    passes = []

    def run():
        st = torch.cuda.current_stream()
        if work.var:
            r = rd._aggregate_grouped([key], aggs, filters or None, max_groups, work.data, work.n_bytes, work.n_rec, st,
                                      rec_off=work.off, rec_len=work.ln, header_only=True)
        else:
            r = rd._aggregate_grouped([key], aggs, filters or None, max_groups, work.data, work.n_bytes, work.n_rec, st,
                                      stride=rd.get_record_size(), header_only=True)
        passes.append(rd.group_pass_times())
        return r

    call_ms = median_ms(run, steps, warmup)
    init, acc, emit = (statistics.median(p[k] for p in passes[-steps:]) for k in range(3))
    res = run()
    rd.close()
    return {"call_ms": round(call_ms, 4), "init_ms": round(init, 4), "accumulate_ms": round(acc, 4), "emit_ms": round(emit, 4),
            "library_ms": round(init + acc + emit, 4), "n_groups": res[0], "n_rows": res[1]}


def ungrouped_ms(work: Work, key, value, filters, steps, warmup):
    rd = work.reader()
    aggs = [A.CountStar(), A.Count(key), A.Count(value), A.Sum(value)]

    def run():
        if work.var:
            return rd.aggregate_device(work.data, work.n_bytes, (work.off, work.ln), aggs, filters or None)
        return rd.aggregate_device(work.data, work.n_bytes, aggs, filters or None)

    ms = median_ms(run, steps, warmup)
    rd.close()
    return ms


def unique_scatter_ms(work: Work, key, value, filters, steps, warmup):
    """Projected (and filtered) decode of the two columns, torch.unique over the keys, scatter reductions."""
    rd = work.reader(columns=[key, value])
    plan = rd.out_plan
    kc, vc = (plan.fields[plan.field_of_node[id(rd.copybook.get_field_by_name(n))]].column for n in (key, value))
    shifts = torch.arange(64, device=work.dev, dtype=torch.int64)

    def run():
        if work.var:
            if filters:
                b = rd.decode_selected(work.data, work.n_bytes, rd.filter(work.data, work.n_bytes, (work.off, work.ln), filters))
            else:
                b = rd.decode_device(work.data, work.n_bytes, work.off, work.ln)
        else:
            b = rd.decode_device(work.data, work.n_bytes, filters=filters or None)
        n = b.n_rec
        k, v = b.cols[kc], b.cols[vc]
        valid = ((v["validity"].unsqueeze(1) >> shifts) & 1).view(-1)[:n]
        if "values" in k:
            keys = k["values"][:n].to(torch.int64)
            knull = ((k["validity"].unsqueeze(1) >> shifts) & 1).view(-1)[:n] == 0
            keys = torch.where(knull, torch.iinfo(torch.int64).min, keys)
        else:   # a short string key: the first 8 bytes of its 16-byte view (length, inline bytes) name the value
            keys = k["views"].view(-1, 16)[:n, :8].contiguous().view(torch.int64).view(-1)
            knull = ((k["validity"].unsqueeze(1) >> shifts) & 1).view(-1)[:n] == 0
            keys = torch.where(knull, torch.iinfo(torch.int64).min, keys)
        uniq, inv = torch.unique(keys, return_inverse=True)
        g = int(uniq.numel())
        rows = torch.zeros(g, dtype=torch.int64, device=work.dev).index_add_(0, inv, torch.ones_like(inv))
        cnt = torch.zeros(g, dtype=torch.int64, device=work.dev).index_add_(0, inv, valid)
        sm = torch.zeros(g, dtype=torch.int64, device=work.dev).index_add_(0, inv, torch.where(valid.bool(), v["values"][:n].to(torch.int64), 0))
        return torch.stack([uniq, rows, cnt, sm]).cpu()

    ms = median_ms(run, steps, warmup)
    rd.close()
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--scale", type=float, default=1.0, help="scale the record counts (a quick run)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-unique", action="store_true", help="leave baseline (a) out")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_group.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    emit({"tool": "bench_group", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
          "abi": N.ABI_VERSION})
    work = None
    for name in args.configs.split(","):
        wl, n, key, value, max_groups = CONFIGS[name]
        n = max(64, int(n * args.scale))
        if work is None or (work.name, work.requested) != (wl, n):
            work = None
            torch.cuda.empty_cache()
            work = Work(wl, n, dev)
            work.requested = n
        for filtered in (False, True):
            filters = FILTERS[wl]() if filtered else []
            row = {"config": name, "filtered": filtered, "records": work.n_rec, "input_bytes": work.n_bytes, "key": key, "value": value}
            row["grouped"] = grouped_times(work, key, value, filters, max_groups, args.steps, args.warmup)
            row["ungrouped_ms"] = round(ungrouped_ms(work, key, value, filters, args.steps, args.warmup), 4)
            row["grouped_over_ungrouped"] = round(row["grouped"]["call_ms"] / row["ungrouped_ms"], 2)
            if not args.skip_unique:
                try:
                    row["unique_scatter_ms"] = round(unique_scatter_ms(work, key, value, filters, args.steps, args.warmup), 4)
                    row["grouped_over_unique_scatter"] = round(row["grouped"]["call_ms"] / row["unique_scatter_ms"], 2)
                except Exception as e:   # noqa: BLE001 -- a baseline that cannot run is reported, the tool goes on
                    row["unique_scatter_error"] = f"{type(e).__name__}: {e}"[:200]
            emit(row)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
