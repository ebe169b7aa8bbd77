"""Measure fan-out joins (cbx_key_map_index_rows, cbx_join_records_expand) against their floor -- the lookup join of
the same input -- and against the torch path they replace.

Workloads, in one process on one GPU, all SYN200 fact records (default 10 M) joined by BR-ID (about 20 k values):
  unique:     (a) a dimension with unique keys (the first record of every BR-ID among 200 k SYN200 records of another
              seed): the expand call against cbx_join_records on the same input, per pass and per call.
  moderate:   (b) 60 k SYN200 records of another seed as they are: about three rows per key.
  hot:        (c) the same with a third of the dimension's rows moved onto the fact file's first BR-ID: one hot key
              carries a large share of the matches.
  selective:  (d) the moderate dimension under a selective fact filter (REC-ID < 50,000,000: about 5 % of the rows).
Per case:
  index:    `KeyMap.index_rows` from the library's HIP events (profiling on) beside the fill pass of the same map, the
            members each sort path took.
  expand:   the test / scan / emit passes of cbx_join_records_expand from HIP events, the call without the decode as
            wall time (capacity known: one attempt), emit ms per output row beside the bytes the emit must write per
            row (28 of selection + 8 of match + 8 of fact row).
  floor:    cbx_join_records (duplicates="first") on the same input: its passes and the call.
  replaced: the path the join replaces, in the same process: projected decode of both key columns, a torch join (sort,
            searchsorted on both sides, repeat_interleave), two selections built with torch, both decodes -- wall time,
            beside the new path end to end (join + decode, dimension()).
Every figure is the median of --steps repetitions after --warmup.  One JSON line per case on stdout (and appended to
--out).  --resource-usage FILE writes the compiler's resource-usage remarks of the new kernels there (no GPU needed).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("scan64_reduce_kernel", "scan64_apply_kernel", "keymap_rows_scatter_kernel", "keymap_rows_classify_kernel",
           "keymap_rows_sort_lds_kernel", "keymap_rows_sort_global_kernel", "keymap_rows_check_kernel", "fanout_compact_kernel",
           "fanout_emit_kernel", "keymap_test_kernel", "keymap_fill_kernel", "keymap_emit_kernel")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="unique,moderate,hot,selective")
    ap.add_argument("--records", type=int, default=10_000_000, help="fact records")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--resource-usage", default="", help="write the new kernels' resource-usage remarks here and exit")
    ap.add_argument("--remarks-from", default="", help="with --resource-usage: a saved compiler log to take them from")
    args = ap.parse_args()
    if args.resource_usage:
        import bench_keymap
        bench_keymap.KERNELS = KERNELS
        if args.remarks_from:
            bench_keymap.write_resource_usage(open(args.remarks_from).read(), args.resource_usage)
        else:
            bench_keymap.resource_usage(args.resource_usage)
        return
    import torch

    from cobrix_amd import filter as F
    from cobrix_amd import native as N
    from cobrix_amd import synth
    from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters

    if not torch.cuda.is_available():
        raise SystemExit("bench_fanout.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    L = N.load()
    steps, warmup = args.steps, args.warmup

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    def wall_ms(fn):
        ms, last = [], None
        for k in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), last

    def med(xs):
        return round(statistics.median(xs[warmup:]), 4)

    def key_column(rd, batch, name):
        plan = rd.out_plan
        fi = plan.field_of_node[id(rd.copybook.get_field_by_name(name))]
        return batch.cols[plan.fields[fi].column]["values"][:batch.n_rec]

    def fixed_selection(rd, idx, stride, device):
        n = int(idx.numel())
        sel, cs = rd._empty_selection(n, device)
        sel["rec_off"][:n] = idx * stride
        sel["rec_len"][:n] = stride
        sel["record_id"][:n] = idx
        sel["segment"][:n] = -1
        sel["n"], sel["struct"] = n, cs
        return sel

    emit({"tool": "bench_fanout", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup})
    n_fact = args.records
    fact = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters())
    dim = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters())
    fkey = {k: FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters(), columns=[k]) for k in ("BR-ID", "REC-ID")}
    for rd in (fact, dim):
        N.check(L.cbx_plan_set_profiling(rd.native.handle, 1))
    fdata = synth.syn200(n_fact, seed=20261015, device=dev).view(-1)
    f_bytes = int(fdata.numel())
    st = torch.cuda.current_stream()
    for name in args.workloads.split(","):
        ffilters = [F.LessThan("REC-ID", 50_000_000)] if name == "selective" else None
        if name == "unique":
            raw = synth.syn200(200_000, seed=7, device=dev)
            br = (raw[:, 4].to(torch.int64) << 8) | raw[:, 5].to(torch.int64)
            order = torch.argsort(br, stable=True)
            first = torch.ones_like(order, dtype=torch.bool)
            first[1:] = br[order][1:] != br[order][:-1]
            ddata = raw[torch.sort(order[first]).values].contiguous().view(-1)
        else:
            raw = synth.syn200(60_000, seed=7, device=dev).clone()
            if name == "hot":
                raw[::3, 4:6] = fdata[4:6]   # every third dimension row takes the first fact row's BR-ID bytes
            ddata = raw.contiguous().view(-1)
        d_bytes = int(ddata.numel())
        row = {"workload": name, "key": "BR-ID", "fact_records": n_fact, "dimension_records": d_bytes // 200,
               "fact_filter": repr(ffilters) if ffilters else None}
        infos, rinfos = [], []

        def build():
            with dim.key_map_of_device(ddata, d_bytes, ["BR-ID"], fact, ["BR-ID"]) as km:
                rinfos.append(km.index_rows())
                infos.append(km.source_info)

        ms, _ = wall_ms(build)
        ri = rinfos[-1]
        row.update(n_values=infos[-1].n_source_keys - infos[-1].n_dropped, n_duplicate_keys=infos[-1].n_duplicate_keys,
                   max_rows_per_key=infos[-1].max_rows_per_key)
        row["index"] = {"index_ms": med([r.index_ms for r in rinfos]), "fill_ms": med([s.fill_ms for s in infos]),
                        "distinct_ms": med([s.distinct_ms for s in infos]), "map_and_index_wall_ms": round(ms, 4),
                        "n_indexed_rows": ri.n_indexed_rows, "n_short": ri.n_short, "n_lds": ri.n_lds, "n_global": ri.n_global,
                        "short_max": ri.short_max, "lds_max": ri.lds_max}
        row["index"]["index_over_fill"] = round(row["index"]["index_ms"] / max(row["index"]["fill_ms"], 1e-9), 3)
        km = dim.key_map_of_device(ddata, d_bytes, ["BR-ID"], fact, ["BR-ID"])
        km.index_rows()
        T, kept = fact._join_records(km, "inner", ffilters, "all", fdata, f_bytes, n_fact, st, stride=200, count_only=True)
        row.update(n_out=T, n_kept=kept)
        passes = []

        def expand():
            res = fact._join_records(km, "inner", ffilters, "all", fdata, f_bytes, n_fact, st, stride=200, decode=False,
                                     max_rows=max(T, 1))
            passes.append(fact.join_expand_pass_times())
            return res.selection["n"]

        ms, n = wall_ms(expand)
        assert n == T
        info = fact.join_expand_info()
        row["expand"] = {"test_ms": med([p[0] for p in passes]), "scan_ms": med([p[1] for p in passes]),
                         "emit_ms": med([p[2] for p in passes]), "call_wall_ms": round(ms, 4), "max_fanout": info.max_fanout,
                         "emit_grid": info.emit_grid, "attempts": 1 if T <= n_fact else 2}
        row["expand"]["emit_ns_per_output_row"] = round(row["expand"]["emit_ms"] * 1e6 / max(T, 1), 4)
        row["expand"]["emit_bytes_written_per_row"] = 28 + 8 + 8
        lp = []

        def lookup():
            res = fact._join_records(km, "inner", ffilters, "first", fdata, f_bytes, n_fact, st, stride=200, decode=False)
            lp.append(fact.join_pass_times())
            return res.selection["n"]

        ms, n = wall_ms(lookup)
        assert n == kept
        row["floor"] = {"test_ms": med([p[0] for p in lp]), "scan_ms": med([p[1] for p in lp]), "emit_ms": med([p[2] for p in lp]),
                        "call_wall_ms": round(ms, 4)}
        for k in ("test_ms", "scan_ms", "emit_ms", "call_wall_ms"):
            row["expand_over_floor_" + k] = round(row["expand"][k] / max(row["floor"][k], 1e-9), 3)

        def new_path():
            res = fact._join_records(km, "inner", ffilters, "all", fdata, f_bytes, n_fact, st, stride=200)
            return res.batch.n_rec + res.dimension().n_rec

        def replaced():
            fb = fkey["BR-ID"].decode_device(fdata, f_bytes)
            fk = key_column(fkey["BR-ID"], fb, "BR-ID").to(torch.int64)
            keep = torch.ones_like(fk, dtype=torch.bool)
            if ffilters:
                rb = fkey["REC-ID"].decode_device(fdata, f_bytes)
                keep &= key_column(fkey["REC-ID"], rb, "REC-ID").to(torch.int64) < 50_000_000
            db = fkey["BR-ID"].decode_device(ddata, d_bytes)
            dk = key_column(fkey["BR-ID"], db, "BR-ID").to(torch.int64)
            sk, order = torch.sort(dk, stable=True)
            lo, hi = torch.searchsorted(sk, fk), torch.searchsorted(sk, fk, right=True)
            cnt = torch.where(keep, hi - lo, torch.zeros_like(lo))
            f_idx = torch.repeat_interleave(torch.arange(fk.numel(), device=dev), cnt)
            start = torch.cumsum(cnt, 0) - cnt
            q = torch.arange(f_idx.numel(), device=dev) - start[f_idx]
            m_idx = order[lo[f_idx] + q]
            a = fact._decode_selection(fdata, f_bytes, fixed_selection(fact, f_idx, 200, dev), False, st)
            b = dim._decode_selection(ddata, d_bytes, fixed_selection(dim, m_idx, 200, dev), False, st)
            return a.n_rec + b.n_rec

        ms_new, n_new = wall_ms(new_path)
        row["end_to_end"] = {"join_ms": round(ms_new, 4)}
        emit(dict(row, partial=True))   # (the replaced path allocates the most: keep what is measured so far)
        ms_old, n_old = wall_ms(replaced)
        row["end_to_end"].update(replaced_ms=round(ms_old, 4), join_over_replaced=round(ms_new / ms_old, 4),
                                 rows_new=n_new, rows_replaced=n_old, rows_agree=n_new == n_old == 2 * T)
        km.close()
        emit(row)
        del ddata
    for rd in [fact, dim] + list(fkey.values()):
        rd.close()


if __name__ == "__main__":
    main()
