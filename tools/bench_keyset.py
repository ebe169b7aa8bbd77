"""Measure key-set filters (cbx_key_set_create, cbx_filter_records_keyed) against what a caller does without them.

Workloads, in one process on one GPU:
  syn200_br:   SYN200 records (default 50 M) by BR-ID (uniform over the 19,999 values of [-9999, 9999]) with sets of 64,
               1,000 and 20,000 values aimed at 1 %, 10 % and 50 % surviving rows.  A set of k values of a uniform key
               keeps at most k / 19,999 of the rows, so the two small sets reach 0.3 % and 5 %: the values a target
               does not need are taken from outside the key's domain, and the measured selectivity is reported.
  syn200_cust: SYN200 records (default 1 M) by CUST-KEY with the 500,000 keys of the first half of the records.
  rdw_narrow:  rdw_narrow_large records (default 10 M) by the string key COMPANY-ID (ten digits) with the keys of the
               first 100,000 records.
Per case: the set's build (HIP events of the library, cbx_key_set_info), the test / scan / emit passes of the keyed
filter (cbx_filter_pass_times), and the keyed filter + decode of the survivors through a `columns=` reader, against
  (a) the caller's way on the parent: the `columns=`-projected decode of all rows, torch.isin on the key column,
      boolean indexing of every column (numeric keys only: torch.isin takes no strings);
  (b) the floor: cbx_filter_records with one OP_IN of 64 literals on the same field (its test pass).
Every figure is the median of --steps repetitions after --warmup, HIP events on the stream.  One JSON line per case on
stdout (and appended to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd import synth  # noqa: E402
from cobrix_amd.keyset import KeySet, compile_key_values  # noqa: E402
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader  # noqa: E402

SYN_COLUMNS = ["BR-ID", "CUST-KEY", "ACCT-NO", "AMT-01", "QTY-01"]
RDW_COLUMNS = ["SEGMENT-ID", "COMPANY-ID"]


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


def pass_times(rd):
    import ctypes
    t = [ctypes.c_float(0) for _ in range(3)]
    N.check(N.load().cbx_filter_pass_times(rd.native.handle, *[ctypes.byref(x) for x in t]))
    return [x.value for x in t]


def passes_median(call, rd, steps, warmup):
    """(whole call ms, [test, scan, emit] ms) of a filter call, medians."""
    seen = []

    def fn():
        call()
        seen.append(pass_times(rd))
    whole = median_ms(fn, steps, warmup)
    return whole, [statistics.median(p[k] for p in seen[-steps:]) for k in range(3)]


def column_of(rd, name):
    return next(c.index for c in rd.out_plan.columns
                if c.node is not None and c.node.name.upper().replace("_", "-") == name)


def be_field(data, n, stride, offset, size):
    """A signed big-endian binary field of the first n fixed-length records, as int64 on the device."""
    b = data[:n * stride].view(n, stride)[:, offset:offset + size].to(torch.int64)
    v = torch.zeros(n, dtype=torch.int64, device=data.device)
    for k in range(size):
        v = (v << 8) | b[:, k]
    return torch.where(v >= (1 << (8 * size - 1)), v - (1 << (8 * size)), v)


def run_fixed(name, key, n_rec, sets, steps, warmup, emit, dev):
    """sets: [(label, python values)]."""
    rd = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters(string_views=True), columns=SYN_COLUMNS)
    data = synth.syn200(n_rec, seed=20261015, device=dev).view(-1)
    n_bytes, st = int(data.numel()), torch.cuda.current_stream()
    N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 1))
    kc = column_of(rd, key)
    value_cols = [c.index for c in rd.out_plan.columns if c.kind == "value" and c.out_type in N.OUT_WIDTH]
    for label, values in sets(data, n_rec):
        row = {"workload": name, "key": key, "records": n_rec, "set": label, "set_size": len(values)}
        compiled = compile_key_values(rd.plan, [key], values)
        builds = []
        for _ in range(warmup + steps):
            with KeySet(rd.plan, rd.native.handle, [key], None, compiled=compiled) as tmp:
                builds.append(tmp.info().build_ms)
        ks = KeySet(rd.plan, rd.native.handle, [key], None, compiled=compiled)
        info = ks.info()
        row.update(build_ms=round(statistics.median(builds[warmup:]), 4), capacity=info.capacity, n_distinct=info.n_distinct,
                   max_probe=info.max_probe, device_bytes=info.device_bytes)
        sel = rd._filter_records(None, data, n_bytes, n_rec, st, stride=200, sets=[ks], negate=[0])
        row["selectivity"] = round(sel["n"] / n_rec, 5)
        whole, (test, scan, em) = passes_median(
            lambda: rd._filter_records(None, data, n_bytes, n_rec, st, stride=200, sets=[ks], negate=[0]), rd, steps, warmup)
        row["keyed"] = {"filter_call_ms": round(whole, 4), "test_ms": round(test, 4), "scan_ms": round(scan, 4), "emit_ms": round(em, 4)}
        flt = [F.InSet(ks)]
        row["keyed_filter_plus_decode_ms"] = round(median_ms(lambda: rd.decode_device(data, n_bytes, filters=flt), steps, warmup), 4)
        # (a) decode everything, torch.isin, boolean indexing
        members = torch.tensor(values, dtype=torch.int64, device=dev)
        parts = {}

        def caller():
            b = rd.decode_device(data, n_bytes)
            col = b.cols[kc]["values"][:n_rec]
            mask = torch.isin(col.to(torch.int64), members)
            return [b.cols[c]["values"][:n_rec][mask] for c in value_cols]

        out = caller()
        assert int(out[0].numel()) == sel["n"], (int(out[0].numel()), sel["n"])   # (BR-ID / CUST-KEY are never null)
        parts["decode_all_ms"] = round(median_ms(lambda: rd.decode_device(data, n_bytes), steps, warmup), 4)
        row["caller_decode_isin_index_ms"] = round(median_ms(caller, steps, warmup), 4)
        row["caller_parts"] = parts
        del out
        # (b) one OP_IN of 64 literals on the same field
        table, un = F.compile_filters(rd.plan, [F.In(key, values[:64])])
        assert not un
        whole_b, (test_b, scan_b, em_b) = passes_median(
            lambda: rd._filter_records(table, data, n_bytes, n_rec, st, stride=200), rd, steps, warmup)
        row["floor_in64"] = {"filter_call_ms": round(whole_b, 4), "test_ms": round(test_b, 4), "scan_ms": round(scan_b, 4),
                             "emit_ms": round(em_b, 4)}
        row["test_over_floor"] = round(test / test_b, 3)
        row["keyed_over_caller"] = round(row["keyed_filter_plus_decode_ms"] / row["caller_decode_isin_index_ms"], 3)
        ks.close()
        emit(row)
    rd.close()
    del data
    torch.cuda.empty_cache()


def br_sets(data, n_rec):
    out = []
    for size, target in ((64, 0.01), (1000, 0.10), (20000, 0.50)):
        inside = min(size, round(target * 19999))
        step = 19999 // inside
        vals = [-9999 + step * j for j in range(inside)] + [20000 + j for j in range(size - inside)]
        out.append((f"{size} values, target {target:.0%}", vals))
    return out


def cust_sets(data, n_rec):
    keys = be_field(data, n_rec // 2, 200, 4 + 2 + 8, 4)
    return [(f"{n_rec // 2} keys of the first half", keys.cpu().tolist())]


def run_rdw(n_rec, steps, warmup, emit, dev):
    p = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID", generate_record_id=True, string_views=True,
                         segment_id_redefine_map={k: v for k, v in synth.RDW_NARROW_SEGMENTS.items()})
    rd = VarLenNestedReader(synth.RDW_NARROW_COPYBOOK, p, columns=RDW_COLUMNS)
    size = synth.rdw_narrow_large_size(n_rec, device=dev)
    buf = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
    data, _ = synth.rdw_narrow_large(n_rec, device=dev, out=buf)
    off, ln = rd.frame(data, size)
    n = int(off.numel())
    st = torch.cuda.current_stream()
    N.check(N.load().cbx_plan_set_profiling(rd.native.handle, 1))
    first = off[:100_000].cpu()
    host = data[:int(first[-1]) + 64].cpu().numpy()
    values = sorted({bytes(host[o + 5:o + 15]).decode("cp037") for o in first.tolist()})
    row = {"workload": "rdw_narrow", "key": "COMPANY-ID", "records": n, "set": "keys of the first 100,000 records",
           "set_size": len(values)}
    compiled = compile_key_values(rd.plan, ["COMPANY-ID"], values)
    builds = []
    for _ in range(warmup + steps):
        with KeySet(rd.plan, rd.native.handle, ["COMPANY-ID"], None, compiled=compiled) as tmp:
            builds.append(tmp.info().build_ms)
    ks = KeySet(rd.plan, rd.native.handle, ["COMPANY-ID"], None, compiled=compiled)
    info = ks.info()
    row.update(build_ms=round(statistics.median(builds[warmup:]), 4), capacity=info.capacity, n_distinct=info.n_distinct,
               max_probe=info.max_probe, device_bytes=info.device_bytes)
    call = lambda: rd._filter_records(None, data, size, n, st, rec_off=off, rec_len=ln, sets=[ks], negate=[0])   # noqa: E731
    sel = call()
    row["selectivity"] = round(sel["n"] / n, 5)
    whole, (test, scan, em) = passes_median(call, rd, steps, warmup)
    row["keyed"] = {"filter_call_ms": round(whole, 4), "test_ms": round(test, 4), "scan_ms": round(scan, 4), "emit_ms": round(em, 4)}
    flt = [F.InSet(ks)]
    row["keyed_filter_plus_decode_ms"] = round(
        median_ms(lambda: rd.decode_selected(data, size, rd.filter(data, size, (off, ln), flt)), steps, warmup), 4)
    row["caller_parts"] = {"decode_all_ms": round(median_ms(lambda: rd.decode_device(data, size, off, ln), steps, warmup), 4)}
    row["caller_decode_isin_index_ms"] = None       # torch.isin takes no strings: the caller's filter runs on the host
    table, un = F.compile_filters(rd.plan, [F.In("COMPANY-ID", values[:64])])
    assert not un
    whole_b, (test_b, scan_b, em_b) = passes_median(
        lambda: rd._filter_records(table, data, size, n, st, rec_off=off, rec_len=ln), rd, steps, warmup)
    row["floor_in64"] = {"filter_call_ms": round(whole_b, 4), "test_ms": round(test_b, 4), "scan_ms": round(scan_b, 4),
                         "emit_ms": round(em_b, 4)}
    row["test_over_floor"] = round(test / test_b, 3)
    ks.close()
    emit(row)
    rd.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="syn200_br,syn200_cust,rdw_narrow")
    ap.add_argument("--records", type=int, default=0, help="records per batch (default: 50 M / 1 M / 10 M)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keyset.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    emit({"tool": "bench_keyset", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup})
    for name in args.workloads.split(","):
        if name == "syn200_br":
            run_fixed(name, "BR-ID", args.records or 50_000_000, br_sets, args.steps, args.warmup, emit, dev)
        elif name == "syn200_cust":
            run_fixed(name, "CUST-KEY", args.records or 1_000_000, cust_sets, args.steps, args.warmup, emit, dev)
        elif name == "rdw_narrow":
            run_rdw(args.records or 10_000_000, args.steps, args.warmup, emit, dev)
        else:
            raise SystemExit(f"unknown workload {name}")


if __name__ == "__main__":
    main()
