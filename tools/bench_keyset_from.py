"""Measure key sets built on the device from a second file's records (cbx_key_set_create_from_records) against the
host round trip they replace.

Workloads, in one process on one GPU (the master sizes of tools/bench_keyset.py):
  syn200_br:   the 19,999 distinct BR-IDs of SYN200 records (default 50 M).
  syn200_cust: the nearly unique CUST-KEYs of the half of SYN200 records (default 1 M) that REC-ID < 500,000,000 keeps
               (about 500 k keys).
  rdw_narrow:  the COMPANY-IDs (ten digits, a string key) of the rdw_narrow_large records (default 10 M) whose
               COMPANY-ID starts with "00" (about 100 k keys).
Per case:
  device: `key_set_of_device` -- the distinct, convert and build passes from the library's HIP events (profiling on),
          and the whole call as wall time, host waits included;
  host:   the path it replaces, in the same process: `aggregate_by_device` on the source with no aggregates,
          `GroupedAggregateResult` to Python values, `key_set(...)` on the probe reader (compile_key_values, upload,
          build) -- wall time, with the grouped call's accumulate pass beside it;
  floor:  the test pass of cbx_filter_records with the source filter and one OP_IN on the key field (64 literals less
          the source filter's own: the table holds 64).
Every figure is the median of --steps repetitions after --warmup.  One JSON line per case on stdout (and appended to
--out).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd import synth  # noqa: E402
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader  # noqa: E402


def wall_ms(fn, steps, warmup):
    """Median wall time of fn in ms (device idle before and after), and what each timed repetition returned."""
    out, ms = [], []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
            out.append(r)
    return statistics.median(ms), out


def filter_test_ms(rd):
    t = [ctypes.c_float(0) for _ in range(3)]
    N.check(N.load().cbx_filter_pass_times(rd.native.handle, *[ctypes.byref(x) for x in t]))
    return t[0].value


def measure(row, source, probe, key, filters, max_values, src_args, src_kw, steps, warmup, emit):
    """source / probe: readers of the same copybook; src_args / src_kw: what follows d_data, n_bytes in the source's
    device entry points (the framing) and `_filter_records`' source keywords."""
    data, n_bytes = src_args[0], src_args[1]
    framing = src_args[2:]

    def device():
        with source.key_set_of_device(data, n_bytes, *framing, [key], probe, filters=filters, max_values=max_values) as ks:
            return ks.source_info, ks.info()

    ms, seen = wall_ms(device, steps, warmup)
    si, ki = seen[-1]
    row.update(n_rows=si.n_rows, n_null_rows=si.n_null_rows, n_source_keys=si.n_source_keys, n_dropped=si.n_dropped,
               source_capacity=si.source_capacity, workspace_bytes=si.workspace_bytes, set_capacity=ki.capacity,
               n_distinct=ki.n_distinct, max_probe=ki.max_probe)
    row["device"] = {"distinct_ms": round(statistics.median(s.distinct_ms for s, _ in seen), 4),
                     "convert_ms": round(statistics.median(s.convert_ms for s, _ in seen), 4),
                     "build_ms": round(statistics.median(k.build_ms for _, k in seen), 4),
                     "key_set_of_wall_ms": round(ms, 4)}
    parts = {"aggregate_by": [], "to_python": [], "key_set": [], "accumulate": []}

    def host():
        t0 = time.perf_counter()
        res = source.aggregate_by_device(data, n_bytes, *framing, [key], [], filters=filters, max_groups=max_values)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        parts["accumulate"].append(source.group_pass_times()[1])
        keys = list(res.groups)
        t2 = time.perf_counter()
        with probe.key_set([key], keys) as ks:
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            n = ks.info().n_distinct
        parts["aggregate_by"].append((t1 - t0) * 1e3)
        parts["to_python"].append((t2 - t1) * 1e3)
        parts["key_set"].append((t3 - t2) * 1e3)
        return n

    ms_h, ns = wall_ms(host, steps, warmup)
    assert ns[-1] == ki.n_distinct, (ns[-1], ki.n_distinct)   # (a null group adds no member)
    row["host"] = {"wall_ms": round(ms_h, 4)}
    row["host"].update({k + "_ms": round(statistics.median(v[-steps:]), 4) for k, v in parts.items()})
    # the floor: the filter stage's test pass over the same records and field
    res = source.aggregate_by_device(data, n_bytes, *framing, [key], [], filters=filters, max_groups=max_values)
    some = [k[0] for k in list(res.groups)[:65] if k[0] is not None]
    for n_lit in (64 - len(filters or []), 32, 8):   # (the literal table holds 64 literals, the source filter's among them)
        table, un = F.compile_filters(source.plan, list(filters or []) + [F.In(key, some[:n_lit])])
        if not un:
            break
    assert not un, un.reasons
    row["floor_in_literals"] = n_lit
    st = torch.cuda.current_stream()
    tests = []
    for k in range(warmup + steps):
        source._filter_records(table, data, n_bytes, row["records"], st, **src_kw)
        tests.append(filter_test_ms(source))
    row["floor_filter_test_ms"] = round(statistics.median(tests[warmup:]), 4)
    row["distinct_over_floor"] = round(row["device"]["distinct_ms"] / row["floor_filter_test_ms"], 3)
    row["device_over_host"] = round(row["device"]["key_set_of_wall_ms"] / row["host"]["wall_ms"], 4)
    emit(row)


def run_fixed(name, key, n_rec, filters, max_values, steps, warmup, emit, dev):
    source = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters())
    probe = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters())
    data = synth.syn200(n_rec, seed=20261015, device=dev).view(-1)
    N.check(N.load().cbx_plan_set_profiling(source.native.handle, 1))
    row = {"workload": name, "key": key, "records": n_rec, "source_filter": repr(filters) if filters else None,
           "max_values": max_values}
    measure(row, source, probe, key, filters, max_values, (data, int(data.numel())), {"stride": 200}, steps, warmup, emit)
    source.close()
    probe.close()
    del data
    torch.cuda.empty_cache()


def run_rdw(n_rec, max_values, steps, warmup, emit, dev):
    p = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID",
                         segment_id_redefine_map={k: v for k, v in synth.RDW_NARROW_SEGMENTS.items()})
    source = VarLenNestedReader(synth.RDW_NARROW_COPYBOOK, p)
    probe = VarLenNestedReader(synth.RDW_NARROW_COPYBOOK, p)
    size = synth.rdw_narrow_large_size(n_rec, device=dev)
    buf = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
    data, _ = synth.rdw_narrow_large(n_rec, device=dev, out=buf)
    off, ln = source.frame(data, size)
    N.check(N.load().cbx_plan_set_profiling(source.native.handle, 1))
    filters = [F.StringStartsWith("COMPANY-ID", "00")]
    row = {"workload": "rdw_narrow", "key": "COMPANY-ID", "records": int(off.numel()), "source_filter": repr(filters),
           "max_values": max_values}
    measure(row, source, probe, "COMPANY-ID", filters, max_values, (data, size, (off, ln)), {"rec_off": off, "rec_len": ln},
            steps, warmup, emit)
    source.close()
    probe.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="syn200_br,syn200_cust,rdw_narrow")
    ap.add_argument("--records", type=int, default=0, help="records per batch (default: 50 M / 1 M / 10 M)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keyset_from.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    emit({"tool": "bench_keyset_from", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup})
    for name in args.workloads.split(","):
        if name == "syn200_br":
            run_fixed(name, "BR-ID", args.records or 50_000_000, None, 65536, args.steps, args.warmup, emit, dev)
        elif name == "syn200_cust":
            run_fixed(name, "CUST-KEY", args.records or 1_000_000, [F.LessThan("REC-ID", 500_000_000)], 1 << 20, args.steps,
                      args.warmup, emit, dev)
        elif name == "rdw_narrow":
            run_rdw(args.records or 10_000_000, 1 << 18, args.steps, args.warmup, emit, dev)
        else:
            raise SystemExit(f"unknown workload {name}")


if __name__ == "__main__":
    main()
