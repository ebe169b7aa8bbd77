"""Measure lookup joins (cbx_key_map_create_from_records, cbx_join_records, cbx_select_ordinals) against their floor
and against the path they replace.

Workloads, in one process on one GPU:
  syn200_br:      SYN200 fact records (default 50 M) joined by BR-ID to a dimension of about 20 k unique BR-IDs (the
                  first record of every BR-ID among 200 k SYN200 records of another seed).
  syn200_br_sel:  the same with a selective fact filter (REC-ID < 50,000,000: about 5 % of the rows).
  syn200_cust:    the same fact records joined by CUST-KEY to a nearly unique dimension: the 1 M SYN200 records of
                  another seed that REC-ID < 500,000,000 keeps (about 500 k keys).
  rdw_narrow:     rdw_narrow_large fact records (default 10 M) joined by the string key COMPANY-ID to the first
                  200 k records of the same generator under another seed (duplicate keys: the first row).
Per case:
  map:      `key_map_of_device` -- distinct, convert and fill (init + fill + stats) from the library's HIP events
            (profiling on), the whole call as wall time, host waits included; fill_over_distinct beside them.
  join:     the test / scan / emit passes of cbx_join_records (INNER, with d_match_rows) from HIP events, and the call
            without the decode as wall time.
  floor:    cbx_filter_records_keyed with the map's own set on the same input: its test / scan / emit passes.
  replaced: (numeric keys) the path the join replaces, in the same process: projected decode of both key columns, a
            torch join (sort + searchsorted), two selections built with torch, both decodes -- wall time, beside the
            new path end to end (join + decode, dimension()).
Every figure is the median of --steps repetitions after --warmup.  One JSON line per case on stdout (and appended to
--out).  --resource-usage FILE compiles the library once more with the compiler's resource-usage remarks and writes
those of the new kernels there (no GPU needed).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("keymap_fill_kernel", "keymap_test_kernel", "keymap_emit_kernel", "ordinals_gather_kernel", "keymap_stats_kernel",
           "keymap_init_kernel", "keyset_test_kernel", "keyset_distinct_kernel")


def resource_usage(path: str) -> None:
    """The -Rpass-analysis=kernel-resource-usage remarks of the new kernels and of the two they are compared with."""
    csrc = os.path.join(ROOT, "cobrix_amd", "csrc")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, os.path.join(csrc, "cbx_capi.hip"), "-lhiprtc"], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-4000:])
    write_resource_usage(r.stderr, path)


def write_resource_usage(remarks: str, path: str) -> None:
    out, take = [], 0
    for line in remarks.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            take = 11 if any(f"{len(k)}{k}" in m.group(1) for k in KERNELS) else 0
            if take:
                out.append("Function Name: " + m.group(1))
            continue
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if m and take:
            out.append("    " + m.group(1).strip())
            take -= 1
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="syn200_br,syn200_br_sel,syn200_cust,rdw_narrow")
    ap.add_argument("--records", type=int, default=0, help="fact records (default: 50 M SYN200 / 10 M rdw_narrow)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--resource-usage", default="", help="write the new kernels' resource-usage remarks here and exit")
    ap.add_argument("--remarks-from", default="", help="with --resource-usage: a saved compiler log to take them from")
    args = ap.parse_args()
    if args.resource_usage:
        if args.remarks_from:
            write_resource_usage(open(args.remarks_from).read(), args.resource_usage)
        else:
            resource_usage(args.resource_usage)
        return
    import torch

    from cobrix_amd import filter as F
    from cobrix_amd import native as N
    from cobrix_amd import synth
    from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader

    if not torch.cuda.is_available():
        raise SystemExit("bench_keymap.py measures on the GPU: no device found")
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

    def filter_passes(rd):
        t = [ctypes.c_float(0) for _ in range(3)]
        N.check(L.cbx_filter_pass_times(rd.native.handle, *[ctypes.byref(x) for x in t]))
        return [x.value for x in t]

    def measure(row, fact, fdata, f_bytes, f_src, f_n, dim, ddata, d_bytes, d_framing, key, dkey, dfilters, ffilters, max_values,
                replaced):
        """fact / dim: readers; f_src: `_join_records`' source keywords; d_framing: what follows d_data, n_bytes in the
        dimension's device entry points."""
        st = torch.cuda.current_stream()
        infos = []

        def build():
            with dim.key_map_of_device(ddata, d_bytes, *d_framing, [dkey], fact, [key], filters=dfilters, max_values=max_values) as km:
                infos.append(km.source_info)

        ms, _ = wall_ms(build)
        si = infos[-1]
        row.update(n_dim_rows=si.n_rows, n_values=si.n_source_keys - si.n_dropped, n_duplicate_keys=si.n_duplicate_keys,
                   max_rows_per_key=si.max_rows_per_key)
        row["map"] = {"distinct_ms": med([s.distinct_ms for s in infos]), "convert_ms": med([s.convert_ms for s in infos]),
                      "fill_ms": med([s.fill_ms for s in infos]), "key_map_of_wall_ms": round(ms, 4)}
        row["map"]["fill_over_distinct"] = round(row["map"]["fill_ms"] / max(row["map"]["distinct_ms"], 1e-9), 3)
        km = dim.key_map_of_device(ddata, d_bytes, *d_framing, [dkey], fact, [key], filters=dfilters, max_values=max_values)
        passes, kept = [], []

        def join():
            res = fact._join_records(km, "inner", ffilters, "first", fdata, f_bytes, f_n, st, decode=False, **f_src)
            passes.append(fact.join_pass_times())
            kept.append(res.selection["n"])

        ms, _ = wall_ms(join)
        row["kept"] = kept[-1]
        row["join"] = {"test_ms": med([p[0] for p in passes]), "scan_ms": med([p[1] for p in passes]),
                       "emit_ms": med([p[2] for p in passes]), "call_wall_ms": round(ms, 4)}
        table, sets, negate, un = F.compile_filters_with_sets(fact.plan, list(ffilters or []) + [F.InSet(km.key_set)])
        assert not un, un.reasons
        fl, floor_kept = [], []

        def floor():
            out = fact._filter_records(table, fdata, f_bytes, f_n, st, sets=sets, negate=negate, **f_src)
            fl.append(filter_passes(fact))
            floor_kept.append(out["n"])

        ms, _ = wall_ms(floor)
        assert floor_kept[-1] == kept[-1], (floor_kept[-1], kept[-1])
        row["floor"] = {"test_ms": med([p[0] for p in fl]), "scan_ms": med([p[1] for p in fl]), "emit_ms": med([p[2] for p in fl]),
                        "call_wall_ms": round(ms, 4)}
        row["join_test_over_floor"] = round(row["join"]["test_ms"] / max(row["floor"]["test_ms"], 1e-9), 3)
        row["join_call_over_floor"] = round(row["join"]["call_wall_ms"] / max(row["floor"]["call_wall_ms"], 1e-9), 3)
        if replaced is not None:
            def new_path():
                res = fact._join_records(km, "inner", ffilters, "first", fdata, f_bytes, f_n, st, **f_src)
                d = res.dimension()
                return res.batch.n_rec + d.n_rec

            ms_new, n_new = wall_ms(new_path)
            row["end_to_end"] = {"join_ms": round(ms_new, 4)}
            emit(dict(row, partial=True))   # (the replaced path allocates the most: keep what is measured so far)
            ms_old, n_old = wall_ms(replaced)
            assert n_new == n_old == 2 * kept[-1], (n_new, n_old, kept[-1])
            row["end_to_end"].update(replaced_ms=round(ms_old, 4), join_over_replaced=round(ms_new / ms_old, 4))
        km.close()
        emit(row)

    def key_column(rd, batch, name):
        plan = rd.out_plan
        fi = plan.field_of_node[id(rd.copybook.get_field_by_name(name))]
        return batch.cols[plan.fields[fi].column]["values"][:batch.n_rec]

    def fixed_selection(rd, idx, stride, device):
        sel, cs = rd._empty_selection(int(idx.numel()), device)
        n = int(idx.numel())
        sel["rec_off"][:n] = idx * stride
        sel["rec_len"][:n] = stride
        sel["record_id"][:n] = idx
        sel["segment"][:n] = -1
        sel["n"], sel["struct"] = n, cs
        return sel

    emit({"tool": "bench_keymap", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup})
    names = args.workloads.split(",")
    if any(n.startswith("syn200") for n in names):
        n_fact = args.records or 50_000_000
        fact = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters())
        dim = FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters())
        fkey = {k: FixedLenNestedReader(synth.SYN200_COPYBOOK, ReaderParameters(), columns=[k]) for k in ("BR-ID", "CUST-KEY", "REC-ID")}
        for rd in (fact, dim):
            N.check(L.cbx_plan_set_profiling(rd.native.handle, 1))
        fdata = synth.syn200(n_fact, seed=20261015, device=dev).view(-1)
        f_bytes = int(fdata.numel())
        st = torch.cuda.current_stream()
        for name in names:
            if not name.startswith("syn200"):
                continue
            key = "CUST-KEY" if name == "syn200_cust" else "BR-ID"
            ffilters = [F.LessThan("REC-ID", 50_000_000)] if name == "syn200_br_sel" else None
            dfilters, max_values = None, 65536
            if name == "syn200_cust":
                ddata = synth.syn200(1_000_000, seed=7, device=dev).view(-1)
                dfilters, max_values = [F.LessThan("REC-ID", 500_000_000)], 1 << 20
            else:   # the first record of every BR-ID: a dimension with unique keys
                raw = synth.syn200(200_000, seed=7, device=dev)
                br = (raw[:, 4].to(torch.int64) << 8) | raw[:, 5].to(torch.int64)
                order = torch.argsort(br, stable=True)
                first = torch.ones_like(order, dtype=torch.bool)
                first[1:] = br[order][1:] != br[order][:-1]
                ddata = raw[torch.sort(order[first]).values].contiguous().view(-1)
            d_bytes = int(ddata.numel())

            def replaced(key=key, ffilters=ffilters, dfilters=dfilters, ddata=ddata, d_bytes=d_bytes):
                fb = fkey[key].decode_device(fdata, f_bytes, filters=None)
                fk = key_column(fkey[key], fb, key).to(torch.int64)
                keep = torch.ones_like(fk, dtype=torch.bool)
                if ffilters:
                    rb = fkey["REC-ID"].decode_device(fdata, f_bytes)
                    keep &= key_column(fkey["REC-ID"], rb, "REC-ID").to(torch.int64) < 50_000_000
                db = fkey[key].decode_device(ddata, d_bytes)
                dk = key_column(fkey[key], db, key).to(torch.int64)
                d_idx = torch.arange(dk.numel(), device=dev)
                if dfilters:
                    rb = fkey["REC-ID"].decode_device(ddata, d_bytes)
                    d_idx = d_idx[key_column(fkey["REC-ID"], rb, "REC-ID").to(torch.int64) < 500_000_000]
                    dk = dk[d_idx]
                sk, order = torch.sort(dk, stable=True)
                pos = torch.searchsorted(sk, fk).clamp(max=sk.numel() - 1)
                keep &= sk[pos] == fk
                f_idx = torch.nonzero(keep).view(-1)
                m_idx = d_idx[order[pos[f_idx]]]
                a = fact._decode_selection(fdata, f_bytes, fixed_selection(fact, f_idx, 200, dev), False, st)
                b = dim._decode_selection(ddata, d_bytes, fixed_selection(dim, m_idx, 200, dev), False, st)
                return a.n_rec + b.n_rec

            row = {"workload": name, "key": key, "fact_records": n_fact, "dimension_records": d_bytes // 200,
                   "fact_filter": repr(ffilters) if ffilters else None, "dimension_filter": repr(dfilters) if dfilters else None}
            measure(row, fact, fdata, f_bytes, {"stride": 200}, n_fact, dim, ddata, d_bytes, (), key, key, dfilters, ffilters,
                    max_values, replaced)
            del ddata
        del fdata
        for rd in [fact, dim] + list(fkey.values()):
            rd.close()
        torch.cuda.empty_cache()
    if "rdw_narrow" in names:
        n_fact = args.records or 10_000_000
        p = ReaderParameters(is_record_sequence=True, segment_field="SEGMENT-ID",
                             segment_id_redefine_map={k: v for k, v in synth.RDW_NARROW_SEGMENTS.items()})
        fact = VarLenNestedReader(synth.RDW_NARROW_COPYBOOK, p)
        dim = VarLenNestedReader(synth.RDW_NARROW_COPYBOOK, p)
        for rd in (fact, dim):
            N.check(L.cbx_plan_set_profiling(rd.native.handle, 1))
        sides = []
        for n, seed in ((n_fact, 20261016), (200_000, 5)):
            size = synth.rdw_narrow_large_size(n, seed=seed, device=dev)
            buf = torch.zeros(size + 64, dtype=torch.uint8, device=dev)
            data, _ = synth.rdw_narrow_large(n, seed=seed, device=dev, out=buf)
            off, ln = fact.frame(data, size)
            sides.append((data, size, off, ln))
        (fdata, f_bytes, foff, fln), (ddata, d_bytes, doff, dln) = sides
        row = {"workload": "rdw_narrow", "key": "COMPANY-ID", "fact_records": int(foff.numel()), "dimension_records": int(doff.numel()),
               "fact_filter": None, "dimension_filter": None}
        measure(row, fact, fdata, f_bytes, {"rec_off": foff, "rec_len": fln}, int(foff.numel()), dim, ddata, d_bytes, ((doff, dln),),
                "COMPANY-ID", "COMPANY-ID", None, None, 1 << 18, None)
        fact.close()
        dim.close()


if __name__ == "__main__":
    main()
