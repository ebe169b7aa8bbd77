"""bench.py --dump-outputs: the sampled .npy files of a small job against the host view of the same
output columns (DecodedBatch.host_column, the path the parity tests pin against the oracle) --
every layout the dump reads: slot rows, string views, Utf8 / large-string offsets, several batches,
OCCURS DEPENDING ON lists.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import bench  # noqa: E402

from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.reader import DecodedBatch  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _job(workload, strings, records, batch):
    dev = torch.device("cuda", 0)
    if workload in ("syn200", "synstr200"):
        return bench._Fixed(workload, records, dev, 0, 0, strings, batch, None,
                            pipeline="0,0" if batch else "")
    return bench._VarLen(workload, records, dev, 0, 1, 0, strings, True, 100, batch, pieces=1)


def _expected_strings(h, info, valid, idx):
    out = []
    for s in range(info.n_slots):
        row = []
        for k, r in enumerate(idx):
            if not valid[s, k]:
                row.append(b"")
            elif "strings" in h:
                row.append(bytes(h["strings"][s][r]))
            else:
                o = h["offsets"][s]
                row.append(bytes(h["data"][int(o[r]):int(o[r + 1])]))
        out.append(row)
    return out


def _check_part(plan, cols, m, load):
    idx = load("records")
    assert idx.dtype == np.float64
    idx = idx.astype(np.int64)
    assert 1 <= len(idx) <= m and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < m
    batch = DecodedBatch(plan, m, cols, 0, False, False)
    seen = 0
    for ci, info in enumerate(plan.columns):
        if info.kind == "list_offsets":
            continue
        name = bench.dump_column_name(ci, info)
        h = batch.host_column(ci)
        valid = np.asarray(h["validity"])[:, idx].astype(bool)
        got_valid = load(name + ".valid")
        assert got_valid.dtype == np.float32 and np.array_equal(got_valid, valid.astype(np.float32)), name
        ot = info.out_type
        if ot in (N.O_STRING, N.O_BINARY):
            exp = _expected_strings(h, info, valid, idx)
            ln, by = load(name + ".length"), load(name + ".bytes")
            assert ln.dtype == np.float32 and by.dtype == np.float32
            assert np.array_equal(ln, np.array([[len(b) for b in row] for row in exp], dtype=np.float32)), name
            assert by.shape == (info.n_slots, len(idx), max(1, int(ln.max())))
            for s, row in enumerate(exp):
                for k, b in enumerate(row):
                    want = np.zeros(by.shape[2], dtype=np.float32)
                    want[:len(b)] = np.frombuffer(b, dtype=np.uint8)
                    assert np.array_equal(by[s, k], want), (name, s, idx[k])
            seen += 1
            continue
        v = np.asarray(h["values"])
        got = load(name + ".values")
        if ot == N.O_DEC128:
            v = np.where(valid[..., None], v.reshape(info.n_slots, m, 2)[:, idx].astype(np.int64), 0)
            exp = np.stack([v[..., 1] >> 32, v[..., 1] & 0xFFFFFFFF, v[..., 0] >> 32, v[..., 0] & 0xFFFFFFFF], -1)
        else:
            v = np.where(valid, v.reshape(info.n_slots, m)[:, idx], 0)
            if ot in (N.O_I64, N.O_DEC64):
                v = v.astype(np.int64)
                exp = np.stack([v >> 32, v & 0xFFFFFFFF], -1)
                # the two words give the value back exactly
                assert np.array_equal((got[..., 0].astype(np.int64) << 32) | got[..., 1].astype(np.int64), v), name
            elif ot == N.O_F32:
                exp = v.astype(np.int32).view(np.float32)
            elif ot == N.O_F64:
                exp = v.astype(np.int64).view(np.float64)
            else:
                exp = v.astype(np.int32)
        assert got.dtype == (np.float32 if ot == N.O_F32 else np.float64), name
        assert got.shape == exp.shape and np.array_equal(got, exp.astype(got.dtype), equal_nan=True), name
        seen += 1
    return seen


@pytest.mark.parametrize("workload,strings,records,batch", [
    ("syn200", "views", 3001, 0),          # slot rows of every numeric type + string views
    ("synstr200", "offsets", 1500, 600),   # Utf8 offsets, three batches on two plans
    ("synstr200", "large", 700, 0),        # large-string offsets
    ("wide_odo", "views", 30, 0),          # OCCURS DEPENDING ON lists, segment redefines
])
def test_dump_outputs_match_the_host_view(tmp_path, workload, strings, records, batch):
    job = _job(workload, strings, records, batch)
    job.prepare(torch.cuda.current_stream())
    dirs = []
    for rep in range(2):   # the same arguments give the same files
        job.step(1)
        torch.cuda.synchronize()
        for h, st in getattr(job, "targets", [(job.h, job.stream)]):
            N.check(job.L.cbx_plan_check(h, st))
        d = str(tmp_path / f"dump{rep}")
        wrote = bench.dump_outputs(job, d, 0, 1)
        files = sorted(os.listdir(d))
        assert wrote["files"] == len(files) and all(f.endswith(".npy") for f in files)
        assert wrote["bytes"] == sum(np.load(os.path.join(d, f)).nbytes for f in files) <= bench.DUMP_LIMIT_BYTES
        dirs.append((d, files))
    assert dirs[0][1] == dirs[1][1]
    for f in dirs[0][1]:
        assert np.array_equal(np.load(os.path.join(dirs[0][0], f)), np.load(os.path.join(dirs[1][0], f)),
                              equal_nan=True), f
    plan = job.rd.plan
    assert len(job.parts) == (3 if batch else 1)
    n_files = 0
    for b, (_, m, cols, _) in enumerate(job.parts):
        prefix = f"batch{b}_" if len(job.parts) > 1 else ""
        used = []

        def load(name):
            used.append(prefix + name + ".npy")
            return np.load(os.path.join(dirs[0][0], prefix + name + ".npy"))

        assert _check_part(plan, cols, m, load) > 0
        n_files += len(used)
        if workload != "wide_odo":   # a small batch of narrow records is dumped whole
            assert len(load("records")) == m
    assert n_files == len(dirs[0][1])   # nothing in the directory but what was checked
