"""The reference's small known-answer specs, as data: tests/golden/specs/<name>.json, one file per test
case of a spec (SCT = spark-cobol/src/test/scala/za/co/absa/cobrix/spark/cobol/, CPT =
cobol-parser/src/test/scala/za/co/absa/cobrix/cobol/).

Each fixture holds the spec's copybook (`copybook`, or `copybook_file` under tests/golden/data), the
Spark options exactly as the spec passes them, the input bytes (`data_hex`, or `data`: one file or a
list of files under tests/golden/data) and what the spec asserts:

  expected / expected_file   the rows of df.toJSON (a list, or the spec's JSON text so that decimals keep
                             their printed scale), after `sort` (orderBy) and `take`
  count                      df.count
  index_entries              the number of sparse index entries
  error                      {"type": the JVM exception, "contains": a substring of its message}
  parses                     the copybook parses (a parser spec: no data)
  float_close                Test03IbmFloats: |value - field| below a bound, in the field's own precision
  schema_file / layout_file  df.schema.json / Copybook.generateRecordLayoutPositions

`replicate`: the rows do not depend on the file around them, so the file repeated N times gives the rows
repeated, Record_Id advancing by `records_per_copy` per copy (test_reference_specs.py proves the rule on
the oracle before the GPU tests rely on it).  The CPU suite replays every fixture through the oracle,
the GPU suite through libcobrix_hip.so.
"""
from __future__ import annotations

import copy
import json
import os
from decimal import Decimal
from typing import Any, Dict, List, Optional

import numpy as np

import goldens as G
import golden_cases as GC

SPECS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "specs")
COPIES = 65          # more than one 64-record tile from files of 2 to 12 records (at most 780 records)

# JVM exception -> what the host raises for it (cobrix_amd/options.py, reader.py)
EXCEPTIONS = {"IllegalArgumentException": ValueError, "IllegalStateException": ValueError}


def files() -> List[str]:
    return sorted(os.listdir(SPECS))


def load(name: str) -> Dict[str, Any]:
    with open(os.path.join(SPECS, name + ".json"), encoding="utf-8") as f:
        return json.load(f, parse_float=Decimal)


def params(fx):
    from cobrix_amd.options import parse_options
    GC.register_custom_code_pages()
    return parse_options(fx["options"])


def copybook_text(fx) -> str:
    if "copybook" in fx:
        return fx["copybook"]
    return G.read(fx["copybook_file"]).decode("latin-1")


def data_files(fx, copies: int = 1) -> List[bytes]:
    """The input files, in the order the reference lists them."""
    if "data_hex" in fx:
        return [bytes.fromhex(fx["data_hex"]) * copies]
    names = fx["data"] if isinstance(fx["data"], list) else [fx["data"]]
    return [G.read(*n.split("/")) * copies for n in names]


def expected_rows(fx, copies: int = 1) -> Optional[List[Any]]:
    """The rows the spec asserts (None when it asserts none); for `copies` > 1 those rows repeated, each
    copy's Record_Id moved on by the copy's records."""
    if "expected_file" in fx:
        rows = GC.load_json_values(fx["expected_file"])
    elif "expected" in fx:
        e = fx["expected"]
        rows = json.loads(e, parse_float=Decimal) if isinstance(e, str) else e
    else:
        return None
    if copies == 1:
        return rows
    assert fx.get("replicate")
    out = []
    for k in range(copies):
        for r in copy.deepcopy(rows):
            if "Record_Id" in r:
                r["Record_Id"] += k * fx["records_per_copy"]
            out.append(r)
    return out


def oracle_rows(cb, p, var_len: bool, files_: List[bytes]) -> List[dict]:
    """The rows of the reference's read, restated (oracle/reader_oracle.py): every file in turn."""
    from oracle import oracle as O
    from oracle import reader_oracle as RO
    rows: List[dict] = []
    for file_id, data in enumerate(files_):
        if p.is_text:
            off, ln, vb = O.frame_text(data, cb.record_size)
            res = O.decode_var(cb, data + b"\0" * (vb - len(data)), off, ln)
            rows += O.rows(res, collapse_root=p.schema_policy == "collapse_root")
        elif var_len:
            rows += RO.var_len_rows(cb, data, p, file_id)
        else:
            rows += RO.fixed_len_rows(cb, data, p)
    return rows


def check_rows(fx, rows: List[dict], copies: int = 1) -> List[str]:
    """`rows` (a whole read, unsorted) against everything the fixture asserts about rows."""
    errs: List[str] = []
    if "count" in fx and len(rows) != fx["count"] * copies:
        errs.append(f"{len(rows)} rows, the spec asserts {fx['count'] * copies}")
    exp = expected_rows(fx, copies)
    if exp is not None:
        got = GC.spark_order(rows, fx.get("sort"))[: fx.get("take", len(rows))]
        if len(got) != len(exp):   # compare_rows tolerates extra rows
            errs.append(f"{len(got)} rows, the spec lists {len(exp)}")
        errs += G.compare_rows(got, exp)
    if "float_close" in fx:
        errs += float_close(fx, rows)
    return errs


def float_close(fx, rows: List[dict]) -> List[str]:
    """Test03IbmFloats.assertFloatEqual / assertDoubleEqual (:43-49): the difference is taken in the
    field's own type, its absolute value compared as a double.  The spec looks at the first row; every
    record of its files holds the same bytes, so every row is held to it."""
    fc = fx["float_close"]
    errs = []
    if not rows:
        errs.append("no rows")
    for i, r in enumerate(rows):
        for name, want in fc.items():
            if name == "row":
                continue
            v = r.get(name)
            if want["as"] == "float":
                ok = isinstance(v, np.float32) and abs(float(v - np.float32(float(want["value"])))) < float(want["below"])
            else:
                ok = isinstance(v, (float, np.float64)) and abs(float(v) - float(want["value"])) < float(want["below"])
            if not ok:
                errs.append(f"row{i}.{name}: {v!r} is not within {want['below']} of {want['value']}")
    return errs
