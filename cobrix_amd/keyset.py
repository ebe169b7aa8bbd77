"""Key sets: a persistent hash set of key values on the device (`cbx_key_set_create`, include/cobrix_hip.h) for the
filters `InSet` / `NotInSet` of `cobrix_amd.filter` -- the semi join of a fact file against the keys of a dimension,
Spark's runtime `In` filters with hundreds to millions of values.

A key value is what `GroupedAggregateResult` yields for a key column: int for an integral column, Decimal (or int)
for a decimal one, str for a string column.  `compile_key_values` converts Python values with the exactness rules
of the filter literals; a value the column can never hold (not representable at its scale, out of its range, a
string longer than the field can produce) is dropped and counted, since it can never match; a tuple with a None is
dropped as well (it can never match under three-valued logic) and remembered, because NOT IN over a null is unknown
for every row.
"""
from __future__ import annotations

import ctypes
import decimal
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

import numpy as np

from . import aggregate as A
from . import native as N
from .filter import Unhandled


@dataclass
class CompiledKeyValues:
    """The host arrays cbx_key_set_create takes."""
    table: N.CbxGroupBy
    keys: List[A.KeySlot]
    values: np.ndarray          # uint8 [n_values * n_keys * sizeof(cbx_key_value)]
    str_bytes: np.ndarray       # uint8 [n_values * str_stride]
    str_stride: int
    str_off: List[int]
    n_values: int
    dropped: int                # values no row can hold
    has_null: bool              # a tuple held a None (dropped, not counted in `dropped`)


_VALUE_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<u8"), ("str_len", "<i4"), ("reserved", "<i4")])
assert _VALUE_DTYPE.itemsize == ctypes.sizeof(N.CbxKeyValue)
_M64 = 0xFFFFFFFFFFFFFFFF


def _numeric(f: N.CbxField, v: Any, name: str) -> Optional[int]:
    """The unscaled value at the column's scale; None when no row can hold it (filter._literal's rules)."""
    if isinstance(v, bool) or not isinstance(v, (int, decimal.Decimal)):
        raise Unhandled(f"{name}: key value {v!r} is not an int or Decimal (not exactly representable)")
    d = decimal.Decimal(v)
    if not d.is_finite():
        raise Unhandled(f"{name}: key value {v!r} is not finite")
    dec_col = f.out_type in (N.O_DEC64, N.O_DEC128)
    with decimal.localcontext() as ctx:
        ctx.prec = 200
        u = d.scaleb(f.out_scale if dec_col else 0)
        if u != u.to_integral_value():
            return None
        u = int(u)
    if dec_col:
        return u if abs(u) < 10 ** f.out_precision else None
    bits = 31 if f.out_type == N.O_I32 else 63
    return u if -(1 << bits) <= u < (1 << bits) else None


def compile_key_values(plan, names: Sequence[str], tuples) -> CompiledKeyValues:
    """The key columns `names` (what `compile_group_by` accepts, refused with its reasons) and the value tuples as the
    library's host arrays.  A single key column also takes plain values instead of 1-tuples."""
    names = list(names)
    try:
        table, keys = A.compile_group_by(plan, names)
    except A.Unhandled as e:
        raise Unhandled(str(e)) from None
    nk = len(keys)
    fields = [plan.fields[k.field] for k in keys]
    str_off, off = [], 0
    for k, f in zip(keys, fields):
        str_off.append(off)
        if k.is_str:
            off += 3 * f.size
    stride = off
    rows, blobs = [], []
    dropped, has_null = 0, False
    for t in tuples:
        if nk == 1 and not isinstance(t, (tuple, list)):
            t = (t,)
        if len(t) != nk:
            raise ValueError(f"key value {t!r}: {nk} key columns take tuples of {nk}")
        if any(v is None for v in t):
            has_null = True
            continue
        cells, blob, ok = [], bytearray(stride), True
        for k, f, name, v, so in zip(keys, fields, names, t, str_off):
            if k.is_str:
                if not isinstance(v, str):
                    raise Unhandled(f"{name}: a string column takes str key values, not {type(v).__name__}")
                b = v.encode("utf-8")
                if len(v) > f.size or len(b) > 3 * f.size:
                    ok = False
                    break
                blob[so:so + len(b)] = b
                cells.append((0, 0, len(b), 0))
            else:
                u = _numeric(f, v, name)
                if u is None:
                    ok = False
                    break
                cells.append((u & _M64, (u >> 64) & _M64, 0, 0))
        if not ok:
            dropped += 1
            continue
        rows.extend(cells)
        blobs.append(bytes(blob))
    values = np.array(rows, dtype=_VALUE_DTYPE) if rows else np.zeros(0, dtype=_VALUE_DTYPE)
    raw = np.frombuffer(b"".join(blobs), dtype=np.uint8) if stride and blobs else np.zeros(0, dtype=np.uint8)
    return CompiledKeyValues(table, keys, values.view(np.uint8).reshape(-1), raw, stride, str_off, len(blobs), dropped, has_null)


def _scale(k: A.KeySlot) -> int:
    return k.out_scale if k.out_type in (N.O_DEC64, N.O_DEC128) else 0


def compile_key_pairs(probe_plan, names: Sequence[str], source_plan, source_names: Sequence[str]):
    """The key tables of a set of `probe_plan` over `names` built from the `source_names` columns of another file's
    records (`cbx_key_set_create_from_records`): (probe table, source table).  Raises `Unhandled` with the reason:
    what `compile_group_by` refuses on either side (prefixed with the side), a different number of columns, a string
    column against a numeric one, a numeric pair of different scales (an integral column is scale 0; nothing is
    rescaled on the device).  Precision, width, encoding and output type may differ."""
    sides = []
    for side, plan, cols in (("probe", probe_plan, names), ("source", source_plan, source_names)):
        try:
            sides.append(A.compile_group_by(plan, list(cols)))
        except A.Unhandled as e:
            raise Unhandled(f"{side}: {e}") from None
    (ptable, pkeys), (stable, skeys) = sides
    if len(pkeys) != len(skeys):
        raise Unhandled(f"{len(pkeys)} probe key columns against {len(skeys)} source key columns")
    for k, (a, b, an, bn) in enumerate(zip(pkeys, skeys, names, source_names)):
        if a.is_str != b.is_str:
            raise Unhandled(f"key {k}: a string column against a numeric one ({an} / {bn})")
        if not a.is_str and _scale(a) != _scale(b):
            raise Unhandled(f"key {k}: scales {_scale(a)} and {_scale(b)} differ ({an} / {bn})")
    return ptable, stable


class KeySet:
    """A device key set of one reader's plan.  Owns the library handle: `close()` (or the context manager) frees
    the device memory; a closed set is refused by the filter compilation."""

    source_info: Optional[N.CbxKeysetSourceInfo] = None   # set by from_records

    @classmethod
    def from_records(cls, probe_plan, probe_handle, names: Sequence[str], source_plan, source_handle,
                     source_names: Sequence[str], d_data_ptr: int, n_bytes: int, n_rec: int, *, sel_struct=None,
                     rec_off_ptr=None, rec_len_ptr=None, stride: int = 0, start_offset: int = 0, filter_table=None,
                     max_values: int = 65536, max_workgroups: int = 0, stream=None) -> "KeySet":
        """A set of `probe_plan` over `names` built on the device from the `source_names` keys of another file's
        records (one source: a selection struct, framed records or a record stride).  `dropped` counts the distinct
        source keys the probe columns can never hold, `has_null` says whether a source row had a null key component
        (such rows are never members), `source_info` holds the library's counts.  Raises `Unhandled` when the
        columns do not pair and `GroupOverflow(max_values)` past max_values distinct source keys."""
        ptable, stable = compile_key_pairs(probe_plan, names, source_plan, source_names)
        info = N.CbxKeysetSourceInfo()
        h = ctypes.c_void_p()
        rc = N.load().cbx_key_set_create_from_records(
            probe_handle, ctypes.byref(ptable), source_handle, ctypes.byref(stable), d_data_ptr, n_bytes,
            ctypes.byref(sel_struct) if sel_struct is not None else None, rec_off_ptr, rec_len_ptr, n_rec, stride,
            start_offset, ctypes.byref(filter_table) if filter_table is not None else None, int(max_values),
            max_workgroups, ctypes.c_void_p(stream.cuda_stream if stream is not None else 0), ctypes.byref(h),
            ctypes.byref(info))
        if rc == N.CBX_E_CAPACITY and info.overflow:
            raise A.GroupOverflow(int(max_values))
        N.check(rc)
        self = cls.__new__(cls)
        self.plan = probe_plan
        self.names = list(names)
        self.dropped = info.n_dropped
        self.has_null = info.n_null_rows > 0
        self.n_values = info.n_source_keys - info.n_dropped
        self.source_info = info
        self.handle = h
        return self

    def __init__(self, plan, plan_handle, names: Sequence[str], values, stream=None,
                 compiled: Optional[CompiledKeyValues] = None):
        c = compiled if compiled is not None else compile_key_values(plan, names, values)
        self.plan = plan
        self.names = list(names)
        self.dropped = c.dropped
        self.has_null = c.has_null
        self.n_values = c.n_values
        off = (ctypes.c_int32 * N.CBX_GROUP_MAX_KEYS)(*c.str_off)
        h = ctypes.c_void_p()
        self.handle = None
        N.check(N.load().cbx_key_set_create(
            plan_handle, ctypes.byref(c.table), c.values.ctypes.data if c.n_values else None,
            c.str_bytes.ctypes.data if c.str_bytes.size else None, c.str_stride, ctypes.addressof(off), c.n_values,
            ctypes.c_void_p(stream.cuda_stream if stream is not None else 0), ctypes.byref(h)))
        self.handle = h

    @property
    def closed(self) -> bool:
        return self.handle is None

    def info(self) -> N.CbxKeysetInfo:
        """n_values, n_distinct, capacity, device_bytes, max_probe, build_ms (profiling on) of the build."""
        if self.closed:
            raise ValueError("the key set is closed")
        out = N.CbxKeysetInfo()
        N.check(N.load().cbx_key_set_info(self.handle, ctypes.byref(out)))
        return out

    def close(self) -> None:
        if self.handle is not None:
            N.load().cbx_key_set_destroy(self.handle)
            self.handle = None

    def __enter__(self) -> "KeySet":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (interpreter shutdown)
            pass

    def __repr__(self) -> str:
        return f"KeySet({self.names}, n_values={self.n_values}, dropped={self.dropped}, closed={self.closed})"


class DuplicateKeys(Exception):
    """A lookup join over a key map whose dimension has duplicate keys: it would return the first matching dimension
    row only (`duplicates="first"` asks for exactly that)."""

    def __init__(self, n_duplicate_keys: int, max_rows_per_key: int):
        super().__init__(f"{n_duplicate_keys} dimension keys have more than one row (up to {max_rows_per_key} rows per key): "
                         "a lookup join returns the first one; pass duplicates='first' to accept that")
        self.n_duplicate_keys = n_duplicate_keys
        self.max_rows_per_key = max_rows_per_key


class JoinOverflow(Exception):
    """A fan-out join (duplicates="all") whose output has more rows than `max_rows` allows."""

    def __init__(self, needed: int, max_rows: int):
        super().__init__(f"the join has {needed} output rows, more than max_rows={max_rows}: raise max_rows, or size the "
                         "output with join_count first")
        self.needed = needed
        self.max_rows = max_rows


def check_join(plan, key_map, how: str, duplicates: str) -> int:
    """The join type (`native.JOIN_INNER` / `JOIN_LEFT`) of a join of `plan`'s rows against `key_map`, after every
    refusal that needs no device: an unknown `how` or `duplicates`, a closed map, a map built for another reader's
    plan, and -- with duplicates="error" -- `DuplicateKeys` when the dimension has a key on more than one row.
    duplicates="all" is the fan-out join: one output row per matching dimension row."""
    if how not in ("inner", "left"):
        raise ValueError(f"join: how={how!r} is neither 'inner' nor 'left' (a lookup join has no right or full form)")
    if duplicates not in ("error", "first", "all"):
        raise ValueError(f"join: duplicates={duplicates!r} is neither 'error' nor 'first' nor 'all'")
    if duplicates == "all" and not hasattr(key_map, "index_rows"):
        raise ValueError("join: duplicates='all' takes a key map that can carry row lists (KeyMap.index_rows); for this "
                         "map it is neither 'error' nor 'first'")
    if key_map.closed:
        raise ValueError("the key map is closed")
    if key_map.plan is not plan:
        raise N.CbxError(N.CBX_E_ARGUMENT, "join: the key map was built for another reader's plan")
    if duplicates == "error" and key_map.n_duplicate_keys > 0:
        raise DuplicateKeys(key_map.n_duplicate_keys, key_map.max_rows_per_key)
    return N.JOIN_INNER if how == "inner" else N.JOIN_LEFT


class _DeviceInt64:
    """n int64 values at a device address, for torch.as_tensor (the CUDA array interface)."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2}


def _device_view(torch, ptr: int, n: int):
    """A copy of n int64 values at device address `ptr` as a tensor of its own."""
    if n <= 0:
        return torch.empty(0, dtype=torch.int64, device="cuda")
    return torch.as_tensor(_DeviceInt64(ptr, n), device="cuda").clone()


class _KeySetView(KeySet):
    """The member set of a key map: owned by the map, so closing the view frees nothing."""

    def close(self) -> None:
        self.handle = None


class KeyMap:
    """A device key map (`cbx_key_map_create_from_records`): the key set of `KeySet.from_records` whose members also
    carry the ordinal of the first source (dimension) row with that key and the number of such rows -- what
    `reader.join` probes.  Owns the library handle: `close()` (or the context manager) frees the device memory,
    `key_set` included.

    The map keeps a reference to the source reader, the source's device bytes and the record source its ordinals
    index (`source`: n_rec / sel / rec_off / rec_len / stride), so `JoinResult.dimension()` can decode the matching
    rows: THE SOURCE BYTES STAY RESIDENT ON THE DEVICE AS LONG AS THE MAP.  When the source filter held key sets of
    its own, the keyed filter ran first and the ordinals index that intermediate selection (which the map keeps too),
    not the file's records."""

    def __init__(self):
        raise TypeError("use KeyMap.from_records (reader.key_map_of / key_map_of_device)")

    @classmethod
    def from_records(cls, probe_plan, probe_handle, names: Sequence[str], source_plan, source_handle,
                     source_names: Sequence[str], d_data_ptr: int, n_bytes: int, n_rec: int, *, sel_struct=None,
                     rec_off_ptr=None, rec_len_ptr=None, stride: int = 0, start_offset: int = 0, filter_table=None,
                     max_values: int = 65536, max_workgroups: int = 0, stream=None) -> "KeyMap":
        """The arguments, refusals and counts of `KeySet.from_records`."""
        ptable, stable = compile_key_pairs(probe_plan, names, source_plan, source_names)
        info = N.CbxKeymapInfo()
        h = ctypes.c_void_p()
        rc = N.load().cbx_key_map_create_from_records(
            probe_handle, ctypes.byref(ptable), source_handle, ctypes.byref(stable), d_data_ptr, n_bytes,
            ctypes.byref(sel_struct) if sel_struct is not None else None, rec_off_ptr, rec_len_ptr, n_rec, stride,
            start_offset, ctypes.byref(filter_table) if filter_table is not None else None, int(max_values),
            max_workgroups, ctypes.c_void_p(stream.cuda_stream if stream is not None else 0), ctypes.byref(h),
            ctypes.byref(info))
        if rc == N.CBX_E_CAPACITY and info.overflow:
            raise A.GroupOverflow(int(max_values))
        N.check(rc)
        self = cls.__new__(cls)
        self.plan = probe_plan
        self.names = list(names)
        self.source_names = list(source_names)
        self.source_info = info
        self.dropped = info.n_dropped
        self.has_null = info.n_null_rows > 0
        self.n_values = info.n_source_keys - info.n_dropped
        self.n_duplicate_keys = info.n_duplicate_keys
        self.max_rows_per_key = info.max_rows_per_key
        self.handle = h
        self.source_reader = None   # set by the reader: what dimension() decodes with
        self.source_data = None
        self.source_bytes = 0
        self.source = None
        # what index_rows presents again: the source's key table, its filter table, its handle and the call's bounds
        self._source_table, self._source_handle = stable, source_handle
        self._source_filter, self._start_offset = filter_table, start_offset
        self._n_rec, self._n_bytes, self._data_ptr = n_rec, n_bytes, d_data_ptr
        self._sel_struct, self._rec_off_ptr, self._rec_len_ptr, self._stride = sel_struct, rec_off_ptr, rec_len_ptr, stride
        ks = _KeySetView.__new__(_KeySetView)
        ks.plan, ks.names = probe_plan, list(names)
        ks.dropped, ks.has_null, ks.n_values = self.dropped, self.has_null, self.n_values
        ks.source_info = info
        ks.handle = ctypes.c_void_p(N.load().cbx_key_map_set(h))
        self.key_set = ks
        return self

    @property
    def closed(self) -> bool:
        return self.handle is None

    def rows_info(self) -> N.CbxKeymapRowsInfo:
        """has_rows, n_indexed_rows, the members each sort path took (n_short / n_lds / n_global), the two boundaries
        (short_max / lds_max) and index_ms (profiling on) of the row lists (`cbx_key_map_rows_info`)."""
        if self.closed:
            raise ValueError("the key map is closed")
        out = N.CbxKeymapRowsInfo()
        N.check(N.load().cbx_key_map_rows_info(self.handle, ctypes.byref(out)))
        return out

    @property
    def has_rows(self) -> bool:
        """Whether the map carries per-key row lists (`index_rows`)."""
        return not self.closed and bool(self.rows_info().has_rows)

    def index_rows(self, max_workgroups: int = 0, stream=None) -> N.CbxKeymapRowsInfo:
        """`cbx_key_map_index_rows`: per member the ascending list of ALL its source rows, which a fan-out join
        (duplicates="all") walks.  Presents the retained source again (the device bytes the map references must be
        unchanged); idempotent: a second call launches nothing.  8 bytes per kept source row plus 8 per value, freed
        with the map."""
        if self.closed:
            raise ValueError("the key map is closed")
        info = N.CbxKeymapRowsInfo()
        N.check(N.load().cbx_key_map_index_rows(
            self.handle, self._source_handle, ctypes.byref(self._source_table), self._data_ptr, self._n_bytes,
            ctypes.byref(self._sel_struct) if self._sel_struct is not None else None, self._rec_off_ptr, self._rec_len_ptr,
            self._n_rec, self._stride, self._start_offset,
            ctypes.byref(self._source_filter) if self._source_filter is not None else None, max_workgroups,
            ctypes.c_void_p(stream.cuda_stream if stream is not None else 0), ctypes.byref(info)))
        return info

    def row_lists(self):
        """(row_start, rows): int64 device tensors over the map's memory (valid until close) -- rows[row_start[v] :
        row_start[v + 1]] are member v's source ordinals, ascending.  (None, None) before `index_rows` and for an
        empty map."""
        if self.closed:
            raise ValueError("the key map is closed")
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        N.check(N.load().cbx_key_map_rows(self.handle, ctypes.byref(a), ctypes.byref(b)))
        if not a.value:
            return None, None
        import torch
        n = self.rows_info().n_indexed_rows
        return _device_view(torch, a.value, self.n_values + 1), _device_view(torch, b.value, n)

    def close(self) -> None:
        if self.handle is not None:
            self.key_set.close()
            N.load().cbx_key_map_destroy(self.handle)
            self.handle = None
            self.source_reader = self.source_data = self.source = None
            self._sel_struct = self._source_filter = None

    def __enter__(self) -> "KeyMap":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (interpreter shutdown)
            pass

    def __repr__(self) -> str:
        return (f"KeyMap({self.source_names} -> {self.names}, n_values={self.n_values}, "
                f"n_duplicate_keys={self.n_duplicate_keys}, closed={self.closed})")
