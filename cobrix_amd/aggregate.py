"""Aggregates pushed down to the GPU: Spark's aggregate function classes and their compilation into the
library's aggregate table (`cbx_aggregate`, include/cobrix_hip.h).

A data source that implements SupportsPushDownAggregates receives `pushAggregation(aggregation)` and answers
whether it computes the whole aggregation itself.  `compile_aggregates` is that answer: pushdown is all or
nothing -- one function the GPU stage cannot compute exactly makes the whole request `Unhandled`, with the
reason; nothing is evaluated in part or dropped silently.  Spark's `isDistinct` is left out: a distinct
aggregate is not pushed.

Semantics (cbx_aggregate.h computes them on the record bytes): the value of a field is the one the row filter
compares -- null where the decode makes it null, else the column's value (int / long / the unscaled decimal
at the column's scale); nulls are skipped.  Sums are exact (192-bit accumulators), so `AggregateResult.raw`
compares bit for bit with Python integers; `AggregateResult.values` maps them to Spark's result types.
"""
from __future__ import annotations

import decimal
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

from . import copybook as cbk
from . import native as N
from .filter import Unhandled

__all__ = ["AggregateFunc", "CountStar", "Count", "Min", "Max", "Sum", "Slot", "AggregateResult",
           "compile_aggregates", "Unhandled", "KeySlot", "GroupOverflow", "GroupedAggregateResult", "compile_group_by"]


class AggregateFunc:
    """org.apache.spark.sql.connector.expressions.aggregate.AggregateFunc."""


@dataclass(frozen=True)
class CountStar(AggregateFunc):
    pass


@dataclass(frozen=True)
class Count(AggregateFunc):
    column: str


@dataclass(frozen=True)
class Min(AggregateFunc):
    column: str


@dataclass(frozen=True)
class Max(AggregateFunc):
    column: str


@dataclass(frozen=True)
class Sum(AggregateFunc):
    column: str


_FUNC_BIT = {Count: N.AGG_COUNT, Min: N.AGG_MIN, Max: N.AGG_MAX, Sum: N.AGG_SUM}
_STRING_KINDS = (N.K_STRING, N.K_STRING_ASCII)
_NUMERIC_KINDS = (N.K_BCD, N.K_BINARY, N.K_ZONED, N.K_ASCII_NUM)
_MASK64 = (1 << 64) - 1


@dataclass(frozen=True)
class Slot:
    """One requested function: its cbx_aggregate_func bit (0: COUNT(*)), the term that holds it (-1: none) and
    the column's type as the plan's field gives it."""
    func: int
    term: int
    field: int
    out_type: int
    out_precision: int
    out_scale: int


def compile_aggregates(plan, aggregates: Sequence[AggregateFunc]) -> Tuple[N.CbxAggregate, List[Slot]]:
    """(table, slots) of the whole request, slots[i] for aggregates[i]; raises Unhandled with the reason when any
    function cannot be pushed.  Several functions of one column share a term."""
    table = N.CbxAggregate()
    slots: List[Slot] = []
    term_of_field: dict = {}
    for ag in aggregates:
        if isinstance(ag, CountStar):
            slots.append(Slot(0, -1, -1, N.O_I64, 0, 0))
            continue
        bit = _FUNC_BIT.get(type(ag))
        if bit is None:
            raise Unhandled(f"{type(ag).__name__} is not a pushed-down aggregate function")
        name = ag.column
        try:
            st = plan.copybook.get_field_by_name(name)
        except ValueError as e:
            raise Unhandled(str(e)) from None
        if not isinstance(st, cbk.Primitive) or id(st) not in plan.field_of_node:
            raise Unhandled(f"{name}: not a decoded primitive field")
        fi = plan.field_of_node[id(st)]
        f = plan.fields[fi]
        if plan.walk is not None:
            raise Unhandled(f"{name}: record-walk plan, fields lie at data-dependent offsets")
        if f.n_dims > 0:
            raise Unhandled(f"{name}: field inside an OCCURS")
        reduces = bit != N.AGG_COUNT
        if f.kind in (N.K_FLOAT, N.K_DOUBLE):
            if reduces:
                raise Unhandled(f"{name}: MIN, MAX or SUM on a COMP-1 / COMP-2 field")
        elif f.kind in _STRING_KINDS:
            if reduces:
                raise Unhandled(f"{name}: MIN, MAX or SUM on a string field")
        elif f.kind not in _NUMERIC_KINDS:
            raise Unhandled(f"{name}: UTF-16, HEX and RAW fields are not aggregated on the GPU")
        t = term_of_field.get(fi)
        if t is None:
            if table.n_terms >= N.CBX_AGG_MAX_TERMS:
                raise Unhandled(f"{name}: more than {N.CBX_AGG_MAX_TERMS} distinct columns")
            t = term_of_field[fi] = table.n_terms
            table.terms[t].field = fi
            table.n_terms += 1
        table.terms[t].funcs |= bit
        slots.append(Slot(bit, t, fi, f.out_type, f.out_precision, f.out_scale))
    return table, slots


def _signed(v: int, bits: int) -> int:
    return v - (1 << bits) if v >> (bits - 1) else v


def _merge_term(a: dict, b: dict) -> dict:
    """agg_merge (cbx_aggregate.h) over the raw values of one term."""
    if b["count"] == 0:
        return dict(a)
    if a["count"] == 0:
        return dict(b)
    pick = lambda fn, x, y: None if x is None else fn(x, y)   # noqa: E731
    return {"field": a["field"], "count": a["count"] + b["count"], "min": pick(min, a["min"], b["min"]),
            "max": pick(max, a["max"], b["max"]), "sum": pick(lambda x, y: x + y, a["sum"], b["sum"])}


class AggregateResult:
    """The result of one pushed aggregation.
    raw:    {"n_rows": COUNT(*), "terms": [{"field", "count", "min", "max", "sum"}]} -- per term of the table the
            number of non-null values and the exact Python ints (unscaled at the column's scale); min / max / sum
            are None when their function was not asked for or no value is non-null.
    values: one value per requested function, in Spark's result types."""

    def __init__(self, slots: Sequence[Slot], n_rows: int, terms: List[dict]):
        self.slots = list(slots)
        self.raw = {"n_rows": n_rows, "terms": terms}

    @classmethod
    def from_struct(cls, table: N.CbxAggregate, slots: Sequence[Slot], res: N.CbxAggregateResult) -> "AggregateResult":
        terms = []
        for t in range(table.n_terms):
            v, funcs = res.values[t], table.terms[t].funcs
            have = v.count > 0
            terms.append({
                "field": table.terms[t].field, "count": v.count,
                "min": _signed(v.min_hi << 64 | v.min_lo, 128) if have and funcs & N.AGG_MIN else None,
                "max": _signed(v.max_hi << 64 | v.max_lo, 128) if have and funcs & N.AGG_MAX else None,
                "sum": _signed(v.sum[2] << 128 | v.sum[1] << 64 | v.sum[0], 192) if have and funcs & N.AGG_SUM else None})
        return cls(slots, res.n_rows, terms)

    @property
    def n_rows(self) -> int:
        return self.raw["n_rows"]

    def merge(self, other: "AggregateResult") -> "AggregateResult":
        """The result over both sides' (disjoint) records: batches, sparse-index entries and multi-GPU shards
        combine on the host with it.  Associative; the same merge as agg_merge."""
        if self.slots != other.slots:
            raise ValueError("merge: the two results answer different aggregate requests")
        terms = [_merge_term(a, b) for a, b in zip(self.raw["terms"], other.raw["terms"])]
        return AggregateResult(self.slots, self.n_rows + other.n_rows, terms)

    @staticmethod
    def _spark(slot: Slot, term: Optional[dict], n_rows: int) -> Any:
        if slot.func == 0:
            return n_rows
        if slot.func == N.AGG_COUNT:
            return term["count"]
        raw = term[{N.AGG_MIN: "min", N.AGG_MAX: "max", N.AGG_SUM: "sum"}[slot.func]]
        if raw is None:
            return None
        is_dec = slot.out_type in (N.O_DEC64, N.O_DEC128)
        if slot.func == N.AGG_SUM:
            if not is_dec:   # Sum of int / long -> long, Java wrap-around (non-ANSI)
                return _signed(raw & _MASK64, 64)
            if abs(raw) >= 10 ** min(38, slot.out_precision + 10):   # decimal(min(38, p + 10), s) overflow -> null
                return None
        if not is_dec:
            return raw
        with decimal.localcontext() as ctx:
            ctx.prec = 80
            return decimal.Decimal(raw).scaleb(-slot.out_scale)

    @property
    def values(self) -> List[Any]:
        terms = self.raw["terms"]
        return [self._spark(s, terms[s.term] if s.term >= 0 else None, self.n_rows) for s in self.slots]

    def __repr__(self) -> str:
        return f"AggregateResult(n_rows={self.n_rows}, values={self.values})"


# ---------------------------------------------------------------------------------------------
# GROUP BY (cbx_aggregate_grouped)
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class KeySlot:
    """One GROUP BY column: its field and the column's type as the plan's field gives it."""
    field: int
    is_str: bool
    out_type: int
    out_precision: int
    out_scale: int


class GroupOverflow(RuntimeError):
    """The data holds more distinct keys than max_groups: nothing was returned; call again with a larger max_groups."""

    def __init__(self, max_groups: int):
        super().__init__(f"more than max_groups = {max_groups} distinct GROUP BY keys; raise max_groups")
        self.max_groups = max_groups


def compile_group_by(plan, columns: Sequence[str]) -> Tuple[N.CbxGroupBy, List[KeySlot]]:
    """(table, key slots) of GROUP BY `columns` (plain column references); raises Unhandled with the reason when
    any key cannot be grouped on the GPU -- all or nothing, as compile_aggregates."""
    columns = list(columns)
    if not 1 <= len(columns) <= N.CBX_GROUP_MAX_KEYS:
        raise Unhandled(f"GROUP BY takes 1 to {N.CBX_GROUP_MAX_KEYS} key columns, not {len(columns)}")
    table = N.CbxGroupBy()
    keys: List[KeySlot] = []
    for name in columns:
        if not isinstance(name, str):
            raise Unhandled(f"{name!r}: a GROUP BY key must be a plain column reference")
        try:
            st = plan.copybook.get_field_by_name(name)
        except ValueError as e:
            raise Unhandled(str(e)) from None
        if not isinstance(st, cbk.Primitive) or id(st) not in plan.field_of_node:
            raise Unhandled(f"{name}: not a decoded primitive field")
        fi = plan.field_of_node[id(st)]
        f = plan.fields[fi]
        if plan.walk is not None:
            raise Unhandled(f"{name}: record-walk plan, fields lie at data-dependent offsets")
        if f.n_dims > 0:
            raise Unhandled(f"{name}: field inside an OCCURS")
        if f.kind in (N.K_FLOAT, N.K_DOUBLE):
            raise Unhandled(f"{name}: COMP-1 / COMP-2 key")
        is_str = f.kind in _STRING_KINDS
        if is_str and f.size > N.GROUP_MAX_STRING_KEY_BYTES:
            raise Unhandled(f"{name}: string key longer than {N.GROUP_MAX_STRING_KEY_BYTES} bytes")
        if not is_str and f.kind not in _NUMERIC_KINDS:
            raise Unhandled(f"{name}: UTF-16, HEX and RAW fields are not grouped on the GPU")
        if any(k.field == fi for k in keys):
            raise Unhandled(f"{name}: key column repeated")
        table.fields[table.n_keys] = fi
        table.n_keys += 1
        keys.append(KeySlot(fi, is_str, f.out_type, f.out_precision, f.out_scale))
    return table, keys


def check_grouped_functions(slots: Sequence[Slot]) -> None:
    """MIN / MAX of a DEC128 column is not computed per group (no 128-bit atomic): Unhandled."""
    for s in slots:
        if s.out_type == N.O_DEC128 and s.func in (N.AGG_MIN, N.AGG_MAX):
            raise Unhandled("MIN or MAX of a DEC128 column under GROUP BY")


def _key_value(k: KeySlot, cell: N.CbxGroupKey, raw: bytes) -> Any:
    if cell.is_null:
        return None
    if k.is_str:
        return raw[:cell.str_len].decode("utf-8")
    v = _signed(cell.hi << 64 | cell.lo, 128)
    if k.out_type in (N.O_DEC64, N.O_DEC128):
        with decimal.localcontext() as ctx:
            ctx.prec = 80
            return decimal.Decimal(v).scaleb(-k.out_scale)
    return v


def _key_order(key: tuple) -> tuple:
    return tuple((0, 0) if v is None else (1, v) for v in key)


class GroupedAggregateResult:
    """The result of one pushed grouped aggregation.
    groups: {key tuple: AggregateResult}, a key value being Spark-typed: int, Decimal at the column's scale, str, or
            None (all nulls of a key column form one group; "" is a group of its own)."""

    def __init__(self, keys: Sequence[KeySlot], slots: Sequence[Slot], groups: Dict[tuple, AggregateResult]):
        self.keys = list(keys)
        self.slots = list(slots)
        self.groups = groups

    @classmethod
    def from_arrays(cls, table: N.CbxAggregate, slots: Sequence[Slot], keys: Sequence[KeySlot], strides: N.CbxGroupStrides,
                    n_groups: int, n_rows, values, cells, key_bytes) -> "GroupedAggregateResult":
        """From the output arrays of cbx_aggregate_grouped (ctypes arrays sized by max_groups)."""
        nt, nk = table.n_terms, len(keys)
        groups: Dict[tuple, AggregateResult] = {}
        raw = bytes(key_bytes) if key_bytes is not None else b""
        for g in range(n_groups):
            key = []
            for k, ks in enumerate(keys):
                at = g * strides.str_stride + strides.str_off[k]
                key.append(_key_value(ks, cells[g * nk + k], raw[at:at + 3 * N.GROUP_MAX_STRING_KEY_BYTES] if ks.is_str else b""))
            res = N.CbxAggregateResult()
            res.n_rows = n_rows[g]
            for t in range(nt):
                res.values[t] = values[g * nt + t]
            key = tuple(key)
            if key in groups:
                raise AssertionError(f"cbx_aggregate_grouped returned the key {key!r} twice")
            groups[key] = AggregateResult.from_struct(table, slots, res)
        return cls(keys, slots, groups)

    @property
    def n_rows(self) -> int:
        return sum(r.n_rows for r in self.groups.values())

    def merge(self, other: "GroupedAggregateResult") -> "GroupedAggregateResult":
        """The result over both sides' (disjoint) records: the union of the keys, AggregateResult.merge where both hold one."""
        if self.slots != other.slots or self.keys != other.keys:
            raise ValueError("merge: the two results answer different grouped requests")
        groups = dict(self.groups)
        for key, r in other.groups.items():
            groups[key] = groups[key].merge(r) if key in groups else r
        return GroupedAggregateResult(self.keys, self.slots, groups)

    def rows(self) -> List[tuple]:
        """(key values..., aggregate values...) per group, sorted by key, nulls first."""
        return [tuple(key) + tuple(self.groups[key].values) for key in sorted(self.groups, key=_key_order)]

    def __repr__(self) -> str:
        return f"GroupedAggregateResult({len(self.groups)} groups, n_rows={self.n_rows})"
