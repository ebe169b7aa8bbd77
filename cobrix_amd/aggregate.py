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
from typing import Any, List, Optional, Sequence, Tuple

from . import copybook as cbk
from . import native as N
from .filter import Unhandled

__all__ = ["AggregateFunc", "CountStar", "Count", "Min", "Max", "Sum", "Slot", "AggregateResult",
           "compile_aggregates", "Unhandled"]


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
