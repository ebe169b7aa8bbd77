"""Top-N (ORDER BY .. LIMIT n) and LIMIT pushed down to the GPU: Spark's sort orders and their compilation into
the library's sort table (`cbx_sort_order`, include/cobrix_hip.h).

A data source that implements SupportsPushDownTopN receives `pushTopN(orders, limit)` (SupportsPushDownLimit:
`pushLimit(limit)`, the same call with no order) and answers whether it applies them.  `compile_order` is that
answer: all or nothing -- one key the GPU stage cannot order exactly makes the whole request `Unhandled`, with
the reason.  The pushdown is PARTIAL (`isPartiallyPushed() == true`): every batch, index entry or shard returns
its own first n rows, in source order, and Spark keeps its Sort + Limit above the scan.

Semantics (cbx_topn.h selects them from the record bytes): a key's value is the one the row filter compares --
null where the decode makes it null, else the column's value; strings order by their UTF-8 bytes, unsigned
(UTF8String.compareTo); rows equal on every key are taken by source position.  `order_rows` sorts decoded
rows the same way on the host, for a caller that wants them ordered.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

from . import copybook as cbk
from . import native as N
from .filter import Unhandled

__all__ = ["SortOrder", "compile_order", "order_rows", "compare_values", "Unhandled"]

_STRING_KINDS = (N.K_STRING, N.K_STRING_ASCII)
_NUMERIC_KINDS = (N.K_BCD, N.K_BINARY, N.K_ZONED, N.K_ASCII_NUM)
TOPN_MAX_STRING_KEY_BYTES = 32


@dataclass(frozen=True)
class SortOrder:
    """org.apache.spark.sql.connector.expressions.SortOrder over a plain column reference.
    nulls_first None is Spark's default: ASC gives NULLS FIRST, DESC gives NULLS LAST."""
    column: str
    descending: bool = False
    nulls_first: Optional[bool] = None

    @property
    def nulls_first_resolved(self) -> bool:
        return (not self.descending) if self.nulls_first is None else bool(self.nulls_first)

    @property
    def flags(self) -> int:
        return (N.SORT_DESC if self.descending else 0) | (0 if self.nulls_first_resolved else N.SORT_NULLS_LAST)


def compile_order(plan, orders: Sequence[SortOrder]) -> N.CbxSortOrder:
    """The sort table of ORDER BY `orders` ([]: the plain LIMIT); raises Unhandled with the reason when any key
    cannot be ordered on the GPU -- all or nothing, as compile_aggregates."""
    orders = list(orders)
    if len(orders) > N.CBX_TOPN_MAX_KEYS:
        raise Unhandled(f"ORDER BY takes up to {N.CBX_TOPN_MAX_KEYS} sort keys, not {len(orders)}")
    table = N.CbxSortOrder()
    for so in orders:
        if not isinstance(so, SortOrder) or not isinstance(so.column, str):
            raise Unhandled(f"{so!r}: a sort key must be a SortOrder over a plain column reference")
        name = so.column
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
            raise Unhandled(f"{name}: COMP-1 / COMP-2 key (NaN ordering is not modelled)")
        is_str = f.kind in _STRING_KINDS
        if is_str and f.size > TOPN_MAX_STRING_KEY_BYTES:
            raise Unhandled(f"{name}: string key longer than {TOPN_MAX_STRING_KEY_BYTES} bytes")
        if not is_str and f.kind not in _NUMERIC_KINDS:
            raise Unhandled(f"{name}: UTF-16, HEX and RAW fields are not ordered on the GPU")
        if any(table.keys[k].field == fi for k in range(table.n_keys)):
            raise Unhandled(f"{name}: sort key repeated")
        table.keys[table.n_keys].field = fi
        table.keys[table.n_keys].flags = so.flags
        table.n_keys += 1
    return table


def compare_values(a: Any, b: Any, so: SortOrder) -> int:
    """-1 / 0 / 1: a before / with / after b under one sort key (None: null; str: by UTF-8 bytes)."""
    if a is None or b is None:
        if a is None and b is None:
            return 0
        return -1 if (a is None) == so.nulls_first_resolved else 1
    if isinstance(a, str):
        a, b = a.encode("utf-8"), b.encode("utf-8")
    c = (a > b) - (a < b)
    return -c if so.descending else c


def _row_value(cb: cbk.Copybook, row: dict, name: str, cache: dict):
    path = cache.get(name)
    if path is None:
        st = cb.get_field_by_name(name)
        p = []
        while st.parent is not None and st.parent.parent is not None:   # up to, not including, the 01 group
            p.append(st.name)
            st = st.parent
        path = cache[name] = tuple(reversed(p))
    v = row
    for k in path:
        if v is None:
            return None
        v = v[k]
    return v


def order_rows(cb: cbk.Copybook, rows: Sequence[dict], orders: Sequence[SortOrder]) -> List[dict]:
    """`rows` (decoded with schema_policy collapse_root, e.g. `top_n(..).to_rows()`) sorted by `orders`; rows
    equal on every key keep their order (a stable sort: the source order of a Top-N result)."""
    orders = list(orders)
    cache: dict = {}
    keyed = [([_row_value(cb, r, so.column, cache) for so in orders], r) for r in rows]

    def cmp(x, y):
        for so, a, b in zip(orders, x[0], y[0]):
            c = compare_values(a, b, so)
            if c:
                return c
        return 0
    return [r for _, r in sorted(keyed, key=functools.cmp_to_key(cmp))]
