"""Row filters pushed down to the GPU: Spark's `sources.Filter` classes and their compilation into the
library's predicate table (`cbx_filter`, include/cobrix_hip.h).

A relation that implements PrunedFilteredScan receives `buildScan(requiredColumns, filters)` -- the filters
AND-ed -- and reports through `unhandledFilters` which of them Spark must still evaluate itself.
`compile_filters` is that split: every filter it can express exactly in the table is compiled, every other
one is returned unhandled with the reason, so nothing is dropped silently.

Semantics (cbx_filter.h evaluates them on the record bytes): SQL three-valued logic, a row is kept only when
the whole filter is true; numerics compare as the column's output value (int / long / the unscaled decimal at
the column's scale), strings as the decoded UTF-8 bytes in unsigned byte order (UTF8String.compareTo);
StringStartsWith / StringEndsWith / StringContains byte-wise over those bytes.  EqualNullSafe, AlwaysTrue and
AlwaysFalse need no op of their own: they compile onto IS_NULL / EQ / NE and fold in `to_cnf`.
"""
from __future__ import annotations

import decimal
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple

from . import copybook as cbk
from . import native as N


class Filter:
    """org.apache.spark.sql.sources.Filter."""


@dataclass(frozen=True)
class EqualTo(Filter):
    attribute: str
    value: Any


@dataclass(frozen=True)
class GreaterThan(Filter):
    attribute: str
    value: Any


@dataclass(frozen=True)
class GreaterThanOrEqual(Filter):
    attribute: str
    value: Any


@dataclass(frozen=True)
class LessThan(Filter):
    attribute: str
    value: Any


@dataclass(frozen=True)
class LessThanOrEqual(Filter):
    attribute: str
    value: Any


@dataclass(frozen=True)
class In(Filter):
    attribute: str
    values: Tuple[Any, ...]

    def __init__(self, attribute: str, values: Sequence[Any]):
        object.__setattr__(self, "attribute", attribute)
        object.__setattr__(self, "values", tuple(values))


@dataclass(frozen=True)
class IsNull(Filter):
    attribute: str


@dataclass(frozen=True)
class IsNotNull(Filter):
    attribute: str


@dataclass(frozen=True)
class StringStartsWith(Filter):
    attribute: str
    value: str


@dataclass(frozen=True)
class StringEndsWith(Filter):
    attribute: str
    value: str


@dataclass(frozen=True)
class StringContains(Filter):
    attribute: str
    value: str


@dataclass(frozen=True)
class EqualNullSafe(Filter):
    """a <=> v: never unknown (null <=> null is true, null <=> v is false)."""
    attribute: str
    value: Any


@dataclass(frozen=True)
class AlwaysTrue(Filter):
    pass


@dataclass(frozen=True)
class AlwaysFalse(Filter):
    pass


@dataclass(frozen=True)
class And(Filter):
    left: Filter
    right: Filter


@dataclass(frozen=True)
class Or(Filter):
    left: Filter
    right: Filter


@dataclass(frozen=True)
class Not(Filter):
    child: Filter


@dataclass(frozen=True, eq=False)
class InSet(Filter):
    """(k1, .., kK) IN key_set: a `cobrix_amd.keyset.KeySet` built on the reader (`reader.key_set(names, values)`).
    A row with a null key column is not kept."""
    key_set: Any


@dataclass(frozen=True, eq=False)
class NotInSet(Filter):
    """k NOT IN key_set (single-column sets).  A row with a null key is not kept."""
    key_set: Any


class Unhandled(Exception):
    """The filter cannot be evaluated exactly by the GPU stage (the reason is the message)."""


class UnhandledFilters(list):
    """The filters left to the caller (PrunedFilteredScan.unhandledFilters), `reasons[i]` says why."""

    def __init__(self):
        super().__init__()
        self.reasons: List[str] = []

    def add(self, f: Filter, reason: str) -> None:
        self.append(f)
        self.reasons.append(reason)


_LEAF_OP = {EqualTo: N.OP_EQ, GreaterThan: N.OP_GT, GreaterThanOrEqual: N.OP_GE, LessThan: N.OP_LT,
            LessThanOrEqual: N.OP_LE, In: N.OP_IN, IsNull: N.OP_IS_NULL, IsNotNull: N.OP_IS_NOT_NULL,
            StringStartsWith: N.OP_STARTS_WITH, StringEndsWith: N.OP_ENDS_WITH, StringContains: N.OP_CONTAINS}
_STRING_ONLY_OPS = (N.OP_STARTS_WITH, N.OP_ENDS_WITH, N.OP_CONTAINS)
# NOT over a leaf under three-valued logic: NOT(unknown) is unknown, and the negated op is unknown on null too
_NEGATED = {N.OP_EQ: N.OP_NE, N.OP_NE: N.OP_EQ, N.OP_LT: N.OP_GE, N.OP_GE: N.OP_LT, N.OP_GT: N.OP_LE,
            N.OP_LE: N.OP_GT, N.OP_IN: N.OP_NOT_IN, N.OP_NOT_IN: N.OP_IN, N.OP_IS_NULL: N.OP_IS_NOT_NULL,
            N.OP_IS_NOT_NULL: N.OP_IS_NULL, N.OP_STARTS_WITH: N.OP_NOT_STARTS_WITH,
            N.OP_NOT_STARTS_WITH: N.OP_STARTS_WITH, N.OP_ENDS_WITH: N.OP_NOT_ENDS_WITH,
            N.OP_NOT_ENDS_WITH: N.OP_ENDS_WITH, N.OP_CONTAINS: N.OP_NOT_CONTAINS, N.OP_NOT_CONTAINS: N.OP_CONTAINS}
_STRING_KINDS = (N.K_STRING, N.K_STRING_ASCII)
_NUMERIC_KINDS = (N.K_BCD, N.K_BINARY, N.K_ZONED, N.K_ASCII_NUM)


@dataclass(frozen=True)
class Leaf:
    """One term of the table: plan field index, cbx_filter_op, converted literals (int / bytes)."""
    field: int
    op: int
    literals: Tuple[Any, ...]


def _literal(f: N.CbxField, is_str: bool, v: Any, name: str):
    if is_str:
        if not isinstance(v, str):
            raise Unhandled(f"{name}: a string column compares with str literals, not {type(v).__name__}")
        return v.encode("utf-8")
    if isinstance(v, bool) or not isinstance(v, (int, decimal.Decimal)):
        raise Unhandled(f"{name}: literal {v!r} is not an int or Decimal (not exactly representable)")
    d = decimal.Decimal(v)
    if not d.is_finite():
        raise Unhandled(f"{name}: literal {v!r} is not finite")
    dec_col = f.out_type in (N.O_DEC64, N.O_DEC128)
    scale = f.out_scale if dec_col else 0
    with decimal.localcontext() as ctx:
        ctx.prec = 200
        u = d.scaleb(scale)
        if u != u.to_integral_value():
            raise Unhandled(f"{name}: literal {v} is not representable at scale {scale}")
        u = int(u)
    if dec_col:
        if abs(u) >= 10 ** f.out_precision:
            raise Unhandled(f"{name}: literal {v} is out of range of decimal({f.out_precision}, {f.out_scale})")
    else:
        bits = 31 if f.out_type == N.O_I32 else 63
        if not -(1 << bits) <= u < (1 << bits):
            raise Unhandled(f"{name}: literal {v} is out of range of the column's {bits + 1}-bit integer")
    return u


def _leaf(plan, flt: Filter) -> Leaf:
    op = _LEAF_OP[type(flt)]
    name = flt.attribute
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
    null_op = op in (N.OP_IS_NULL, N.OP_IS_NOT_NULL)
    if f.kind in (N.K_FLOAT, N.K_DOUBLE):
        if not null_op:
            raise Unhandled(f"{name}: comparison on a COMP-1 / COMP-2 field")
    elif f.kind not in _STRING_KINDS + _NUMERIC_KINDS:
        raise Unhandled(f"{name}: UTF-16, HEX and RAW fields are not filtered on the GPU")
    is_str = f.kind in _STRING_KINDS
    if op in _STRING_ONLY_OPS and not is_str:
        raise Unhandled(f"{name}: {type(flt).__name__} on a numeric column")
    if null_op:
        lits: Tuple[Any, ...] = ()
    elif op == N.OP_IN:
        if any(v is None for v in flt.values):
            raise Unhandled(f"{name}: In with a null literal")
        lits = tuple(_literal(f, is_str, v, name) for v in flt.values)
    else:
        if flt.value is None:
            raise Unhandled(f"{name}: comparison with a null literal")
        lits = (_literal(f, is_str, flt.value, name),)
    return Leaf(fi, op, lits)


_MAX_CLAUSE_TERMS = 4 * N.CBX_FILTER_MAX_TERMS   # conversion stops early: the table could never hold it


def to_cnf(plan, flt: Filter, negate: bool = False) -> List[List[Leaf]]:
    """The filter as AND-ed clauses of OR-ed leaves: NOT pushed to the leaves (De Morgan, ops flipped), OR
    distributed over AND.  Constants fold here: true is no clause, false is one empty clause, which the AND
    concatenation and the OR distribution below carry as they carry any other.  Raises Unhandled."""
    if isinstance(flt, Not):
        return to_cnf(plan, flt.child, not negate)
    if isinstance(flt, (AlwaysTrue, AlwaysFalse)):
        return [] if isinstance(flt, AlwaysTrue) != negate else [[]]
    if isinstance(flt, EqualNullSafe):
        # never unknown: NOT (a <=> v) is true on a null a, where NE is unknown
        if flt.value is None:
            return to_cnf(plan, IsNull(flt.attribute), negate)
        eq = _leaf(plan, EqualTo(flt.attribute, flt.value))
        if not negate:
            return [[eq]]
        return [[_leaf(plan, IsNull(flt.attribute)), Leaf(eq.field, N.OP_NE, eq.literals)]]
    if isinstance(flt, (And, Or)):
        a, b = to_cnf(plan, flt.left, negate), to_cnf(plan, flt.right, negate)
        if isinstance(flt, And) != negate:   # a conjunction (And, or a negated Or)
            return a + b
        out = [x + [t for t in y if t not in x] for x in a for y in b]
        if sum(len(c) for c in out) > _MAX_CLAUSE_TERMS:
            raise Unhandled("conjunctive normal form exceeds the table limits")
        return out
    if type(flt) not in _LEAF_OP:
        raise Unhandled(f"{type(flt).__name__} is not a pushed-down filter")
    leaf = _leaf(plan, flt)
    return [[Leaf(leaf.field, _NEGATED[leaf.op], leaf.literals) if negate else leaf]]


def _false_leaf(plan) -> Leaf:
    """A term no row satisfies, nulls included: IN over no literal, on the plan's first field the stage filters."""
    if plan.walk is None:
        for i, f in enumerate(plan.fields):
            if f.n_dims == 0 and f.kind in _STRING_KINDS + _NUMERIC_KINDS:
                return Leaf(i, N.OP_IN, ())
    raise Unhandled("a constantly false filter needs a field the GPU stage filters, and the plan has none")


def _append(table: N.CbxFilter, clauses: List[List[Leaf]], group: int) -> bool:
    """Append the clauses to the table as groups group, group + 1, ..; False (table untouched) when they do not fit."""
    nt, nl, nb = table.n_terms, table.n_literals, table.pool_bytes
    terms = sum(len(c) for c in clauses)
    lits = sum(len(t.literals) for c in clauses for t in c)
    pool = sum(len(v) for c in clauses for t in c for v in t.literals if isinstance(v, bytes))
    if nt + terms > N.CBX_FILTER_MAX_TERMS or nl + lits > N.CBX_FILTER_MAX_LITERALS or nb + pool > N.CBX_FILTER_POOL_BYTES:
        return False
    for g, clause in enumerate(clauses):
        for t in clause:
            tt = table.terms[nt]
            tt.field, tt.op, tt.group, tt.lit_begin, tt.lit_count = t.field, t.op, group + g, nl, len(t.literals)
            nt += 1
            for v in t.literals:
                lt = table.literals[nl]
                if isinstance(v, bytes):
                    lt.str_off, lt.str_len = nb, len(v)
                    for j, b in enumerate(v):
                        table.pool[nb + j] = b
                    nb += len(v)
                else:
                    lt.lo = v & 0xFFFFFFFFFFFFFFFF          # two's complement: sign-extended to 128 bits
                    lt.hi = (v >> 64) & 0xFFFFFFFFFFFFFFFF
                nl += 1
    table.n_terms, table.n_literals, table.pool_bytes = nt, nl, nb
    return True


def compile_filters(plan, filters: Optional[Sequence[Filter]]) -> Tuple[Optional[N.CbxFilter], UnhandledFilters]:
    """(table or None, unhandled): the AND of `filters` as far as the GPU stage evaluates it exactly.  A filter is
    compiled whole or returned unhandled; None when no filter was compiled (a constantly true filter is handled
    and adds nothing; a constantly false one is one IN term with no literal)."""
    table = N.CbxFilter()
    unhandled = UnhandledFilters()
    group = 0
    for flt in filters or ():
        try:
            clauses = to_cnf(plan, flt)
            if any(not c for c in clauses):   # an empty clause: the filter is constantly false
                clauses = [[_false_leaf(plan)]]
        except Unhandled as e:
            unhandled.add(flt, str(e))
            continue
        if not _append(table, clauses, group):
            unhandled.add(flt, "the filter does not fit the table limits "
                               f"({N.CBX_FILTER_MAX_TERMS} terms, {N.CBX_FILTER_MAX_LITERALS} literals, "
                               f"{N.CBX_FILTER_POOL_BYTES} literal bytes)")
            continue
        group += len(clauses)
    return (table if group > 0 else None), unhandled


MAX_KEY_SETS = N.CBX_KEYSET_MAX_SETS


def _has_set(flt: Filter) -> bool:
    if isinstance(flt, (InSet, NotInSet)):
        return True
    if isinstance(flt, (And, Or)):
        return _has_set(flt.left) or _has_set(flt.right)
    return isinstance(flt, Not) and _has_set(flt.child)


def _conjuncts(flt: Filter) -> List[Filter]:
    """A top-level And that holds a set filter, as its AND-ed parts (others stay whole)."""
    if isinstance(flt, And) and _has_set(flt):
        return _conjuncts(flt.left) + _conjuncts(flt.right)
    return [flt]


def compile_filters_with_sets(plan, filters: Optional[Sequence[Filter]]):
    """(table or None, sets, negate, unhandled): `compile_filters` plus the key-set filters of the conjunction, for
    cbx_filter_records_keyed.  `sets` are the KeySet objects to probe, negate[i] != 0 for NOT IN.  Not(InSet) at
    top level is NotInSet.  Returned unhandled, with the reason: a set filter under Or (or under a Not that is
    not directly over it), a set past the stage's four, a negated set of more than one column, NotInSet over values
    that held a null (the whole predicate is unknown), a set built on another reader's plan."""
    sets: List[Any] = []
    negate: List[int] = []
    plain: List[Filter] = []
    late = UnhandledFilters()
    for top in filters or ():
        for flt in _conjuncts(top):
            f = flt
            while isinstance(f, Not) and isinstance(f.child, Not):
                f = f.child.child
            if isinstance(f, Not) and isinstance(f.child, (InSet, NotInSet)):
                f = NotInSet(f.child.key_set) if isinstance(f.child, InSet) else InSet(f.child.key_set)
            if not isinstance(f, (InSet, NotInSet)):
                if _has_set(f):
                    late.add(flt, "a key-set filter under Or or under a negated group is not pushed down")
                else:
                    plain.append(flt)
                continue
            ks = f.key_set
            if ks.closed:
                raise ValueError("the key set is closed")
            neg = isinstance(f, NotInSet)
            if ks.plan is not plan:
                late.add(flt, "the key set was built on another reader's plan")
            elif neg and len(ks.names) != 1:
                late.add(flt, "only a single-column key set may be negated")
            elif neg and ks.has_null:
                late.add(flt, "NotInSet over values that hold a null: the predicate is unknown for every row")
            elif len(sets) >= MAX_KEY_SETS:
                late.add(flt, f"more than {MAX_KEY_SETS} key sets in one filter call")
            else:
                sets.append(ks)
                negate.append(1 if neg else 0)
    table, unhandled = compile_filters(plan, plain)
    for f, r in zip(late, late.reasons):
        unhandled.add(f, r)
    return table, sets, negate, unhandled
