"""Suffix / substring filters, null-safe equality and constant filters, the parts that need no GPU: how
StringEndsWith, StringContains, EqualNullSafe, AlwaysTrue and AlwaysFalse compile into the predicate table,
the new header constants, and the per-record evaluator of cobrix_amd/csrc/cbx_filter.h run on the host
(tests/native/filter_host.cpp, unchanged) against a Python evaluator over the oracle's rows.

The contract (include/cobrix_hip.h): ENDS_WITH / CONTAINS compare the literal's bytes with the column's decoded
UTF-8 bytes as UTF8String.endsWith / contains do; a null value is unknown for an op and for its negation; an
empty literal is true for every non-null value.  `py_eval_s` states it with bytes.endswith and `in`;
test_gpu_filter_strings.py uses the same evaluator and the same literal families on the GPU.
"""
from __future__ import annotations

import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from cobrix_amd import filter as F
from cobrix_amd import native as N
from cobrix_amd.reader import ReaderParameters
from cobrix_amd.synth import SYN200_COPYBOOK
from test_filter import (FUZZ_N, LADDER_COPYBOOK, WIDE_COPYBOOK, _fi, _plan, _table, ascii_records,  # noqa: F401
                         fuzz_records, host_keep, host_keep_framed, host_shim, ladder_file, ladder_params,
                         leaf_names, narrow_file, narrow_params, py_eval, reader_plan, row_value)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cobrix_hip.h")

POSITIVE = {N.OP_ENDS_WITH: F.StringEndsWith, N.OP_CONTAINS: F.StringContains}
NEGATIVE = {N.OP_NOT_ENDS_WITH: F.StringEndsWith, N.OP_NOT_CONTAINS: F.StringContains}
STRING_OPS = (N.OP_ENDS_WITH, N.OP_NOT_ENDS_WITH, N.OP_CONTAINS, N.OP_NOT_CONTAINS)


# ---------------------------------------------------------------------------------------------
# The contract over decoded rows (three-valued: True / False / None = unknown)
# ---------------------------------------------------------------------------------------------
def _bytes(v):
    return v.encode("utf-8") if isinstance(v, str) else v


def py_eval_s(cb, row, f):
    """test_filter.py_eval with the new classes.  A literal may be given as bytes (the raw C table takes byte
    strings that are no valid UTF-8: a literal cut inside a character)."""
    if isinstance(f, F.And):
        a, b = py_eval_s(cb, row, f.left), py_eval_s(cb, row, f.right)
        return False if a is False or b is False else (None if a is None or b is None else True)
    if isinstance(f, F.Or):
        a, b = py_eval_s(cb, row, f.left), py_eval_s(cb, row, f.right)
        return True if a is True or b is True else (None if a is None or b is None else False)
    if isinstance(f, F.Not):
        a = py_eval_s(cb, row, f.child)
        return None if a is None else not a
    if isinstance(f, F.AlwaysTrue):
        return True
    if isinstance(f, F.AlwaysFalse):
        return False
    if isinstance(f, F.EqualNullSafe):   # never unknown
        v = row_value(cb, row, f.attribute)
        if v is None or f.value is None:
            return v is None and f.value is None
        return _bytes(v) == _bytes(f.value)
    if isinstance(f, (F.StringEndsWith, F.StringContains)):
        v = row_value(cb, row, f.attribute)
        if v is None:
            return None
        v, x = _bytes(v), _bytes(f.value)
        return v.endswith(x) if isinstance(f, F.StringEndsWith) else x in v
    return py_eval(cb, row, f)


def py_keep_s(cb, row, filters) -> bool:
    return all(py_eval_s(cb, row, f) is True for f in filters)


def expected_keep_s(cb, rows, filters) -> np.ndarray:
    return np.array([py_keep_s(cb, r, filters) for r in rows], dtype=bool)


# ---------------------------------------------------------------------------------------------
# compile_filters: the new classes
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syn_plan():
    return _plan(SYN200_COPYBOOK)


@pytest.fixture(scope="module")
def wide_plan():
    return _plan(WIDE_COPYBOOK)


def _groups(t):
    """[[(field, op, literals)] per group] of a compiled table."""
    out = {}
    for g, fld, op, lits in _table(t):
        out.setdefault(g, []).append((fld, op, lits))
    return [out[g] for g in sorted(out)]


def test_ends_with_and_contains_compile(syn_plan):
    name = _fi(syn_plan, "NAME")
    for cls, op, neg in ((F.StringEndsWith, N.OP_ENDS_WITH, N.OP_NOT_ENDS_WITH),
                         (F.StringContains, N.OP_CONTAINS, N.OP_NOT_CONTAINS)):
        t, un = F.compile_filters(syn_plan, [cls("NAME", "éB")])
        assert not un and _groups(t) == [[(name, op, [(0, 0, "éB".encode())])]]
        t, un = F.compile_filters(syn_plan, [F.Not(cls("NAME", "AB"))])
        assert not un and _groups(t) == [[(name, neg, [(0, 0, b"AB")])]]
        t, un = F.compile_filters(syn_plan, [F.Not(F.Not(cls("NAME", "")))])
        assert not un and _groups(t) == [[(name, op, [(0, 0, b"")])]]
        assert F._NEGATED[op] == neg and F._NEGATED[neg] == op
    assert (N.OP_ENDS_WITH, N.OP_NOT_ENDS_WITH, N.OP_CONTAINS, N.OP_NOT_CONTAINS) == (13, 14, 15, 16)
    # De Morgan over the new leaves
    f = F.Not(F.Or(F.StringContains("NAME", "X"), F.And(F.StringEndsWith("NAME", "Y"), F.EqualTo("BR-ID", 1))))
    t, un = F.compile_filters(syn_plan, [f])
    assert not un
    assert [[(op) for _, op, _ in g] for g in _groups(t)] == [[N.OP_NOT_CONTAINS], [N.OP_NOT_ENDS_WITH, N.OP_NE]]


def test_ends_with_and_contains_unhandled_cases(syn_plan, wide_plan):
    for cls in (F.StringEndsWith, F.StringContains):
        for f, word in ((cls("AMT-01", "1"), "numeric"), (cls("BR-ID", "1"), "numeric"), (cls("NAME", 5), "str literals"),
                        (cls("NAME", b"A"), "str literals"), (cls("NAME", None), "null literal"),
                        (cls("NO-SUCH", "A"), "not found")):
            t, un = F.compile_filters(syn_plan, [f, F.EqualTo("BR-ID", 4)])
            assert un == [f] and word in un.reasons[0], (f, un.reasons)
            assert t.n_terms == 1                     # the supported filter still compiles
            assert cls.__name__ in un.reasons[0] or word != "numeric"
            t, un = F.compile_filters(syn_plan, [F.Not(f)])
            assert t is None and len(un) == 1
        f = cls("ITEM-NO", "1")
        assert "OCCURS" in F.compile_filters(wide_plan, [f])[1].reasons[0]
        f = cls("RATE", "1")
        assert F.compile_filters(wide_plan, [f])[1] == [f]


def test_equal_null_safe_compiles(syn_plan, wide_plan):
    """EqualNullSafe(a, None) is IS_NULL / IS_NOT_NULL; EqualNullSafe(a, v) is EQ, and under Not the one clause
    IS_NULL(a) OR NE(a, v): `<=>` is never unknown, so its negation is true on a null."""
    for plan, col, v, lit in ((syn_plan, "NAME", "AB", (0, 0, b"AB")), (syn_plan, "AMT-01", 3, (300, 0, b""))):
        fi = _fi(plan, col)
        t, un = F.compile_filters(plan, [F.EqualNullSafe(col, v)])
        assert not un and _groups(t) == [[(fi, N.OP_EQ, [lit])]]
        t, un = F.compile_filters(plan, [F.Not(F.EqualNullSafe(col, v))])
        assert not un and _groups(t) == [[(fi, N.OP_IS_NULL, []), (fi, N.OP_NE, [lit])]]
        t, un = F.compile_filters(plan, [F.EqualNullSafe(col, None)])
        assert not un and _groups(t) == [[(fi, N.OP_IS_NULL, [])]]
        t, un = F.compile_filters(plan, [F.Not(F.EqualNullSafe(col, None))])
        assert not un and _groups(t) == [[(fi, N.OP_IS_NOT_NULL, [])]]
    rate = _fi(wide_plan, "RATE")   # COMP-1: only the None form
    t, un = F.compile_filters(wide_plan, [F.EqualNullSafe("RATE", None), F.Not(F.EqualNullSafe("RATE", None))])
    assert not un and _groups(t) == [[(rate, N.OP_IS_NULL, [])], [(rate, N.OP_IS_NOT_NULL, [])]]
    for f in (F.EqualNullSafe("RATE", 1), F.Not(F.EqualNullSafe("RATE", 1))):
        t, un = F.compile_filters(wide_plan, [f])
        assert t is None and un == [f] and "COMP-1" in un.reasons[0]
    # the literal is converted as EqualTo converts it
    for f in (F.EqualNullSafe("AMT-01", 1.5), F.EqualNullSafe("NAME", 5), F.Not(F.EqualNullSafe("AMT-01", "x"))):
        assert F.compile_filters(syn_plan, [f])[1] == [f]
    # inside a tree: NOT (a <=> v) AND b  ->  (IS_NULL(a) | NE(a, v)) (b)
    t, un = F.compile_filters(syn_plan, [F.Not(F.Or(F.EqualNullSafe("NAME", "A"), F.IsNull("BR-ID")))])
    assert not un and [[op for _, op, _ in g] for g in _groups(t)] == [[N.OP_IS_NULL, N.OP_NE], [N.OP_IS_NOT_NULL]]


def _first_filterable(plan):
    return next(i for i, f in enumerate(plan.fields)
                if f.n_dims == 0 and f.kind in (N.K_STRING, N.K_STRING_ASCII, N.K_BCD, N.K_BINARY, N.K_ZONED, N.K_ASCII_NUM))


def test_constants_fold(syn_plan, wide_plan):
    x, y = F.EqualTo("BR-ID", 1), F.StringContains("NAME", "A")
    one = lambda f: F.compile_filters(syn_plan, [f])   # noqa: E731
    gx = _groups(one(x)[0])
    false = [[(_first_filterable(syn_plan), N.OP_IN, [])]]
    # true: no clause
    for f in (F.AlwaysTrue(), F.Not(F.AlwaysFalse()), F.Or(F.AlwaysTrue(), x), F.Or(x, F.Not(F.AlwaysFalse())),
              F.And(F.AlwaysTrue(), F.AlwaysTrue()), F.Not(F.And(F.AlwaysFalse(), x))):
        t, un = one(f)
        assert t is None and not un, f            # handled, and adds no group
    t, un = F.compile_filters(syn_plan, [F.AlwaysTrue(), x, F.AlwaysTrue()])
    assert not un and _groups(t) == gx
    # x: the constant drops out
    for f in (F.Or(F.AlwaysFalse(), x), F.Or(x, F.AlwaysFalse()), F.And(F.AlwaysTrue(), x), F.And(x, F.Not(F.AlwaysFalse())),
              F.Not(F.Or(F.AlwaysFalse(), F.Not(x))), F.Or(F.Not(F.AlwaysTrue()), x)):
        t, un = one(f)
        assert not un and _groups(t) == gx, f
    t, un = one(F.Or(F.AlwaysFalse(), F.And(x, y)))
    assert not un and [[op for _, op, _ in g] for g in _groups(t)] == [[N.OP_EQ], [N.OP_CONTAINS]]
    # false: IN over no literal on the plan's first filterable field, one term whatever stood beside it
    for f in (F.AlwaysFalse(), F.Not(F.AlwaysTrue()), F.And(F.AlwaysFalse(), x), F.And(x, F.And(y, F.AlwaysFalse())),
              F.Or(F.AlwaysFalse(), F.AlwaysFalse()), F.Not(F.Or(x, F.AlwaysTrue())),
              F.Or(F.And(F.AlwaysFalse(), x), F.Not(F.AlwaysTrue()))):
        t, un = one(f)
        assert not un and _groups(t) == false and t.n_literals == 0, f
    t, un = F.compile_filters(syn_plan, [x, F.AlwaysFalse()])
    assert not un and _groups(t) == gx + false
    assert wide_plan.fields[_first_filterable(wide_plan)].n_dims == 0
    # an unhandled leaf beside a constant leaves the whole filter unhandled (nothing is guessed)
    bad = F.Or(F.AlwaysTrue(), F.GreaterThan("RATE", 1))
    assert F.compile_filters(wide_plan, [bad])[1] == [bad]


def test_constant_false_without_a_filterable_field_is_unhandled():
    plan = _plan("       01  R.\n           05  RATE   COMP-1.\n           05  T  PIC 9(2) OCCURS 2 TIMES.\n")
    f = F.Not(F.AlwaysTrue())
    t, un = F.compile_filters(plan, [f, F.AlwaysTrue()])
    assert t is None and un == [f] and "constantly false" in un.reasons[0]


def test_compile_filters_with_sets_passes_the_new_classes_through(syn_plan):
    fs = [F.StringContains("NAME", "A"), F.Not(F.EqualNullSafe("BR-ID", 2)), F.AlwaysTrue()]
    t, sets, negate, un = F.compile_filters_with_sets(syn_plan, fs)
    assert not un and not sets and [[op for _, op, _ in g] for g in _groups(t)] == [[N.OP_CONTAINS], [N.OP_IS_NULL, N.OP_NE]]


# ---------------------------------------------------------------------------------------------
# Header constants and the new entry point
# ---------------------------------------------------------------------------------------------
def test_header_constants_and_max_op(tmp_path):
    consts = {"CBX_OP_STARTS_WITH": N.OP_STARTS_WITH, "CBX_OP_NOT_STARTS_WITH": N.OP_NOT_STARTS_WITH,
              "CBX_OP_ENDS_WITH": N.OP_ENDS_WITH, "CBX_OP_NOT_ENDS_WITH": N.OP_NOT_ENDS_WITH,
              "CBX_OP_CONTAINS": N.OP_CONTAINS, "CBX_OP_NOT_CONTAINS": N.OP_NOT_CONTAINS, "CBX_ABI_VERSION": N.ABI_VERSION}
    # (the declaration is used in an unevaluated operand: the program needs no library to link)
    src = ['#include <stdio.h>', '#include "cobrix_hip.h"', "int main(void) {",
           "int32_t (*fn)(void); (void)sizeof(fn = cbx_filter_max_op);",
           'printf("max_op_result_bytes %d\\n", (int)sizeof(cbx_filter_max_op()));']
    src += [f'printf("{c} %d\\n", (int){c});' for c in consts]
    src.append("return 0; }")
    c = tmp_path / "consts.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "consts"
    r = subprocess.run(["gcc", "-I", os.path.dirname(HDR), "-o", str(exe), str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.strip().split("\n"))}
    assert got.pop("max_op_result_bytes") == 4
    assert got == consts and got["CBX_OP_NOT_CONTAINS"] == 16 and got["CBX_ABI_VERSION"] == 25
    lib = N.load()
    assert lib.cbx_filter_max_op() == N.FILTER_MAX_OP == N.OP_NOT_CONTAINS == 16
    assert "cbx_filter_max_op" in N.EXPORTED_SYMBOLS and set(N.FILTER_STRING_SYMBOLS) <= set(N.EXPORTED_SYMBOLS)


# ---------------------------------------------------------------------------------------------
# Literal families drawn from the data (shared with test_gpu_filter_strings.py)
# ---------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 4)
MATCHES_ITS_ROW = {N.OP_ENDS_WITH: ("suffix", "whole"), N.OP_CONTAINS: ("prefix", "suffix", "middle", "whole")}


def data_literals(values, rng: random.Random, per_field: int):
    """{literal bytes: kinds} from `per_field` sampled non-empty values (UTF-8 bytes) of a field: prefix, suffix
    and middle at 1 to 4 bytes and at full length, the whole value, the whole value plus one byte (in front and
    behind), and the empty literal.  Slices are by bytes: some cut a multi-byte character."""
    out = {b"": {"empty"}}
    pool = [v for v in values if v]
    for v in (rng.sample(pool, per_field) if len(pool) > per_field else pool):
        for ln in sorted({min(k, len(v)) for k in LENGTHS} | {len(v)}):
            m = (len(v) - ln) // 2
            for kind, lit in (("prefix", v[:ln]), ("suffix", v[len(v) - ln:]), ("middle", v[m:m + ln])):
                out.setdefault(lit, set()).add(kind)
        out.setdefault(v, set()).add("whole")
        out.setdefault(v + b"A", set()).add("plus_one")
        out.setdefault(bytes([v[-1]]) + v, set()).add("plus_one")
    return out


def raw_table(fi: int, op: int, lits) -> N.CbxFilter:
    """One term built by hand, as a C caller builds it: any byte string is a literal."""
    t = N.CbxFilter()
    t.n_terms, t.n_literals = 1, len(lits)
    t.terms[0].field, t.terms[0].op, t.terms[0].group, t.terms[0].lit_begin, t.terms[0].lit_count = fi, op, 0, 0, len(lits)
    nb = 0
    for k, lit in enumerate(lits):
        t.literals[k].str_off, t.literals[k].str_len = nb, len(lit)
        for b in lit:
            t.pool[nb] = b
            nb += 1
    t.pool_bytes = nb
    return t


def _is_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def string_fields(cb, plan):
    return [nm for nm in leaf_names(cb) if plan.fields[_fi(plan, nm)].kind in (N.K_STRING, N.K_STRING_ASCII)
            and plan.fields[_fi(plan, nm)].n_dims == 0]


def string_family(cb, plan, rows, rng: random.Random, per_field: int = 3, names=None):
    """[(field name, op, literal bytes, kinds)]: every string field crossed with the four ops over its data_literals."""
    out = []
    for nm in names or string_fields(cb, plan):
        values = [_bytes(v) for v in (row_value(cb, r, nm) for r in rows) if v is not None]
        for lit, kinds in data_literals(values, rng, per_field).items():
            out += [(nm, op, lit, kinds) for op in STRING_OPS]
    return out


def family_filter(name: str, op: int, lit):
    """The filter object of a family member (for the evaluator: the literal stays bytes)."""
    return POSITIVE[op](name, lit) if op in POSITIVE else F.Not(NEGATIVE[op](name, lit))


def family_table(plan, name: str, op: int, lit: bytes):
    """The compiled table: through the filter classes where the literal is a str, the raw C table otherwise."""
    if not _is_utf8(lit):
        return raw_table(_fi(plan, name), op, [lit]), True
    cls = POSITIVE.get(op) or NEGATIVE[op]
    f = cls(name, lit.decode("utf-8"))
    t, un = F.compile_filters(plan, [f if op in POSITIVE else F.Not(f)])
    assert not un and t.n_terms == 1 and t.terms[0].op == op, (name, op, lit, un.reasons)
    return t, False


def check_string_family(cb, plan, rows, family, keep_fn, expected=None, from_data=True):
    """Every member through keep_fn(table) -> keep flags, against the evaluator over the oracle's rows.
    Non-vacuity, from the reference alone: a positive op over a literal cut from a value in a way that must
    match that value (MATCHES_ITS_ROW) keeps a row and drops another; a null is kept by neither an
    op nor its negation.  Returns (members, raw-table members).
    from_data=False: hand-made literals, or a single row, which no filter can both keep and drop."""
    expected = {} if expected is None else expected
    bad, raw, must, separated = [], 0, 0, 0
    for name, op, lit, kinds in family:
        key = (name, op, lit)
        exp = expected.get(key)
        if exp is None:
            exp = expected[key] = expected_keep_s(cb, rows, [family_filter(name, op, lit)])
        if from_data and op in POSITIVE and kinds & set(MATCHES_ITS_ROW[op]):
            assert exp.any(), (name, op, lit, kinds)
            must += 1
            separated += not exp.all()
        if op in POSITIVE and "empty" in kinds:
            nulls = np.array([row_value(cb, r, name) is None for r in rows])
            assert np.array_equal(exp, ~nulls)
        table, is_raw = family_table(plan, name, op, lit)
        raw += is_raw
        keep = keep_fn(table)
        assert keep.shape == exp.shape
        for i in np.nonzero(keep != exp)[0][:2]:
            bad.append((name, op, lit, int(i), row_value(cb, rows[i], name), bool(keep[i])))
    print(f"string filters: {len(family)} members, {raw} through the raw table, {must} must match, {separated} of them drop rows, "
          f"{len(bad)} mismatches")
    assert not bad, (len(bad), bad[:5])
    assert not from_data or 0 < must == separated, (must, separated)
    return len(family), raw


def _fixed_fn(lib, plan, data, stride, start_off=0):
    def fn(table):
        rc, keep, err = host_keep(lib, plan, table, data, stride, start_off=start_off)
        assert rc == 0, err
        return keep
    return fn


def _framed_fn(lib, plan, raw, off, ln, seg=None):
    def fn(table):
        rc, keep, err = host_keep_framed(lib, plan, table, raw, off, ln, seg)
        assert rc == 0, err
        return keep
    return fn


# ---------------------------------------------------------------------------------------------
# The host shim against the evaluator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code_page,trim", [("common", "both"), ("cp037", "left"), ("cp875", "none")])
def test_host_fuzz_copybook(host_shim, code_page, trim):   # noqa: F811
    """The three strings of FUZZ_COPYBOOK over random bytes: every code-page entry length, literals that begin
    and end inside a character (raw table)."""
    from oracle import reader_oracle as RO
    from test_decode_fuzz import FUZZ_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", ebcdic_code_page=code_page, string_trimming_policy=trim)
    cb, plan = reader_plan(FUZZ_COPYBOOK, p)
    data = fuzz_records(cb, FUZZ_N, 31)
    rows = RO.fixed_len_rows(cb, data, p)
    family = string_family(cb, plan, rows, random.Random(41), per_field=6)
    n, raw = check_string_family(cb, plan, rows, family, _fixed_fn(host_shim, plan, data, cb.record_size))
    assert n > 300 and (raw > 0 or code_page == "common")


@pytest.mark.parametrize("charset", ["", "windows-1252"])
def test_host_ascii_copybook(host_shim, charset):   # noqa: F811
    from oracle import reader_oracle as RO
    from test_decode_fuzz import ASCII_COPYBOOK
    p = ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, ascii_charset=charset)
    cb, plan = reader_plan(ASCII_COPYBOOK, p)
    data = ascii_records(cb, FUZZ_N, 32)
    rows = RO.fixed_len_rows(cb, data, p)
    names = string_fields(cb, plan)
    assert names and {plan.fields[_fi(plan, nm)].kind for nm in names} == {N.K_STRING if charset else N.K_STRING_ASCII}
    family = string_family(cb, plan, rows, random.Random(42), per_field=8)
    n, _ = check_string_family(cb, plan, rows, family, _fixed_fn(host_shim, plan, data, cb.record_size))
    assert n > 100


@pytest.mark.parametrize("trim", ["none", "both"])
def test_host_width_ladder_cut_at_every_length(host_shim, trim):   # noqa: F811
    """Strings of 1-47 bytes, one record per length 1..L: the register path's partial last word and the pointer
    path with every field cut after each of its bytes; the backward walk starts at the cut."""
    from oracle import reader_oracle as RO
    p = ladder_params(trim)
    cb, plan = reader_plan(LADDER_COPYBOOK, p)
    raw, off, ln = ladder_file(seed=34, every_length=True)
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == cb.record_size
    names = string_fields(cb, plan)
    assert len(names) == 19 and plan.fields[_fi(plan, "X33")].size > 32 >= plan.fields[_fi(plan, "X32")].size
    family = string_family(cb, plan, rows, random.Random(43), per_field=2)
    n, raw_n = check_string_family(cb, plan, rows, family, _framed_fn(host_shim, plan, raw, off, ln))
    assert n > 1000 and raw_n > 0


def test_host_segment_redefines(host_shim):   # noqa: F811
    """A string of a redefine that is not the record's active segment is null: kept by neither an op nor its
    negation."""
    from cobrix_amd.synth import RDW_NARROW_COPYBOOK
    from oracle import oracle as O
    from oracle import reader_oracle as RO
    p = narrow_params()
    cb, plan = reader_plan(RDW_NARROW_COPYBOOK, p)
    raw = narrow_file(300, 21)
    off, ln = O.frame_rdw(raw)
    recs = RO.var_len_records(cb, raw, p)
    rows = RO.var_len_rows(cb, raw, p)
    groups = [g.name.upper() for g in plan.segment_groups]
    seg = np.array([groups.index(r.active_segment.upper()) if r.active_segment is not None else -1 for r in recs],
                   dtype=np.int32)
    assert {-1, 0, 1} == set(seg.tolist())
    family = string_family(cb, plan, rows, random.Random(44), per_field=4)
    expected = {}
    n, _ = check_string_family(cb, plan, rows, family, _framed_fn(host_shim, plan, raw, off, ln, seg), expected)
    assert n > 200
    nulls = np.array([row_value(cb, r, "COMPANY-NAME") is None for r in rows])
    assert nulls.any() and not nulls.all()
    seen = 0
    for (name, op, lit), exp in expected.items():
        if name.replace("_", "-") == "COMPANY-NAME":   # (leaf names are the transformed identifiers)
            assert not exp[nulls].any()
            seen += 1
    assert seen >= 4 * 8


# ---------------------------------------------------------------------------------------------
# Hand-made cases
# ---------------------------------------------------------------------------------------------
HAND_COPYBOOK = """
       01  R.
           05  A             PIC X(8).
           05  B             PIC X(1).
           05  L             PIC X(40).
"""
HAND_VALUES = ["aaab", "abababc", "abab", "aab", "", "b", "ababc", "aaaaaaab", "c", "ab ab"]
HAND_LITERALS = ["aab", "ababc", "aaab", "abababc", "", "b", "a", "ab", "abab", "c", "aaaaaaab", "aaaaaaaab", "bab", "b ab", " "]


def hand_records() -> bytes:
    """A and L hold the same value (registers / the pointer path), B its first character."""
    return b"".join(v.ljust(8).encode() + v[:1].ljust(1).encode() + v.ljust(40).encode() for v in HAND_VALUES)


def hand_params(trim: str = "both") -> ReaderParameters:
    return ReaderParameters(schema_policy="collapse_root", is_ebcdic=False, string_trimming_policy=trim)


def hand_family():
    return [(nm, op, lit.encode(), {"hand"}) for nm in ("A", "B", "L") for lit in HAND_LITERALS for op in STRING_OPS]


@pytest.mark.parametrize("trim", ["both", "none"])
def test_host_hand_made_cases(host_shim, trim):   # noqa: F811
    """Restarts after a partial match ("aab" in "aaab", "ababc" in "abababc"), a literal equal to the value, a
    value that trims to empty against the empty and a one-byte literal, a one-byte field; the same for ENDS_WITH."""
    from oracle import reader_oracle as RO
    p = hand_params(trim)
    cb, plan = reader_plan(HAND_COPYBOOK, p)
    data = hand_records()
    rows = RO.fixed_len_rows(cb, data, p)
    assert [r["A"] for r in rows] == ([v for v in HAND_VALUES] if trim == "both" else [v.ljust(8) for v in HAND_VALUES])
    fn = _fixed_fn(host_shim, plan, data, cb.record_size)

    def kept(name, op, lit):
        return [HAND_VALUES[i] for i in np.nonzero(fn(family_table(plan, name, op, lit.encode())[0]))[0]]

    if trim == "both":
        for nm in ("A", "L"):
            assert kept(nm, N.OP_CONTAINS, "aab") == ["aaab", "aab", "aaaaaaab"]
            assert kept(nm, N.OP_CONTAINS, "ababc") == ["abababc", "ababc"]
            assert kept(nm, N.OP_ENDS_WITH, "aab") == ["aaab", "aab", "aaaaaaab"]
            assert kept(nm, N.OP_ENDS_WITH, "ababc") == ["abababc", "ababc"]
            assert kept(nm, N.OP_ENDS_WITH, "abab") == ["abab"] and kept(nm, N.OP_CONTAINS, "abab") == ["abababc", "abab", "ababc"]
            assert kept(nm, N.OP_CONTAINS, "aaaaaaab") == ["aaaaaaab"] == kept(nm, N.OP_ENDS_WITH, "aaaaaaab")
            assert kept(nm, N.OP_CONTAINS, "aaaaaaaab") == [] == kept(nm, N.OP_ENDS_WITH, "aaaaaaaab")
            assert kept(nm, N.OP_CONTAINS, "") == HAND_VALUES == kept(nm, N.OP_ENDS_WITH, "")
            assert kept(nm, N.OP_NOT_CONTAINS, "") == [] == kept(nm, N.OP_NOT_ENDS_WITH, "")
            assert "" not in kept(nm, N.OP_CONTAINS, "b") and "" in kept(nm, N.OP_NOT_CONTAINS, "b")
            assert "" not in kept(nm, N.OP_ENDS_WITH, "b") and "" in kept(nm, N.OP_NOT_ENDS_WITH, "b")
        assert kept("B", N.OP_CONTAINS, "a") == [v for v in HAND_VALUES if v[:1] == "a"] == kept("B", N.OP_ENDS_WITH, "a")
        assert kept("B", N.OP_CONTAINS, "ab") == []
    n, _ = check_string_family(cb, plan, rows, hand_family(), fn, from_data=False)
    assert n == 3 * len(HAND_LITERALS) * 4


def test_raw_table_rejections(host_shim, wide_plan):   # noqa: F811
    """filter_build: an op above 16 is unknown; the string ops take a string field and exactly one literal."""
    rec = bytes(wide_plan.copybook.record_size)
    name, num = _fi(wide_plan, "NAME"), _fi(wide_plan, "ID")
    rc, _, err = host_keep(host_shim, wide_plan, raw_table(name, 17, [b"A"]), rec, len(rec))
    assert rc == N.CBX_E_ARGUMENT and "unknown op" in err
    for op, word in ((N.OP_ENDS_WITH, "ENDS_WITH"), (N.OP_NOT_ENDS_WITH, "ENDS_WITH"), (N.OP_CONTAINS, "CONTAINS"),
                     (N.OP_NOT_CONTAINS, "CONTAINS")):
        rc, _, err = host_keep(host_shim, wide_plan, raw_table(num, op, [b"1"]), rec, len(rec))
        assert rc == N.CBX_E_ARGUMENT and f"{word} on a numeric field" in err
        for lits in ([], [b"A", b"B"]):
            rc, _, err = host_keep(host_shim, wide_plan, raw_table(name, op, lits), rec, len(rec))
            assert rc == N.CBX_E_ARGUMENT and "literal" in err
        assert host_keep(host_shim, wide_plan, raw_table(name, op, [b"A"]), rec, len(rec))[0] == 0
    rc, _, err = host_keep(host_shim, wide_plan, raw_table(_fi(wide_plan, "RATE"), N.OP_CONTAINS, [b"1"]), rec, len(rec))
    assert rc == N.CBX_E_UNSUPPORTED and "COMP-1" in err


def test_constants_and_null_safe_equality_on_the_host(host_shim):   # noqa: F811
    """Trees with the constants and EqualNullSafe through compile_filters and the evaluator: nulls are plentiful
    (a fifth of SYN200's numeric fields malformed)."""
    from cobrix_amd.reader import parse_copybook_for
    from cobrix_amd.synth import syn200
    from oracle import oracle as O
    cb = parse_copybook_for(SYN200_COPYBOOK, ReaderParameters())
    plan = _plan(SYN200_COPYBOOK)
    data = syn200(500, seed=5, malformed_rate=0.2).numpy().tobytes()
    rows = O.rows(O.decode_fixed(cb, data), collapse_root=True)
    amt = next(v for v in (row_value(cb, r, "AMT-01") for r in rows) if v is not None)
    name = next(v for v in (row_value(cb, r, "NAME") for r in rows) if v)
    x = F.StringContains("NAME", name[:1])
    cases = [[F.EqualNullSafe("AMT-01", amt)], [F.Not(F.EqualNullSafe("AMT-01", amt))], [F.EqualNullSafe("AMT-01", None)],
             [F.Not(F.EqualNullSafe("AMT-01", None))], [F.EqualNullSafe("NAME", name)], [F.Not(F.EqualNullSafe("NAME", name))],
             [F.Or(F.AlwaysFalse(), x)], [F.Not(F.AlwaysTrue())], [F.And(x, F.Not(F.EqualNullSafe("AMT-02", None)))],
             [x, F.AlwaysTrue()], [F.Not(F.Or(F.EqualNullSafe("AMT-01", amt), F.StringEndsWith("NAME", name[-1:])))]]
    for filters in cases:
        t, un = F.compile_filters(plan, filters)
        assert not un and t is not None, (filters, un.reasons)
        rc, keep, err = host_keep(host_shim, plan, t, data, 200)
        assert rc == 0, err
        exp = expected_keep_s(cb, rows, filters)
        assert np.array_equal(keep, exp), (filters, np.nonzero(keep != exp)[0][:5])
        if filters == [F.Not(F.AlwaysTrue())]:
            assert not exp.any()
        else:
            assert exp.any() and not exp.all(), filters
    nulls = np.array([row_value(cb, r, "AMT-01") is None for r in rows])
    assert nulls.any() and expected_keep_s(cb, rows, cases[1])[nulls].all()   # NOT (a <=> v) keeps the nulls


# ---------------------------------------------------------------------------------------------
# The stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------
def test_host_program_under_the_sanitizers(tmp_path):
    """tests/native/filter_strings_host_main.cpp built with -fsanitize=address,undefined: the four ops over field
    sizes 1-40, the record cut at every length, 0-16 bytes in front of it, in exact-size heap buffers, literal
    lengths 0-5; every answer checked against a naive search.  A subprocess of its own: nothing loaded into
    Python runs under a sanitizer."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path / "filter_strings_host_check"
    native = os.path.join(ROOT, "tests", "native")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cobrix_amd", "csrc"), "-o", str(exe),
                        os.path.join(native, "filter_host.cpp"), os.path.join(native, "filter_strings_host_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-4000:], r.stdout)
    assert "no sanitizer report" in r.stdout
