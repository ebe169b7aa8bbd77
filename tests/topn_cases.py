"""Top-N pushdown: what the CPU tests (test_topn.py) and the GPU tests (test_gpu_topn.py) share -- the contract
over the oracle's rows, stated twice and independently of the code under test:

- `expected_indices`: the EVALUATOR.  sorted(kept indices, key = compare the keys' values with the None and
  direction rules, then the index)[:limit], ascending.  It knows nothing about the composite key.
- `encode_composite`: the ENCODER of the composite key (cbx_topn.h) from a row's values, and `expected_info`,
  which derives from the encoded keys how many select levels a call must run and how large its tie classes are
  (by sorting, not by a radix select).

and the synthetic case tables with their expected `cbx_topn_info` values written out.
"""
from __future__ import annotations

import decimal
import functools
from decimal import Decimal

import numpy as np

from cobrix_amd import native as N
from cobrix_amd.topn import SortOrder, compare_values
from test_filter import py_keep, row_value

ALL_FLAGS = [(False, True), (False, False), (True, True), (True, False)]   # (descending, nulls_first)


def _fi(plan, name):
    return plan.field_of_node[id(plan.copybook.get_field_by_name(name))]


def kept_indices(cb, rows, filters=()):
    return [i for i, r in enumerate(rows) if py_keep(cb, r, filters)] if filters else list(range(len(rows)))


def expected_indices(cb, rows, orders, limit, filters=()):
    """(kept, chosen): the indices the filters keep, and of them the first `limit` under `orders` (ties by index),
    ascending."""
    kept = kept_indices(cb, rows, filters)
    vals = {i: [row_value(cb, rows[i], so.column) for so in orders] for i in kept}

    def cmp(a, b):
        for so, x, y in zip(orders, vals[a], vals[b]):
            c = compare_values(x, y, so)
            if c:
                return c
        return (a > b) - (a < b)
    return kept, sorted(sorted(kept, key=functools.cmp_to_key(cmp))[:limit])


def unscaled(v, scale: int) -> int:
    if isinstance(v, Decimal):
        with decimal.localcontext() as ctx:
            ctx.prec = 120
            u = v.scaleb(scale)
            assert u == u.to_integral_value(), (v, scale)
            return int(u)
    assert isinstance(v, (int, np.integer)) and not isinstance(v, bool), (type(v), v)
    return int(v)


def encode_composite(plan, orders, values, index: int) -> bytes:
    """The composite key of cbx_topn.h from a row's key values (None: null)."""
    out = bytearray()
    for so, v in zip(orders, values):
        f = plan.fields[_fi(plan, so.column)]
        is_str = f.kind in (N.K_STRING, N.K_STRING_ASCII)
        width = 3 * f.size + 1 if is_str else {N.O_I32: 4, N.O_I64: 8, N.O_DEC64: 8, N.O_DEC128: 16}[f.out_type]
        if v is None:
            out += bytes([0 if so.nulls_first_resolved else 2]) + bytes(width)
            continue
        if is_str:
            u = v.encode("utf-8")
            assert len(u) <= 3 * f.size
            payload = u + bytes(3 * f.size - len(u)) + bytes([len(u)])
        else:
            x = unscaled(v, f.out_scale if f.out_type in (N.O_DEC64, N.O_DEC128) else 0)
            payload = ((x + (1 << (8 * width - 1))) % (1 << (8 * width))).to_bytes(width, "big")
            assert -(1 << (8 * width - 1)) <= x < 1 << (8 * width - 1)
        if so.descending:
            payload = bytes(b ^ 0xFF for b in payload)
        out += b"\x01" + payload
    out += bytes(-len(out) % 8)
    return bytes(out) + index.to_bytes(8, "big")


def composite_keys(cb, plan, rows, orders):
    return [encode_composite(plan, orders, [row_value(cb, r, so.column) for so in orders], i) for i, r in enumerate(rows)]


def expected_info(keys, kept, limit: int, n_rec: int) -> dict:
    """How cbx_top_n_records must run over the composite keys `keys` (one per source record), `kept` the indices
    the filter keeps: by sorting each level's 8-byte words."""
    info = {"n_live": len(kept), "levels_run": 0, "ties_after_level0": 0, "ties_max": 0,
            "levels_total": len(keys[0]) // 8 if keys else None}
    if n_rec == 0:
        return dict(info, n_live=0)
    if limit == 0:
        return dict(info, n_live=-1)
    if limit >= n_rec:
        return info
    cand, need, level = list(kept), limit, 0
    while True:
        info["levels_run"] = level + 1
        if level == 0 and need >= len(cand):
            return info
        words = sorted(keys[i][8 * level:8 * level + 8] for i in cand)
        t = words[need - 1]
        below = sum(w < t for w in words)
        ties = sum(w == t for w in words)
        need -= below
        if ties == need:
            return info
        if level == 0:
            info["ties_after_level0"] = ties
        info["ties_max"] = max(info["ties_max"], ties)
        cand = [i for i in cand if keys[i][8 * level:8 * level + 8] == t]
        level += 1


# ---------------------------------------------------------------------------------------------
# Synthetic fixed-length records with every kind of key the select has to get right
# ---------------------------------------------------------------------------------------------
KEYS_COPYBOOK = """
       01  R.
           05  SEQ   PIC 9(9) COMP.
           05  CST   PIC S9(4) COMP.
           05  LOW   PIC S9(4) COMP.
           05  LNG   PIC S9(18) COMP.
           05  BIG   PIC S9(38) COMP-3.
           05  AMT   PIC S9(7)V99 COMP-3.
           05  TXT   PIC X(6).
           05  HEX   PIC X(3).
"""
KEYS_OPTIONS = dict(schema_policy="collapse_root", ebcdic_code_page="cp037")
KEYS_SIZE = 4 + 2 + 2 + 8 + 20 + 5 + 6 + 3
TOP38 = 10 ** 38 - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _bcd(v: int, size: int) -> bytes:
    nib = [int(c) for c in str(abs(v)).rjust(2 * size - 1, "0")] + [0xD if v < 0 else 0xC]
    return bytes((nib[2 * j] << 4) | nib[2 * j + 1] for j in range(size))


def keys_records(n: int, seed: int = 7) -> bytes:
    """n records.  CST is constant; LOW takes 5 values in an order that spreads every value over all tiles; LNG
    cycles through INT64 min / max, -1, 0, 1 and random values (S9(18) COMP holds any 64-bit pattern); BIG through
    +-(10^38 - 1), 0 and random 38-digit values, every 11th malformed (null); AMT random, every 7th malformed; TXT
    cp037 text with blanks and a two-byte character, every 13th all blanks (the empty string under trimming); HEX
    three bytes of pound / cent (two UTF-8 bytes each, 0xC2 first), 'A' and blank -- under DESC the zero padding
    behind a short value becomes 0xFF bytes."""
    rng = np.random.default_rng(seed)
    lng_edge = [I64_MIN, I64_MAX, -1, 0, 1]
    big_edge = [TOP38, -TOP38, 0]
    letters = [0xC1, 0xC2, 0x5F, 0x81, 0x40, 0xF0]
    out = bytearray()
    for i in range(n):
        lng = lng_edge[i % 8] if i % 8 < 5 else int(rng.integers(I64_MIN, I64_MAX, endpoint=True))
        big = big_edge[i % 5] if i % 5 < 3 else int(rng.integers(0, 10 ** 18)) * int(rng.integers(0, 10 ** 18)) * (-1) ** i
        out += i.to_bytes(4, "big") + (42).to_bytes(2, "big") + ((i * 7) % 5 - 2).to_bytes(2, "big", signed=True)
        out += lng.to_bytes(8, "big", signed=True)
        out += b"\xAA" * 20 if i % 11 == 10 else _bcd(big, 20)
        out += b"\xFF" * 5 if i % 7 == 6 else _bcd(int(rng.integers(-10 ** 9 + 1, 10 ** 9)), 5)
        out += bytes([0x40] * 6) if i % 13 == 12 else bytes(letters[int(k)] for k in rng.integers(0, 6, 6))
        out += bytes([(0xB1, 0x4A, 0xC1, 0x40)[int(k)] for k in rng.integers(0, 4, 3)])
    assert len(out) == n * KEYS_SIZE
    return bytes(out)


def S(column, descending=False, nulls_first=None):
    return SortOrder(column, descending, nulls_first)


# (name, n_rec, orders, limit, max_workgroups, odd address, expected cbx_topn_info values): n_live / levels_run /
# ties_after_level0 as `expected_info` derives them from the oracle's rows -- test_topn.py pins every literal here
# against it, test_gpu_topn.py asserts the library's cbx_top_n_info against the literals.
KEYS_CASES = [
    # n_rec in {1, 63, 64, 65, 1000, 4097}, limits around the tile and the batch
    ("one_record", 1, [S("AMT")], 1, 0, False, (1, 0, 0)),
    ("n63_limit1", 63, [S("AMT", True)], 1, 0, False, (63, 1, 0)),
    ("n64_limit63", 64, [S("LNG")], 63, 0, False, (64, 3, 8)),
    ("n64_limit64", 64, [S("LNG")], 64, 0, False, (64, 0, 0)),
    ("n65_limit64", 65, [S("LNG", True)], 64, 0, True, (65, 3, 9)),
    ("n65_limit65", 65, [S("LNG")], 65, 0, False, (65, 0, 0)),
    ("n65_limit66", 65, [S("LNG")], 66, 0, False, (65, 0, 0)),
    ("n1000_limit999", 1000, [S("AMT")], 999, 3, False, (1000, 1, 0)),
    ("n1000_limit0", 1000, [S("AMT")], 0, 0, False, (-1, 0, 0)),
    ("n0", 0, [S("AMT")], 5, 0, False, (0, 0, 0)),
    # constant key: every row ties on word 0 (null byte + value + padding), the first n by index win
    ("constant_first_n", 1000, [S("CST")], 65, 1, False, (1000, 2, 1000)),
    ("constant_desc", 4097, [S("CST", True)], 100, 3, False, (4097, 2, 4097)),
    # low cardinality: the boundary class spans every tile and workgroup
    ("low_card", 4097, [S("LOW")], 1000, 0, False, (4097, 2, 819)),
    ("low_card_one_wg", 4097, [S("LOW", True, True)], 1700, 1, True, (4097, 2, 820)),
    # extremes at digit 0x00 / 0xFF of every round
    ("int64_extremes_asc", 1000, [S("LNG")], 100, 0, False, (1000, 3, 125)),
    ("int64_extremes_desc", 1000, [S("LNG", True)], 130, 3, False, (1000, 1, 0)),
    ("dec128_extremes", 1000, [S("BIG")], 150, 0, False, (1000, 4, 182)),
    ("dec128_desc_nulls_first", 1000, [S("BIG", True, True)], 95, 0, False, (1000, 4, 182)),
    ("ff_string_bytes", 1000, [S("HEX", True)], 64, 0, False, (1000, 3, 34)),
    # the four flag combinations on a key with nulls
    ("amt_asc_nf", 1000, [S("AMT", False, True)], 100, 0, False, (1000, 3, 142)),
    ("amt_asc_nl", 1000, [S("AMT", False, False)], 900, 0, False, (1000, 3, 142)),
    ("amt_desc_nf", 1000, [S("AMT", True, True)], 100, 0, False, (1000, 3, 142)),
    ("amt_desc_nl", 1000, [S("AMT", True, False)], 990, 3, False, (1000, 3, 142)),
    # two and four keys, strings and numbers mixed
    ("two_keys", 1000, [S("LOW"), S("TXT", True)], 333, 0, False, (1000, 1, 0)),
    ("four_keys", 4097, [S("TXT"), S("LOW", True), S("BIG", False, False), S("AMT", True)], 2000, 3, True, (4097, 4, 2)),
    ("four_keys_const_first", 1000, [S("CST"), S("LOW"), S("HEX"), S("LNG", True)], 500, 0, False, (1000, 2, 600)),
    # the plain LIMIT
    ("limit_only", 1000, [], 65, 0, False, (1000, 1, 0)),
]
