"""Key-set filters on the GPU (cbx_key_set_create, cbx_filter_records_keyed -> cbx_decode_selected) against the contract:
the rows of the ORACLE read whose key columns have no None and whose key tuple is (not) in the Python set, and that the
other filters keep (test_keyset.py expected_set_keep over the oracle's rows -- never the code under test), in file
order, ids carried.  Every test calls entry points the library did not have before key sets (cbx_key_set_create,
cbx_filter_records_keyed): none of them passes without the feature.
"""
from __future__ import annotations

import ctypes
from decimal import Decimal

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from cobrix_amd import aggregate as A  # noqa: E402
from cobrix_amd import filter as F  # noqa: E402
from cobrix_amd import native as N  # noqa: E402
from cobrix_amd.keyset import KeySet  # noqa: E402
from cobrix_amd.options import parse_options  # noqa: E402
from cobrix_amd.reader import FixedLenNestedReader, ReaderParameters, VarLenNestedReader  # noqa: E402
from cobrix_amd.synth import RDW_NARROW_COPYBOOK, SYN200_COPYBOOK, rdw_file, syn200  # noqa: E402
from oracle import reader_oracle as RO  # noqa: E402
from test_aggregate import ALL_FUNCS, expected_aggregates  # noqa: E402
from test_filter import py_keep, row_value  # noqa: E402
from test_gpu_filter import NARROW_OPTIONS, _flags  # noqa: E402
from test_gpu_filter import narrow  # noqa: E402,F401  (fixture)
from test_group import check_groups, expected_groups  # noqa: E402
from test_keyset import distinct_keys, expected_set_keep, half  # noqa: E402
from topn_cases import S, expected_indices  # noqa: E402

PARAMS = ReaderParameters(schema_policy="collapse_root")
COUNTS = [1, 63, 64, 65, 321]
SET_SIZES = [0, 1, 2, 64, 65, 1000, 70000]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _device(data: bytes):
    return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()


def _kept_rows(cb, rows, filters, specs):
    keep = expected_set_keep(cb, rows, filters, specs)
    return [r for r, k in zip(rows, keep) if k]


def _fixed_flags(rd, t, n_bytes, n, sets, negate, table=None, first_record_id=0):
    sel = rd._filter_records(table, t, n_bytes, n, torch.cuda.current_stream(), stride=rd.get_record_size(),
                             first_record_id=first_record_id, sets=sets, negate=negate)
    k = sel["n"]
    assert np.array_equal(sel["rec_off"][:k].cpu().numpy(), (sel["record_id"][:k].cpu().numpy() - first_record_id) * 200)
    assert (sel["rec_len"][:k].cpu().numpy() == 200).all()
    return _flags(sel["record_id"][:k].cpu().numpy() - first_record_id, n, (sets, negate))


# ---------------------------------------------------------------------------------------------
# Fixed-length SYN200, a fifth of the numeric fields malformed: record counts x set sizes
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syn():
    """(reader, data of 321 records, oracle rows, device tensor) -- computed once, shared, never changed."""
    rd = FixedLenNestedReader(SYN200_COPYBOOK, PARAMS)
    data = syn200(321, seed=11, malformed_rate=0.2).numpy().tobytes()
    rows = RO.fixed_len_rows(rd.copybook, data, PARAMS)
    assert len(rows) == 321
    yield rd, data, rows, _device(data)
    rd.close()


@pytest.fixture(scope="module")
def acct_sets(syn):
    """{size: (values, KeySet)} over ACCT-NO (int64): every other present key first, then values no record has."""
    rd, data, rows, t = syn
    present = half(distinct_keys(rd.copybook, rows, ["ACCT-NO"]))
    have = {k[0] for k in distinct_keys(rd.copybook, rows, ["ACCT-NO"])}
    absent = [v for v in range(-35000, 36000) if v not in have]
    out = {}
    for size in SET_SIZES:
        vals = ([k[0] for k in present] + absent)[:size] if size else []
        # the record of a one-row batch is in every non-empty set
        if size:
            vals[-1] = row_value(rd.copybook, rows[0], "ACCT-NO")
        out[size] = (vals, rd.key_set(["ACCT-NO"], vals))
    assert row_value(rd.copybook, rows[0], "ACCT-NO") is not None
    yield out
    for _, ks in out.values():
        ks.close()


def test_set_info(syn, acct_sets):
    for size, (vals, ks) in acct_sets.items():
        info = ks.info()
        cap = 2
        while cap < 2 * size:
            cap <<= 1
        assert (info.n_values, info.n_distinct, info.capacity, info.n_keys) == (size, len(set(vals)), cap, 1), size
        assert 0 <= info.max_probe <= cap and (info.max_probe >= 1) == (size > 0) and info.device_bytes >= 8 * cap + 24 * size
        assert ks.dropped == 0 and not ks.has_null and info.build_ms == 0.0
    assert acct_sets[70000][1].info().capacity == 1 << 18          # more than one build workgroup
    rd = syn[0]
    with rd.key_set(["BR-ID", "NAME"], [(7, "SAME")] * 1000) as dup:
        assert (dup.info().n_values, dup.info().n_distinct) == (1000, 1)
    assert dup.closed
    with pytest.raises(ValueError):
        dup.info()


@pytest.mark.parametrize("n", COUNTS)
def test_record_counts_and_set_sizes(syn, acct_sets, n):
    rd, data, rows, t = syn
    cb = rd.copybook
    kept = []
    for size, (vals, ks) in acct_sets.items():
        for neg in (0, 1):
            exp = expected_set_keep(cb, rows[:n], [], [(["ACCT-NO"], vals, neg)])
            got = _fixed_flags(rd, t, 200 * n, n, [ks], [neg])
            assert np.array_equal(got, exp), (size, neg, np.flatnonzero(got != exp)[:8])
            kept.append(int(exp.sum()))
    if n == 321:
        assert any(0 < k < n for k in kept) and 0 in kept
    b = rd.decode_device(t, 200 * n, filters=[F.InSet(acct_sets[1000][1])])
    assert b.unhandled_filters == [] and b.to_rows() == _kept_rows(cb, rows[:n], [], [(["ACCT-NO"], acct_sets[1000][0], 0)])


def test_no_records_launches_nothing(syn, acct_sets):
    rd, data, rows, t = syn
    sel = rd._filter_records(None, t, 0, 0, torch.cuda.current_stream(), stride=200, sets=[acct_sets[64][1]], negate=[0])
    assert sel["n"] == 0


def test_first_record_id_and_pass_times(syn, acct_sets):
    rd, data, rows, t = syn
    vals, ks = acct_sets[65]
    exp = expected_set_keep(rd.copybook, rows, [], [(["ACCT-NO"], vals, 0)])
    L = N.load()
    N.check(L.cbx_plan_set_profiling(rd.native.handle, 1))
    try:
        assert np.array_equal(_fixed_flags(rd, t, len(data), 321, [ks], [0], first_record_id=5000), exp)
        ms = [ctypes.c_float(-1) for _ in range(3)]
        N.check(L.cbx_filter_pass_times(rd.native.handle, *[ctypes.byref(m) for m in ms]))
        assert all(m.value > 0 for m in ms)
        with rd.key_set(["ACCT-NO"], vals) as timed:
            assert timed.info().build_ms > 0
    finally:
        N.check(L.cbx_plan_set_profiling(rd.native.handle, 0))
    _fixed_flags(rd, t, len(data), 321, [ks], [0])
    N.check(L.cbx_filter_pass_times(rd.native.handle, *[ctypes.byref(m) for m in ms]))
    assert all(m.value == 0 for m in ms)


# ---------------------------------------------------------------------------------------------
# Two sets at once, with and without a cbx_filter; the differential against OP_IN / OP_NOT_IN
# ---------------------------------------------------------------------------------------------
def test_two_sets_with_and_without_a_filter(syn):
    rd, data, rows, t = syn
    cb = rd.copybook
    br, nm = distinct_keys(cb, rows, ["BR-ID"]), distinct_keys(cb, rows, ["NAME"])
    a_vals, b_vals = br[: 2 * len(br) // 3], half(nm)
    with rd.key_set(["BR-ID"], a_vals) as a, rd.key_set(["NAME"], b_vals) as b:
        specs = [(["BR-ID"], a_vals, 0), (["NAME"], b_vals, 1)]
        for plain in ([], [F.GreaterThan("AMT-01", 0)], [F.Or(F.IsNull("QTY-01"), F.LessThan("ZD-01", 0))]):
            batch = rd.decode_device(t, len(data), filters=plain + [F.InSet(a), F.Not(F.InSet(b))])
            exp = _kept_rows(cb, rows, plain, specs)
            assert batch.unhandled_filters == [] and batch.to_rows() == exp
            assert 0 < len(exp) < len(rows)
        # a filter the stage cannot push stays with the caller, the sets are still applied
        odd = F.In("BR-ID", list(range(65)))
        batch = rd.decode_device(t, len(data), filters=[odd, F.InSet(a)])
        assert batch.unhandled_filters == [odd] and batch.to_rows() == _kept_rows(cb, rows, [], specs[:1])


@pytest.mark.parametrize("column", ["BR-ID", "ACCT-NO", "AMT-01", "ZD-01", "NAME"])
def test_differential_against_in_literals(syn, column):
    """Single-column sets of at most 64 values: the selection equals cbx_filter_records with OP_IN / OP_NOT_IN on the
    same literals, array for array."""
    rd, data, rows, t = syn
    cb = rd.copybook
    keys = [k[0] for k in distinct_keys(cb, rows, [column])]
    st = torch.cuda.current_stream()
    most = 40 if column == "NAME" else 64          # (64 names of 18 bytes would not fit the literal pool)
    for vals in (keys[:1], half(keys)[:most], keys[-3:] + keys[-3:]):
        with rd.key_set([column], vals) as ks:
            for neg, flt in ((0, F.In(column, vals)), (1, F.Not(F.In(column, vals)))):
                table, un = F.compile_filters(rd.plan, [flt])
                assert not un
                old = rd._filter_records(table, t, len(data), 321, st, stride=200, first_record_id=7)
                new = rd._filter_records(None, t, len(data), 321, st, stride=200, first_record_id=7, sets=[ks], negate=[neg])
                assert old["n"] == new["n"] and (neg or old["n"] > 0)
                for arr in ("rec_off", "rec_len", "record_id", "segment"):
                    assert torch.equal(old[arr][:old["n"]], new[arr][:new["n"]]), (column, neg, arr)


# ---------------------------------------------------------------------------------------------
# Key shapes: int32 / int64 / DEC64 / DEC128 with negatives, strings of 1, 12, 13 and 32 bytes over a code page with
# two-byte entries, a composite of four mixed kinds
# ---------------------------------------------------------------------------------------------
SHAPES_COPYBOOK = """
       01  R.
           05  K32   PIC S9(9) COMP.
           05  K64   PIC S9(18) COMP.
           05  KD    PIC S9(13)V99 COMP-3.
           05  KB    PIC S9(25)V9(5) COMP-3.
           05  S01   PIC X(1).
           05  S12   PIC X(12).
           05  S13   PIC X(13).
           05  S32   PIC X(32).
"""
SHAPES_SIZE = 4 + 8 + 8 + 16 + 1 + 12 + 13 + 32
_TWO = [0x4A, 0x5F, 0xB1, 0xB2, 0x9E]          # cp037 bytes whose characters take two UTF-8 bytes
_ONE = [0xC1, 0xC2, 0x81, 0xF1]


def _bcd(v: int, size: int, bad: bool = False) -> bytes:
    nib = [int(c) for c in str(abs(v)).rjust(2 * size - 1, "0")] + [0xD if v < 0 else 0xC]
    if bad:
        nib[3] = 0xB
    return bytes((nib[2 * j] << 4) | nib[2 * j + 1] for j in range(size))


def shapes_records(n: int) -> bytes:
    """Values drawn from small pools (so that keys repeat), negatives and the types' extremes among them, a tenth of the
    COMP-3 fields malformed; strings of full width, blank, and padded on either side."""
    rng = np.random.default_rng(41)
    p32 = [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 123456, -123456]
    p64 = [0, -1, 2 ** 40, -2 ** 40, 10 ** 18 - 1, -(10 ** 18 - 1), 77]
    pd = [0, -1, 150, -150, 10 ** 15 - 1, -(10 ** 15 - 1)]
    pb = [0, -1, 10 ** 29, -(10 ** 29), 10 ** 30 - 1, -(10 ** 30 - 1), 12345, 2 ** 64, -(2 ** 64)]

    def text(size):
        k = int(rng.integers(0, 4))
        body = [int(rng.choice(_TWO + _ONE)) for _ in range(size if k == 0 else int(rng.integers(0, min(size, 3) + 1)))]
        lead = 0 if k < 2 else int(rng.integers(0, size - len(body) + 1))
        return bytes([0x40] * lead + body + [0x40] * (size - lead - len(body)))

    out = bytearray()
    for _ in range(n):
        out += int(rng.choice(p32)).to_bytes(4, "big", signed=True) + int(p64[int(rng.integers(0, 7))]).to_bytes(8, "big", signed=True)
        out += _bcd(pd[int(rng.integers(0, 6))], 8, rng.random() < 0.1) + _bcd(pb[int(rng.integers(0, 9))], 16, rng.random() < 0.1)
        out += text(1) + text(12) + text(13) + text(32)
    assert len(out) == n * SHAPES_SIZE
    return bytes(out)


@pytest.fixture(scope="module", params=["both", "none"])
def shapes(request):
    p = ReaderParameters(schema_policy="collapse_root", string_trimming_policy=request.param, ebcdic_code_page="cp037")
    rd = FixedLenNestedReader(SHAPES_COPYBOOK, p)
    assert rd.copybook.record_size == SHAPES_SIZE
    data = shapes_records(321)
    rows = RO.fixed_len_rows(rd.copybook, data, p)
    types = [rd.plan.fields[rd.plan.field_of_node[id(rd.copybook.get_field_by_name(c))]].out_type for c in ("K32", "K64", "KD", "KB")]
    assert types == [N.O_I32, N.O_I64, N.O_DEC64, N.O_DEC128]
    assert any(len(r["S32"].encode()) > 32 for r in rows) and any(r["KB"] is None for r in rows)
    assert any(r["KB"] is not None and r["KB"] < -10 ** 20 for r in rows)
    yield rd, data, rows, _device(data)
    rd.close()


@pytest.mark.parametrize("names", [["K32"], ["K64"], ["KD"], ["KB"], ["S01"], ["S12"], ["S13"], ["S32"], ["K32", "KB", "S13", "KD"],
                                   ["S32", "S01", "S12", "K64"]])
def test_key_shapes(shapes, names):
    rd, data, rows, t = shapes
    cb = rd.copybook
    keys = distinct_keys(cb, rows, names)
    assert len(keys) >= 3
    vals = half(keys)
    with rd.key_set(names, vals + vals[:2]) as ks:
        assert ks.info().n_distinct == len(vals) and ks.dropped == 0
        b = rd.decode_device(t, len(data), filters=[F.InSet(ks)])
        exp = _kept_rows(cb, rows, [], [(names, vals, 0)])
        assert b.unhandled_filters == [] and b.to_rows() == exp and 0 < len(exp) < len(rows)
        flt = F.NotInSet(ks)
        b = rd.decode_device(t, len(data), filters=[flt])
        if len(names) == 1:
            exp = _kept_rows(cb, rows, [], [(names, vals, 1)])
            assert b.unhandled_filters == [] and b.to_rows() == exp and 0 < len(exp) < len(rows)
        else:   # a negated composite is handed back, nothing is filtered
            assert b.unhandled_filters == [flt] and b.n_rec == len(rows)


# ---------------------------------------------------------------------------------------------
# Framed records with a fifth cut short; a selection with Seg_Id levels
# ---------------------------------------------------------------------------------------------
def test_framed_records_a_fifth_cut_short(syn):
    _, data, _, _ = syn
    recs = [data[200 * i:200 * (i + 1)] for i in range(321)]
    recs = [r[:(37 * i) % 200 + 1] if i % 5 == 4 else r for i, r in enumerate(recs)]
    raw = rdw_file(recs)
    p = ReaderParameters(is_record_sequence=True, schema_policy="collapse_root", generate_record_id=True)
    rd = VarLenNestedReader(SYN200_COPYBOOK, p)
    cb = rd.copybook
    rows = RO.var_len_rows(cb, raw, p)
    assert len(rows) == 321
    for names in (["BR-ID"], ["ZD-01"], ["NAME"], ["ACCT-NO", "NAME", "AMT-08"]):
        assert any(any(row_value(cb, r, c) is None for c in names) for r in rows)
        vals = half(distinct_keys(cb, rows, names))
        with rd.key_set(names, vals) as ks:
            for neg in ((0, 1) if len(names) == 1 else (0,)):
                exp = _kept_rows(cb, rows, [], [(names, vals, neg)])
                flt = F.NotInSet(ks) if neg else F.InSet(ks)
                for b in (rd.read(raw, filters=[flt]), rd.decode(raw, filters=[flt])):
                    assert b.unhandled_filters == [] and b.to_rows() == exp
                assert 0 < len(exp) < len(rows)
    rd.close()


def test_selection_with_seg_id_levels(narrow):  # noqa: F811
    """RDW_NARROW through select (Record_Id, Seg_Id0 / Seg_Id1 from seg_state): ids and state survive the keyed filter."""
    rd, p, raw, rows = narrow
    cb = rd.copybook
    by_id = {r["Record_Id"]: r for r in rows}
    for names in (["TAXPAYER-NUM"], ["SEGMENT-ID", "TAXPAYER-TYPE"], ["COMPANY-ID"]):
        vals = half(distinct_keys(cb, rows, names))
        with rd.key_set(names, vals) as ks:
            for plain in ([], [F.EqualTo("SEGMENT-ID", "C")]):
                b = rd.read(raw, filters=plain + [F.InSet(ks)])
                got = b.to_rows()
                exp = _kept_rows(cb, rows, plain, [(names, vals, 0)])
                assert b.unhandled_filters == [] and got == exp and 0 < len(exp) < len(rows), names
                assert all(by_id[g["Record_Id"]]["Seg_Id0"] == g["Seg_Id0"] and by_id[g["Record_Id"]]["Seg_Id1"] == g["Seg_Id1"]
                           for g in got)
            # framed records are refused on a reader with segment id levels, as by the plain filter
            with pytest.raises(N.CbxError) as e:
                rd.decode(raw, filters=[F.InSet(ks)])
            assert e.value.code == N.CBX_E_ARGUMENT and "select" in str(e.value)
    # NOT IN keeps no record whose key is in the inactive redefine
    vals = half(distinct_keys(cb, rows, ["TAXPAYER-NUM"]))
    with rd.key_set(["TAXPAYER-NUM"], vals) as ks:
        got = rd.read(raw, filters=[F.Not(F.InSet(ks))]).to_rows()
        assert got == _kept_rows(cb, rows, [], [(["TAXPAYER-NUM"], vals, 1)]) and all(g["STATIC_DETAILS"] is not None for g in got)


# ---------------------------------------------------------------------------------------------
# End to end: read, aggregate, aggregate_by, top_n; the distinct keys of one file as the set of another
# ---------------------------------------------------------------------------------------------
AGGS = [A.CountStar()] + [fn(c) for c in ("AMT-01", "ACCT-NO", "ZD-01") for fn in ALL_FUNCS] + [A.Count("NAME")]


def test_aggregate_group_and_top_n_take_set_filters(syn):
    rd, data, rows, t = syn
    cb = rd.copybook
    vals = half(distinct_keys(cb, rows, ["BR-ID", "NAME"]))
    with rd.key_set(["BR-ID", "NAME"], vals) as ks:
        for plain in ([], [F.LessThan("ZD-01", 0)]):
            filters = plain + [F.InSet(ks)]
            kept = _kept_rows(cb, rows, plain, [(["BR-ID", "NAME"], vals, 0)])
            kept_at = np.flatnonzero(expected_set_keep(cb, rows, plain, [(["BR-ID", "NAME"], vals, 0)]))
            assert 0 < len(kept) < len(rows)
            got = rd.aggregate_device(t, len(data), AGGS, filters)
            n_rows, values, _ = expected_aggregates(cb, rd.plan, kept, AGGS)
            assert got.n_rows == n_rows == len(kept) and got.values == values
            grouped = rd.aggregate_by_device(t, len(data), ["BR-ID"], AGGS, filters)
            check_groups(grouped, expected_groups(cb, rd.plan, kept, ["BR-ID"], AGGS), AGGS)
            orders = [S("AMT-01", True), S("NAME")]
            for limit in (1, 10, len(kept) + 1):
                _, chosen = expected_indices(cb, kept, orders, limit)
                b = rd.top_n_device(t, len(data), orders, limit, filters, first_record_id=100)
                assert b.to_rows() == [kept[i] for i in chosen], (plain, limit)
                # the record ids of the source survive the keyed filter's selection and the Top-N over it
                sel = rd._top_n_records(orders, limit, filters, t, len(data), 321, torch.cuda.current_stream(), stride=200,
                                        first_record_id=100)
                assert sel["n"] == len(chosen)
                assert sel["record_id"][:sel["n"]].cpu().tolist() == [100 + int(kept_at[i]) for i in chosen]
                assert sel["rec_off"][:sel["n"]].cpu().tolist() == [200 * int(kept_at[i]) for i in chosen]
        # all or nothing: a set filter the stage cannot push makes the call unhandled
        with pytest.raises(A.Unhandled, match="Or"):
            rd.aggregate_device(t, len(data), AGGS, [F.Or(F.InSet(ks), F.IsNull("QTY-01"))])


def test_semi_join_of_two_files(syn):
    """The distinct (BR-ID, NAME) keys aggregate_by finds in one file, fed as a set to a second file, select exactly the
    joined rows; a null key of the dimension never joins."""
    rd, data, rows, t = syn
    cb = rd.copybook
    dim = data[200 * 40:200 * 150]       # records 40..149 of the fact file
    dim_rows = RO.fixed_len_rows(cb, dim, PARAMS)
    for names in (["BR-ID", "NAME"], ["ZD-01"]):
        keys = list(rd.aggregate_by(dim, names, [A.CountStar()]).groups)
        assert set(keys) == {tuple(row_value(cb, r, c) for c in names) for r in dim_rows}
        with rd.key_set(names, keys) as ks:
            assert ks.has_null == any(None in k for k in keys) and ks.dropped == 0
            dim_keys = {k for k in keys if None not in k}
            exp = [r for r in rows if tuple(row_value(cb, r, c) for c in names) in dim_keys]
            got = rd.decode_device(t, len(data), filters=[F.InSet(ks)]).to_rows()
            assert got == exp and len(exp) >= 110 - sum(None in tuple(row_value(cb, r, c) for c in names) for r in dim_rows)
            if names == ["ZD-01"]:
                assert ks.has_null
                flt = F.NotInSet(ks)
                b = rd.decode_device(t, len(data), filters=[flt])
                assert b.unhandled_filters == [flt] and b.n_rec == len(rows)


# ---------------------------------------------------------------------------------------------
# Error paths
# ---------------------------------------------------------------------------------------------
def _raw_keyed(rd, t, n_bytes, n_rec, handles, negate, n_sets):
    out, cs = rd._empty_selection(n_rec, t.device)
    ns = ctypes.c_int64(-1)
    hs = (ctypes.c_void_p * 8)(*handles)
    ng = (ctypes.c_int32 * 8)(*negate)
    rc = N.load().cbx_filter_records_keyed(rd.native.handle, t.data_ptr(), n_bytes, None, None, None, n_rec, 200, 0, 0, None,
                                           ctypes.addressof(hs), ctypes.addressof(ng), n_sets, ctypes.byref(cs), ctypes.byref(ns),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, N.load().cbx_last_error().decode(), ns.value


def test_c_level_refusals(syn, acct_sets):
    rd, data, rows, t = syn
    one = acct_sets[64][1]
    other = FixedLenNestedReader(SYN200_COPYBOOK, PARAMS)
    with other.key_set(["ACCT-NO"], [1, 2]) as foreign, rd.key_set(["BR-ID", "NAME"], [(1, "A")]) as pair:
        for handles, negate, n_sets, word in (([one.handle], [0], 0, "1 to 4"), ([one.handle] * 5, [0] * 5, 5, "1 to 4"),
                                              ([foreign.handle], [0], 1, "another plan"), ([one.handle, None], [0, 0], 2, "null"),
                                              ([one.handle, pair.handle], [0, 1], 2, "single-column")):
            rc, err, ns = _raw_keyed(rd, t, len(data), 321, handles, negate, n_sets)
            assert rc == N.CBX_E_ARGUMENT and word in err, (n_sets, rc, err)
        assert _raw_keyed(rd, t, len(data), 321, [one.handle, pair.handle], [1, 0], 2)[0] == N.CBX_OK
        rc, err, ns = _raw_keyed(rd, t, len(data), 400, [one.handle], [0], 1)
        assert rc == N.CBX_E_ARGUMENT and "exceed n_bytes" in err
        # the reader refuses the foreign set too (it is handed back), and a closed one outright
        flt = F.InSet(foreign)
        b = rd.decode_device(t, len(data), filters=[flt])
        assert b.unhandled_filters == [flt] and b.n_rec == 321
    assert foreign.closed and pair.closed
    with pytest.raises(ValueError, match="closed"):
        rd.decode_device(t, len(data), filters=[F.InSet(pair)])
    other.close()
    # cbx_key_set_create: what group_build refuses, and the value checks
    L = N.load()
    h = ctypes.c_void_p()
    g = N.CbxGroupBy()
    g.n_keys, g.fields[0] = 1, rd.plan.field_of_node[id(rd.copybook.get_field_by_name("NAME"))]
    v = N.CbxKeyValue(0, 0, 3 * 18 + 1, 0)
    raw = (ctypes.c_uint8 * 54)()
    off = (ctypes.c_int32 * 4)()
    for stride, n, word in ((54, 1, "str_len"), (53, 1, "str_stride"), (54, -1, "negative")):
        rc = L.cbx_key_set_create(rd.native.handle, ctypes.byref(g), ctypes.byref(v), ctypes.addressof(raw), stride,
                                  ctypes.addressof(off), n, None, ctypes.byref(h))
        assert rc == N.CBX_E_ARGUMENT and word in L.cbx_last_error().decode() and not h.value
    g.fields[0] = 999
    assert L.cbx_key_set_create(rd.native.handle, ctypes.byref(g), None, None, 0, None, 0, None, ctypes.byref(h)) == N.CBX_E_ARGUMENT
    with pytest.raises(F.Unhandled, match="COMP-1 / COMP-2 key"):
        rd.key_set(["FX-RATE"], [])


def test_hierarchical_reader_raises():
    opts = {"is_record_sequence": "true", "segment_field": "SEGMENT_ID",
            "redefine_segment_id_map:1": "STATIC-DETAILS => C", "redefine-segment-id-map:2": "CONTACTS => P",
            "segment-children:1": "STATIC-DETAILS => CONTACTS"}
    p, _ = parse_options(opts)
    rd = VarLenNestedReader(RDW_NARROW_COPYBOOK, p)
    assert rd.hierarchical
    from cobrix_amd.synth import rdw_narrow
    raw = rdw_narrow(50, seed=4)[0].numpy().tobytes()
    with rd.key_set(["SEGMENT-ID"], ["C"]) as ks:
        assert isinstance(ks, KeySet)
        with pytest.raises(N.CbxError) as e:
            rd.read(raw, filters=[F.InSet(ks)])
        assert e.value.code == N.CBX_E_UNSUPPORTED
    rd.close()
