// cbx_group.h -- grouped aggregates (cbx_aggregate_grouped): GROUP BY up to four key fields, COUNT(*) and the
// terms of cbx_aggregate.h per distinct key, computed from the records' bytes with the row filter fused in.
//
// Table: open addressing with linear probing over `capacity` slots (the power of two >= 2 * max_groups).  A
// slot is one 64-bit word and its accumulators.  The word is 0 (empty) or the index + 1 of a representative
// record, and THE SLOT'S KEY IS DEFINED AS THE KEY OF THAT RECORD: the input is immutable, so nothing else
// has to be published.  A prober that meets a non-empty slot decodes the representative's key fields from
// the input and compares them with its own; an empty slot is claimed with one device-scope 64-bit
// compare-and-swap, and when that fails the word it returns is the winner's representative -- compare and
// go on.  There is no "being written" state, no flag, no fence and no wait: no loop here depends on a store
// of another lane, and every probe loop is bounded by the capacity.
//   init:       slot words 0, accumulators at their identities (min INT64_MAX, max INT64_MIN, the rest 0).
//   accumulate: one lane per record, 64 records per tile, grid-stride as aggregate_kernel.  Each kept lane
//               finds or claims its slot; the wave then walks the distinct slot ids of the tile (up to
//               kGrpTileIds, compared as 32-bit ids), reduces the members' values of each term with the
//               butterflies of agg_tile_reduce and merges them into a wave-private, direct-mapped LDS cache
//               of running accumulators (lane t owns term t; no wave shares an entry, so the loop has no
//               barrier).  A conflict flushes the resident entry to the slot's global accumulators with
//               device-scope 64-bit atomics, the loop's end flushes them all; lanes past the id bound and
//               ids whose entry another id of the same tile holds flush their single values directly.
//   emit:       one lane per slot; an occupied slot takes a dense index, decodes the representative's key
//               into the output cell and widens the accumulators to cbx_aggregate_value.
// MIN / MAX are signed 64-bit atomics (a DEC128 column takes COUNT and SUM only); the 192-bit sum is three
// 64-bit atomic adds that return the old limb, the carry out of a limb computed from it and added into the
// next -- every limb ends as the sum of what was added to it modulo 2^64 and every wrap is counted once, so
// the result is exact whatever the order.
//
// group_build, the key hash, the key comparison, find-or-claim and the limb-carry add are host/device:
// tests/native/group_host.cpp runs them on the host (CBX_FILTER_HOST_ONLY leaves the kernels out).
#pragma once

#include "cbx_aggregate.h"

namespace cbx {

struct GrpProg {
    int32_t n_keys, reserved[3];
    AggTerm keys[CBX_GROUP_MAX_KEYS];      // funcs unused; is_str / fast / wide as for a term
};

// A slot's accumulator of one term (64 bytes: one per cache line pair, limbs never straddle a line).
struct GrpAcc {
    int64_t count, mn, mx;
    uint64_t sum[3];
    uint64_t pad[2];
};
static_assert(sizeof(GrpAcc) == 64, "GrpAcc is 64 bytes");

// One record of the source: its bytes, what may be read in front of them, its active segment.
struct GrpRec {
    const uint8_t* rec;
    int avail;
    int64_t head;
    int seg;
};

// A numeric key's value (null: hi = lo = 0).
struct GrpKeyVal {
    int64_t hi;
    uint64_t lo;
    int32_t null;
};

struct GrpHostTab {
    const GrpProg* p;
    CBX_HD int n_keys() const { return p->n_keys; }
    CBX_HD AggTerm key(int k) const { return p->keys[k]; }
};

// cbx_group_by + the plan's field table (+ the built terms) -> GrpProg.  Status and reason as aggregate_build.
inline int group_build(const cbx_field* fields, int32_t n_fields, bool walk_plan, const cbx_group_by* gb,
                       const AggProg& agg, GrpProg* out, std::string& err) {
    if (!gb || gb->n_keys < 1 || gb->n_keys > CBX_GROUP_MAX_KEYS) {
        err = "cbx_group_by: 1 to " + std::to_string(CBX_GROUP_MAX_KEYS) + " key fields";
        return CBX_E_ARGUMENT;
    }
    GrpProg& P = *out;
    memset(&P, 0, sizeof(P));
    P.n_keys = gb->n_keys;
    for (int k = 0; k < gb->n_keys; k++) {
        const int fi = gb->fields[k];
        const std::string at = "cbx_group_by: key " + std::to_string(k) + ": ";
        if (fi < 0 || fi >= n_fields) { err = at + "field index out of range"; return CBX_E_ARGUMENT; }
        for (int u = 0; u < k; u++)
            if (gb->fields[u] == fi) { err = at + "field repeated"; return CBX_E_ARGUMENT; }
        const cbx_field& cf = fields[fi];
        if (walk_plan) { err = at + "record-walk plan: fields lie at data-dependent offsets"; return CBX_E_UNSUPPORTED; }
        if (cf.n_dims > 0) { err = at + "field inside an OCCURS"; return CBX_E_UNSUPPORTED; }
        bool is_str = false;
        switch (cf.kind) {
        case CBX_K_STRING: case CBX_K_STRING_ASCII:
            if (cf.size > kFltRegBytes) {
                err = at + "string key longer than " + std::to_string(kFltRegBytes) + " bytes";
                return CBX_E_UNSUPPORTED;
            }
            is_str = true;
            break;
        case CBX_K_BCD: case CBX_K_BINARY: case CBX_K_ZONED: case CBX_K_ASCII_NUM: break;
        case CBX_K_FLOAT: case CBX_K_DOUBLE:
            err = at + "COMP-1 / COMP-2 key";
            return CBX_E_UNSUPPORTED;
        case CBX_K_HEX: case CBX_K_RAW: case CBX_K_UTF16_BE: case CBX_K_UTF16_LE:
            err = at + "UTF-16, HEX and RAW fields are not grouped on the GPU";
            return CBX_E_UNSUPPORTED;
        default:
            err = at + "generated columns are not grouped on the GPU";
            return CBX_E_UNSUPPORTED;
        }
        AggTerm& d = P.keys[k];
        d.f = make_field(cf);
        d.op = make_numop(d.f, 0, cf.offset, nullptr, nullptr, 0);
        d.funcs = 0;
        d.is_str = is_str;
        const int v = d.f.variant;
        d.fast = (v == V_BCD8 || v == V_BCD16 || v == V_BIN8 || v == V_ZONED16) ? v : 0;
        d.wide = cf.out_type == CBX_O_DEC128;
    }
    for (int t = 0; t < agg.n_terms; t++)
        if (agg.terms[t].wide && (agg.terms[t].funcs & (CBX_AGG_MIN | CBX_AGG_MAX))) {
            err = "cbx_aggregate: term " + std::to_string(t) + ": MIN or MAX of a DEC128 column under GROUP BY (no 128-bit atomic)";
            return CBX_E_UNSUPPORTED;
        }
    return CBX_OK;
}

// Strides of the output's string area and the table's capacity; CBX_E_ARGUMENT (reason in err) when max_groups
// or the workspace is out of range.
inline int group_strides(const cbx_field* fields, const cbx_group_by* gb, int32_t n_terms, int64_t max_groups,
                         cbx_group_strides* s, std::string& err) {
    memset(s, 0, sizeof(*s));
    if (max_groups < 1) { err = "cbx_aggregate_grouped: max_groups must be at least 1"; return CBX_E_ARGUMENT; }
    int32_t off = 0;
    for (int k = 0; k < gb->n_keys; k++) {
        const cbx_field& cf = fields[gb->fields[k]];
        s->str_off[k] = off;
        if (cf.kind == CBX_K_STRING || cf.kind == CBX_K_STRING_ASCII) off += 3 * cf.size;
    }
    s->str_stride = off;
    const int64_t limit = CBX_GROUP_MAX_WORKSPACE_BYTES;
    const int64_t per_slot = 16 + 64 * (int64_t)n_terms;
    const int64_t per_group = 8 + (int64_t)sizeof(cbx_aggregate_value) * n_terms + (int64_t)sizeof(cbx_group_key) * gb->n_keys + off;
    if (max_groups > limit / 2 / per_slot || max_groups > limit / per_group) {
        err = "cbx_aggregate_grouped: max_groups needs a workspace above " + std::to_string(limit) + " bytes";
        return CBX_E_ARGUMENT;
    }
    int64_t cap = 2;
    while (cap < 2 * max_groups) cap <<= 1;
    s->capacity = cap;
    s->workspace_bytes = cap * per_slot + max_groups * per_group + 4096;
    if (s->workspace_bytes > limit) {
        err = "cbx_aggregate_grouped: max_groups needs a workspace above " + std::to_string(limit) + " bytes";
        return CBX_E_ARGUMENT;
    }
    return CBX_OK;
}

CBX_HD uint64_t grp_mix(uint64_t h, uint64_t v) {
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

template <typename LutFn>
CBX_HD uint32_t grp_lut(int kind, LutFn lut, uint32_t b) {
    return kind == CBX_K_STRING_ASCII ? ascii_lut(b) : lut(b);
}

// A string key of record r: false where it is null (an inactive segment, a start past the record's end), else
// the field's bytes in registers and the trimmed span.
template <typename LutFn>
CBX_HD bool grp_str_load(const AggTerm& k, const GrpRec& r, int start_off, LutFn lut, FltBytes& b, StrSpan& s) {
    const Field& f = k.f;
    const bool seg_ok = f.segment < 0 || f.segment == r.seg;
    const int o = start_off + f.offset;
    s = StrSpan{0, 0, 0};
    if (!(seg_ok && o <= r.avail)) return false;
    const int n = f.size < r.avail - o ? f.size : r.avail - o;
    b = flt_load_bytes(r.rec + o, n, f.size, r.head + o);
    const int kind = f.kind;
    s = flt_trim_span(f.trim, b, n, [&](uint32_t x) -> uint32_t { return grp_lut(kind, lut, x); });
    return true;
}

// Do the two spans decode to the same UTF-8 bytes?  Both stream through the code page as flt_str_cmp does.
template <typename LutFn>
CBX_HD bool grp_str_eq(int kind, const FltBytes& a, const StrSpan& sa, const FltBytes& b, const StrSpan& sb, LutFn lut) {
    int ia = sa.begin, ib = sb.begin, la = 0, lb = 0;
    uint32_t ea = 0, eb = 0;
    for (int step = 0; step <= 3 * kFltRegBytes; step++) {
        while (la == 0 && ia < sa.end) { ea = grp_lut(kind, lut, a[ia++]); la = (int)((ea >> 24) & 3); }
        while (lb == 0 && ib < sb.end) { eb = grp_lut(kind, lut, b[ib++]); lb = (int)((eb >> 24) & 3); }
        if (la == 0 || lb == 0) return la == lb;
        if ((ea & 0xFFu) != (eb & 0xFFu)) return false;
        ea >>= 8; eb >>= 8; la--; lb--;
    }
    return false;   // (not reached: a span yields at most 3 * kFltRegBytes bytes)
}

// One key field of record r into the running hash h; kv receives a numeric key's value for the comparisons.
template <typename LutFn>
CBX_HD uint64_t grp_hash_one(const AggTerm& tm, const GrpRec& r, int start_off, LutFn lut, uint64_t h, GrpKeyVal& kv) {
    kv = GrpKeyVal{0, 0, 1};
    if (tm.is_str) {
        FltBytes b;
        StrSpan s;
        if (!grp_str_load(tm, r, start_off, lut, b, s)) return grp_mix(h, 0x6E756C6Cull);
        kv.null = 0;
        uint64_t g = 0xCBF29CE484222325ull, len = 0;
        for (int i = s.begin; i < s.end; i++) {
            uint32_t e = grp_lut(tm.f.kind, lut, b[i]);
            for (int l = (int)((e >> 24) & 3); l > 0; l--) { g = (g ^ (e & 0xFFu)) * 0x100000001B3ull; e >>= 8; len++; }
        }
        return grp_mix(grp_mix(h, g), len + 1);
    }
    int64_t hi;
    uint64_t lo;
    if (!agg_value(tm, r.rec, r.avail, r.head, start_off, r.seg, hi, lo)) return grp_mix(h, 0x6E756C6Cull);
    kv = GrpKeyVal{hi, lo, 0};
    return grp_mix(grp_mix(h, lo), (uint64_t)hi + 2);
}

// The hash of record r's key (the keys written out one by one: kv stays in registers).
template <typename Tab, typename LutFn>
CBX_HD uint64_t grp_key_hash(const Tab& tab, const GrpRec& r, int start_off, LutFn lut, GrpKeyVal* kv) {
    static_assert(CBX_GROUP_MAX_KEYS == 4, "the keys are written out one by one");
    uint64_t h = 0x243F6A8885A308D3ull;
    const int nk = tab.n_keys();
    kv[1] = kv[2] = kv[3] = GrpKeyVal{0, 0, 1};
    h = grp_hash_one(tab.key(0), r, start_off, lut, h, kv[0]);
    if (nk > 1) h = grp_hash_one(tab.key(1), r, start_off, lut, h, kv[1]);
    if (nk > 2) h = grp_hash_one(tab.key(2), r, start_off, lut, h, kv[2]);
    if (nk > 3) h = grp_hash_one(tab.key(3), r, start_off, lut, h, kv[3]);
    return h ^ (h >> 32);
}

// Is key field tm of record me (a numeric's value in kv) equal to that of record rep?  NULL equals NULL only.
template <typename LutFn>
CBX_HD bool grp_equal_one(const AggTerm& tm, const GrpKeyVal& kv, const GrpRec& me, const GrpRec& rep, int start_off, LutFn lut) {
    if (tm.is_str) {
        FltBytes a, b;
        StrSpan sa, sb;
        const bool va = grp_str_load(tm, me, start_off, lut, a, sa), vb = grp_str_load(tm, rep, start_off, lut, b, sb);
        if (va != vb) return false;
        return !va || grp_str_eq(tm.f.kind, a, sa, b, sb, lut);
    }
    int64_t hi;
    uint64_t lo;
    const bool v = agg_value(tm, rep.rec, rep.avail, rep.head, start_off, rep.seg, hi, lo);
    if (v == (kv.null != 0)) return false;
    return !v || (hi == kv.hi && lo == kv.lo);
}

// Is record me's key (numeric values in kv) the key of record rep?
template <typename Tab, typename LutFn>
CBX_HD bool grp_key_equal(const Tab& tab, const GrpKeyVal* kv, const GrpRec& me, const GrpRec& rep, int start_off, LutFn lut) {
    const int nk = tab.n_keys();
    if (!grp_equal_one(tab.key(0), kv[0], me, rep, start_off, lut)) return false;
    if (nk > 1 && !grp_equal_one(tab.key(1), kv[1], me, rep, start_off, lut)) return false;
    if (nk > 2 && !grp_equal_one(tab.key(2), kv[2], me, rep, start_off, lut)) return false;
    if (nk > 3 && !grp_equal_one(tab.key(3), kv[3], me, rep, start_off, lut)) return false;
    return true;
}

// The slot of record i's key, claimed if the table does not hold it yet; -1 when the record is dropped (the
// overflow flag is up, or the probe sequence is exhausted, which raises it).  Ops: load(p) and cas(p, want)
// (the word found, 0 when the claim succeeded) on slot words, stopped() (the overflow flag), claimed() (one
// more group: raises the flag past max_groups) and exhausted().  src(j) gives record j.
template <typename Tab, typename Src, typename Ops, typename LutFn>
CBX_HD int64_t grp_find_or_claim(const Tab& tab, Src src, Ops& ops, LutFn lut, int start_off, uint64_t* slots,
                                 uint64_t capacity, uint64_t hash, int64_t i, const GrpKeyVal* kv, const GrpRec& me) {
    const uint64_t mask = capacity - 1;
    for (uint64_t p = 0; p < capacity; p++) {
        const uint64_t idx = (hash + p) & mask;
        uint64_t w = ops.load(slots + idx);
        if (w == 0) {
            if (ops.stopped()) return -1;
            w = ops.cas(slots + idx, (uint64_t)i + 1);
            if (w == 0) { ops.claimed(); return (int64_t)idx; }
        }
        const GrpRec rep = src((int64_t)(w - 1));
        if (grp_key_equal(tab, kv, me, rep, start_off, lut)) return (int64_t)idx;
    }
    ops.exhausted();
    return -1;
}

// s += b over 192-bit two's complement numbers with one returning add per limb (add(p, v): the old *p).  The
// carry out of a limb is read off the old value; limb 1 receives b[1] + carry, and where that sum itself
// wraps (b[1] all ones) it is zero and the carry goes straight to limb 2.
template <typename Ops>
CBX_HD void grp_add192(Ops& ops, uint64_t* s, const uint64_t* b) {
    uint64_t c1 = 0, c2 = 0;
    if (b[0]) {
        const uint64_t old = ops.add(s, b[0]);
        c1 = old + b[0] < old ? 1u : 0u;
    }
    const uint64_t b1 = b[1] + c1;
    if (b1 < c1) c2 = 1;
    if (b1) {
        const uint64_t old = ops.add(s + 1, b1);
        c2 += old + b1 < old ? 1u : 0u;
    }
    const uint64_t b2 = b[2] + c2;
    if (b2) ops.add(s + 2, b2);
}

// v (count > 0, identities where a function is not asked for) into the slot's accumulator.
template <typename Ops>
CBX_HD void grp_flush(Ops& ops, GrpAcc* g, const GrpAcc& v, int funcs) {
    if (v.count == 0) return;
    ops.add((uint64_t*)&g->count, (uint64_t)v.count);
    if (funcs & CBX_AGG_MIN) ops.min64(&g->mn, v.mn);
    if (funcs & CBX_AGG_MAX) ops.max64(&g->mx, v.mx);
    if (funcs & CBX_AGG_SUM) grp_add192(ops, g->sum, v.sum);
}

CBX_HD GrpAcc grp_identity() {
    GrpAcc a;
    a.count = 0; a.mn = INT64_MAX; a.mx = INT64_MIN;
    a.sum[0] = a.sum[1] = a.sum[2] = 0;
    a.pad[0] = a.pad[1] = 0;
    return a;
}

// One value as an accumulator (what a lane past the tile's id bound flushes on its own).
CBX_HD GrpAcc grp_single(int64_t hi, uint64_t lo) {
    GrpAcc a = grp_identity();
    a.count = 1; a.mn = a.mx = (int64_t)lo;
    a.sum[0] = lo; a.sum[1] = (uint64_t)hi; a.sum[2] = (uint64_t)(hi >> 63);
    return a;
}

// The slot's accumulator as the ungrouped call reports a term: zero where count == 0 or a function was not asked.
CBX_HD cbx_aggregate_value grp_widen(const GrpAcc& a, int funcs) {
    cbx_aggregate_value r;
    r.count = a.count;
    r.min_lo = r.min_hi = r.max_lo = r.max_hi = 0;
    r.sum[0] = r.sum[1] = r.sum[2] = 0;
    if (a.count == 0) return r;
    if (funcs & CBX_AGG_MIN) { r.min_lo = (uint64_t)a.mn; r.min_hi = (uint64_t)(a.mn >> 63); }
    if (funcs & CBX_AGG_MAX) { r.max_lo = (uint64_t)a.mx; r.max_hi = (uint64_t)(a.mx >> 63); }
    if (funcs & CBX_AGG_SUM) { r.sum[0] = a.sum[0]; r.sum[1] = a.sum[1]; r.sum[2] = a.sum[2]; }
    return r;
}

// The key cells (and string bytes, at bytes + strides.str_off[k]) of record r's key.
template <typename Tab, typename LutFn>
CBX_HD void grp_key_emit(const Tab& tab, const GrpRec& r, int start_off, LutFn lut, const int32_t* str_off,
                         cbx_group_key* cells, uint8_t* bytes) {
    const int nk = tab.n_keys();
    for (int k = 0; k < nk; k++) {
        const AggTerm tm = tab.key(k);
        cbx_group_key c;
        c.lo = c.hi = 0; c.is_null = 1; c.str_len = 0;
        if (tm.is_str) {
            FltBytes b;
            StrSpan s;
            if (grp_str_load(tm, r, start_off, lut, b, s)) {
                c.is_null = 0;
                uint8_t* o = bytes + str_off[k];
                int n = 0;
                for (int i = s.begin; i < s.end; i++) {
                    uint32_t e = grp_lut(tm.f.kind, lut, b[i]);
                    for (int l = (int)((e >> 24) & 3); l > 0; l--) { o[n++] = (uint8_t)(e & 0xFFu); e >>= 8; }
                }
                c.str_len = n;
            }
        } else {
            int64_t hi;
            uint64_t lo;
            if (agg_value(tm, r.rec, r.avail, r.head, start_off, r.seg, hi, lo)) { c.is_null = 0; c.lo = lo; c.hi = (uint64_t)hi; }
        }
        cells[k] = c;
    }
}

#ifndef CBX_FILTER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernels (included by cbx_capi.hip after cbx_aggregate.h)
// ------------------------------------------------------------------------------------------
constexpr int kGrpTileIds = 8;            // distinct slot ids of a tile that go through the cache
constexpr int kGrpCacheWords = 1024;      // 8 KiB of LDS per wave: E entries of (id, n_rows, n_terms x 6 words)
constexpr int kGrpCacheMaxEntries = 128;
constexpr int kGrpRowsLane = 63;          // the lane that owns the entries' n_rows (terms: lane t < 16)
constexpr int kGrpInitThreads = 256;

struct GrpTable {
    uint64_t* slots;      // [capacity] 0 or representative record + 1
    uint64_t* rows;       // [capacity] COUNT(*) of the slot
    GrpAcc* acc;          // [capacity][n_terms]
    uint64_t* hdr;        // [0] slots claimed, [1] overflow, [2] groups emitted
    uint64_t capacity;
    int64_t max_groups;
};

struct GrpArgs {
    AggArgs a;
    const CBX_CONST GrpProg* grp;
    GrpTable t;
};

struct GrpOut {
    int64_t* n_rows;
    cbx_aggregate_value* values;
    cbx_group_key* keys;
    uint8_t* key_bytes;
    int32_t str_stride;
    int32_t str_off[CBX_GROUP_MAX_KEYS];
};

struct GrpDevTab {
    const CBX_CONST GrpProg* p;
    __device__ __forceinline__ int n_keys() const { return p->n_keys; }
    __device__ __forceinline__ AggTerm key(int k) const { return ldc(&p->keys[k]); }
};

// Device-scope, relaxed: a slot word is the only thing a prober depends on, and what it names is immutable input.
struct GrpDevOps {
    uint64_t* hdr;
    int64_t max_groups;
    __device__ __forceinline__ uint64_t load(uint64_t* p) const {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint64_t cas(uint64_t* p, uint64_t want) const {
        uint64_t expected = 0;
        __hip_atomic_compare_exchange_strong(p, &expected, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;   // 0: claimed; else the winner's word
    }
    __device__ __forceinline__ bool stopped() const { return load(hdr + 1) != 0; }
    __device__ __forceinline__ void claimed() const {
        const uint64_t n = __hip_atomic_fetch_add(hdr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        if ((int64_t)n > max_groups) exhausted();
    }
    __device__ __forceinline__ void exhausted() const {
        __hip_atomic_store(hdr + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint64_t add(uint64_t* p, uint64_t v) const {
        return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void min64(int64_t* p, int64_t v) const {
        (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void max64(int64_t* p, int64_t v) const {
        (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// record j of the source with its active segment, as aggregate_kernel takes them
__device__ __forceinline__ GrpRec grp_record(const FilterArgs& a, const uint32_t* s_lut, int64_t j) {
    GrpRec r;
    int64_t off;
    r.avail = flt_record(a, j, off);
    r.rec = a.data + off;
    r.head = off;
    r.seg = -1;
    if (a.rec_seg) r.seg = a.rec_seg[j];
    else if (a.segmap) r.seg = flt_segment(a, s_lut, r.rec, r.avail);
    return r;
}

__global__ __launch_bounds__(kGrpInitThreads) void group_init_kernel(GrpTable t, int32_t n_terms) {
    const uint64_t i = (uint64_t)blockIdx.x * kGrpInitThreads + threadIdx.x;
    if (i < 4) t.hdr[i] = 0;
    if (i >= t.capacity) return;
    t.slots[i] = 0;
    t.rows[i] = 0;
    const GrpAcc id = grp_identity();
    for (int k = 0; k < n_terms; k++) t.acc[i * (uint64_t)n_terms + k] = id;
}

// entries of a wave's cache for n_terms terms: the largest power of two that fits kGrpCacheWords
__host__ __device__ inline int grp_cache_entries(int n_terms) {
    int e = kGrpCacheMaxEntries;
    while (e > 1 && e * (2 + 6 * n_terms) > kGrpCacheWords) e >>= 1;
    return e;
}

// Entry e of this wave's cache goes to the global accumulators of slot `id`: lane t its term, one lane the rows.
__device__ __forceinline__ void grp_cache_flush(const GrpArgs& g, const GrpDevOps& ops, uint64_t* cache, int E, int nt,
                                                int e, int64_t id, int lane) {
    if (lane < nt) {
        const uint64_t* w = cache + 2 * E + (e * nt + lane) * 6;
        GrpAcc v = grp_identity();
        v.count = (int64_t)w[0]; v.mn = (int64_t)w[1]; v.mx = (int64_t)w[2];
        v.sum[0] = w[3]; v.sum[1] = w[4]; v.sum[2] = w[5];
        grp_flush(ops, g.t.acc + (uint64_t)id * nt + lane, v, ldc(&g.a.agg->terms[lane]).funcs);
    }
    if (lane == kGrpRowsLane) {
        const uint64_t r = cache[E + e];
        if (r) ops.add(g.t.rows + id, r);
    }
}

// Whole waves stay in the tile loop together; the only barrier is the one after the LDS tables are filled.
__global__ __launch_bounds__(kAggThreads) void group_accumulate_kernel(GrpArgs g) {
    __shared__ uint32_t s_lut[256];
    __shared__ uint8_t s_pool[CBX_FILTER_POOL_BYTES];
    __shared__ uint64_t s_cache[kAggWaves][kGrpCacheWords];
    __shared__ uint64_t s_mem[kAggWaves][kGrpTileIds];
    __shared__ int32_t s_ent[kAggWaves][kGrpTileIds];
    const FilterArgs& a = g.a.src;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = g.a.agg->n_terms;
    const int E = grp_cache_entries(nt);
    uint64_t* cache = s_cache[wave];
    for (int i = threadIdx.x; i < 256; i += kAggThreads) s_lut[i] = a.lut[i];
    if (g.a.has_filter) {
        const CBX_CONST uint32_t* pw = (const CBX_CONST uint32_t*)a.prog->pool;
        for (int i = threadIdx.x; i < CBX_FILTER_POOL_BYTES / 4; i += kAggThreads) ((uint32_t*)s_pool)[i] = pw[i];
    }
    // Every lane writes every entry id of its wave's cache: from here on a lane reads only what it wrote itself
    // (ids, member words and entry indices are stored by all lanes with one value; term t's words by lane t).
    for (int e = 0; e < E; e++) cache[e] = ~0ull;
    __syncthreads();
    const GrpDevTab tab{g.grp};
    const GrpDevOps ops{g.t.hdr, g.t.max_groups};
    auto lutf = [&](uint32_t b) -> uint32_t { return s_lut[b]; };
    auto src = [&](int64_t j) -> GrpRec { return grp_record(a, s_lut, j); };
    for (int64_t tile = (int64_t)blockIdx.x * kAggWaves + wave; tile < a.n_tiles; tile += (int64_t)gridDim.x * kAggWaves) {
        const int64_t i = tile * 64 + lane;
        bool keep = false;
        GrpRec me{a.data, 0, 0, -1};
        if (i < a.n) {
            me = grp_record(a, s_lut, i);
            keep = true;
            if (g.a.has_filter) {
                FilterDevTab ftab{a.prog};
                keep = filter_keep(ftab, s_pool, me.rec, me.avail, me.head, a.start_off, me.seg, lutf);
            }
        }
        if (__ballot(keep) == 0) continue;
        int32_t sid = -1;
        if (keep) {
            GrpKeyVal kv[CBX_GROUP_MAX_KEYS];
            const uint64_t h = grp_key_hash(tab, me, a.start_off, lutf, kv);
            sid = (int32_t)grp_find_or_claim(tab, src, ops, lutf, a.start_off, g.t.slots, g.t.capacity, h, i, kv, me);
        }
        // the tile's distinct slot ids -> cache entries
        uint64_t remaining = __ballot(sid >= 0);
        int K = 0;
        bool direct = false;
        while (remaining) {
            if (K == kGrpTileIds) { direct |= ((remaining >> lane) & 1) != 0; break; }
            const int leader = __ffsll((unsigned long long)remaining) - 1;
            const int32_t d = __shfl(sid, leader, 64);
            const uint64_t mem = __ballot(sid == d);
            remaining &= ~mem;
            const int e = d & (E - 1);
            const int64_t cur = (int64_t)cache[e];
            if (cur != d) {
                bool clash = false;
                for (int j = 0; j < K; j++) clash |= s_ent[wave][j] == e;
                if (clash) { direct |= sid == d; continue; }   // another id of this tile holds the entry
                if (cur >= 0) grp_cache_flush(g, ops, cache, E, nt, e, cur, lane);
                cache[e] = (uint64_t)(int64_t)d;
                if (lane < nt) {
                    uint64_t* w = cache + 2 * E + (e * nt + lane) * 6;
                    w[0] = 0; w[1] = (uint64_t)INT64_MAX; w[2] = (uint64_t)INT64_MIN; w[3] = w[4] = w[5] = 0;
                }
                if (lane == kGrpRowsLane) cache[E + e] = 0;
            }
            s_ent[wave][K] = e;
            s_mem[wave][K] = mem;
            K++;
        }
        if (lane == kGrpRowsLane)
            for (int j = 0; j < K; j++) cache[E + s_ent[wave][j]] += (uint64_t)__popcll(s_mem[wave][j]);
        if (direct) ops.add(g.t.rows + sid, 1ull);
        for (int t = 0; t < nt; t++) {
            const AggTerm tm = ldc(&g.a.agg->terms[t]);
            int64_t hi = 0;
            uint64_t lo = 0;
            bool valid = false;
            if (sid >= 0) valid = agg_value(tm, me.rec, me.avail, me.head, a.start_off, me.seg, hi, lo);
            if (__ballot(valid) == 0) continue;
            for (int j = 0; j < K; j++) {
                const bool v = valid && ((s_mem[wave][j] >> lane) & 1);
                const uint64_t vm = __ballot(v);
                if (vm == 0) continue;
                const cbx_aggregate_value tv = agg_tile_reduce(tm.funcs, tm.wide, v, hi, lo, __popcll(vm));
                if (lane == t) {
                    uint64_t* w = cache + 2 * E + (s_ent[wave][j] * nt + t) * 6;
                    w[0] += (uint64_t)tv.count;
                    if (tm.funcs & CBX_AGG_MIN) { const int64_t x = (int64_t)tv.min_lo; if (x < (int64_t)w[1]) w[1] = (uint64_t)x; }
                    if (tm.funcs & CBX_AGG_MAX) { const int64_t x = (int64_t)tv.max_lo; if (x > (int64_t)w[2]) w[2] = (uint64_t)x; }
                    if (tm.funcs & CBX_AGG_SUM) agg_add192(w + 3, tv.sum);
                }
            }
            if (direct && valid) grp_flush(ops, g.t.acc + (uint64_t)sid * nt + t, grp_single(hi, lo), tm.funcs);
        }
    }
    for (int e = 0; e < E; e++) {
        const int64_t cur = (int64_t)cache[e];
        if (cur >= 0) grp_cache_flush(g, ops, cache, E, nt, e, cur, lane);
    }
}

// One lane per slot: an occupied slot takes the next dense index (never past max_groups: an overflowing call
// may have claimed more slots than the output holds).
__global__ __launch_bounds__(kAggThreads) void group_emit_kernel(GrpArgs g, GrpOut o) {
    __shared__ uint32_t s_lut[256];
    const FilterArgs& a = g.a.src;
    for (int i = threadIdx.x; i < 256; i += kAggThreads) s_lut[i] = a.lut[i];
    __syncthreads();
    const uint64_t idx = (uint64_t)blockIdx.x * kAggThreads + threadIdx.x;
    if (idx >= g.t.capacity) return;
    const uint64_t w = g.t.slots[idx];
    if (w == 0) return;
    const uint64_t at = __hip_atomic_fetch_add(g.t.hdr + 2, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int64_t)at >= g.t.max_groups) return;
    const int nt = g.a.agg->n_terms;
    o.n_rows[at] = (int64_t)g.t.rows[idx];
    for (int t = 0; t < nt; t++)
        o.values[at * nt + t] = grp_widen(g.t.acc[idx * (uint64_t)nt + t], ldc(&g.a.agg->terms[t]).funcs);
    const GrpDevTab tab{g.grp};
    const GrpRec rep = grp_record(a, s_lut, (int64_t)(w - 1));
    grp_key_emit(tab, rep, a.start_off, [&](uint32_t b) -> uint32_t { return s_lut[b]; }, o.str_off,
                 o.keys + at * (uint64_t)tab.n_keys(), o.key_bytes + at * (uint64_t)o.str_stride);
}
#endif   // CBX_FILTER_HOST_ONLY

}  // namespace cbx
