// cbx_aggregate.h -- aggregate pushdown (cbx_aggregate_records): COUNT(*), COUNT(col), MIN, MAX and SUM
// computed from the records' bytes, with the row filter of cbx_filter.h fused in front.
//
// What Spark's SupportsPushDownAggregates.pushAggregation hands a data source.  Without it a profiling
// query (row counts, value ranges, control totals) filters, emits a selection, decodes the column into
// HBM and reduces it with another library; here no keep word, selection or column is written:
//   accumulate: one lane per record, 64 records per tile, a grid-stride loop over the tiles.  Per tile
//               filter_keep (when a filter is given), the rows count from the ballot, then per term the
//               field decoded straight from HBM exactly as filter_term_true decodes it, a cross-lane
//               reduction, and a merge into the term's running accumulator, which lane t of the wave
//               owns for term t.  After the loop the workgroup's waves combine through LDS and store
//               one slab [workgroup][term].
//   combine:    one workgroup merges the slabs into the result (a second small launch: there are no
//               128-bit atomics to build min / max from, and the result stays deterministic).
// The accumulator (cbx_aggregate_value) holds count, min and max as signed 128-bit numbers and the sum
// as three 64-bit limbs, 192-bit two's complement: |value| < 2^127 and fewer than 2^63 records, so no
// order of addition overflows and the sum is exact whatever the reduction order.  All limb arithmetic
// is unsigned add-with-carry.
//
// aggregate_build, agg_value, agg_accumulate and agg_merge are host/device: tests/native/aggregate_host.cpp
// runs them on the host (CBX_FILTER_HOST_ONLY leaves the kernels out).  Not part of the hipRTC bundle.
#pragma once

#include "cbx_filter.h"

namespace cbx {

// One term, pre-resolved by the host: the field's descriptor, its fast-path constants, the functions.
struct AggTerm {
    Field f;
    NumOp op;                 // SWAR decoder constants (fast != 0)
    int32_t funcs;            // cbx_aggregate_func bits
    int32_t is_str;           // COUNT only: the null test of a string field
    int32_t fast;             // Variant of the SWAR decoder, 0: byte loop (as FilterTerm)
    int32_t wide;             // a DEC128 column: 128-bit min / max, three-limb tile sum
};
static_assert(sizeof(AggTerm) % 4 == 0, "AggTerm is a dword struct");

struct AggProg {
    int32_t n_terms, reserved[3];
    AggTerm terms[CBX_AGG_MAX_TERMS];
};

// cbx_aggregate + the plan's field table -> AggProg.  Returns CBX_OK, CBX_E_ARGUMENT (malformed table)
// or CBX_E_UNSUPPORTED (a field or function the stage does not evaluate), the reason in err.
inline int aggregate_build(const cbx_field* fields, int32_t n_fields, bool walk_plan, const cbx_aggregate* ag,
                           AggProg* out, std::string& err) {
    if (!ag || ag->n_terms < 0 || ag->n_terms > CBX_AGG_MAX_TERMS) {
        err = "cbx_aggregate: table sizes out of range";
        return CBX_E_ARGUMENT;
    }
    AggProg& P = *out;
    memset(&P, 0, sizeof(P));
    P.n_terms = ag->n_terms;
    const int all = CBX_AGG_COUNT | CBX_AGG_MIN | CBX_AGG_MAX | CBX_AGG_SUM;
    for (int t = 0; t < ag->n_terms; t++) {
        const cbx_aggregate_term& s = ag->terms[t];
        const std::string at = "cbx_aggregate: term " + std::to_string(t) + ": ";
        if (s.field < 0 || s.field >= n_fields) { err = at + "field index out of range"; return CBX_E_ARGUMENT; }
        if (s.funcs == 0 || (s.funcs & ~all)) { err = at + "empty or unknown function mask"; return CBX_E_ARGUMENT; }
        for (int u = 0; u < t; u++)
            if (ag->terms[u].field == s.field) { err = at + "field repeated (one term holds all its functions)"; return CBX_E_ARGUMENT; }
        const cbx_field& cf = fields[s.field];
        if (walk_plan) { err = at + "record-walk plan: fields lie at data-dependent offsets"; return CBX_E_UNSUPPORTED; }
        if (cf.n_dims > 0) { err = at + "field inside an OCCURS"; return CBX_E_UNSUPPORTED; }
        const bool reduces = (s.funcs & ~CBX_AGG_COUNT) != 0;
        bool is_str = false;
        switch (cf.kind) {
        case CBX_K_STRING: case CBX_K_STRING_ASCII:
            if (reduces) { err = at + "MIN, MAX or SUM on a string field"; return CBX_E_UNSUPPORTED; }
            is_str = true;
            break;
        case CBX_K_BCD: case CBX_K_BINARY: case CBX_K_ZONED: case CBX_K_ASCII_NUM: break;
        case CBX_K_FLOAT: case CBX_K_DOUBLE:
            if (reduces) { err = at + "MIN, MAX or SUM on a COMP-1 / COMP-2 field"; return CBX_E_UNSUPPORTED; }
            break;
        case CBX_K_HEX: case CBX_K_RAW: case CBX_K_UTF16_BE: case CBX_K_UTF16_LE:
            err = at + "UTF-16, HEX and RAW fields are not aggregated on the GPU";
            return CBX_E_UNSUPPORTED;
        default:
            err = at + "generated columns are not aggregated on the GPU";
            return CBX_E_UNSUPPORTED;
        }
        AggTerm& d = P.terms[t];
        d.f = make_field(cf);
        d.op = make_numop(d.f, 0, cf.offset, nullptr, nullptr, 0);
        d.funcs = s.funcs;
        d.is_str = is_str;
        const int v = d.f.variant;
        d.fast = (v == V_BCD8 || v == V_BCD16 || v == V_BIN8 || v == V_ZONED16) ? v : 0;
        d.wide = cf.out_type == CBX_O_DEC128;
    }
    return CBX_OK;
}

// The term's field of the record at rec (avail bytes, decoded at +start_off, active segment seg; head:
// bytes readable in front of rec): false where filter_term_true finds it null -- an inactive segment, a
// numeric reaching past the record's end, a string starting past it, a malformed value -- else the
// column's output value (flt_widen) in (hi, lo).  The decoders and their order are filter_term_true's.
CBX_HD bool agg_value(const AggTerm& tm, const uint8_t* rec, int avail, int64_t head, int start_off, int seg,
                      int64_t& hi, uint64_t& lo) {
    const Field& f = tm.f;
    const bool seg_ok = f.segment < 0 || f.segment == seg;
    const int o = start_off + f.offset;
    hi = 0; lo = 0;
    if (tm.is_str) return seg_ok && o <= avail;
    if (!(seg_ok && o + f.size <= avail)) return false;
    const uint8_t* p = rec + o;
    Val v = null_val();
    bool defer = true;
    if (tm.fast && head + o + f.size >= 16) {
        defer = false;
        const uint64_t r1 = flt_le64(p + f.size - 8);
        switch (tm.fast) {
        case V_BCD8: v = bcd8_raw<0>(tm.op, r1); break;
        case V_BCD16: v = bcd16_raw<0>(tm.op, r1, flt_le64(p + f.size - 16)); break;
        case V_BIN8: v = bin8_raw<0>(tm.op, r1); break;
        default: v = zoned16_raw<0>(tm.op, r1, flt_le64(p + f.size - 16), defer); break;
        }
    }
    if (defer) v = decode_numeric(f, p);
    if (!v.valid) return false;
    if (f.kind == CBX_K_FLOAT || f.kind == CBX_K_DOUBLE) return true;   // COUNT only
    flt_widen(v, f.out_type, hi, lo);
    return true;
}

// a += b over 192-bit two's complement numbers (three unsigned limbs, add with carry)
CBX_HD void agg_add192(uint64_t* a, const uint64_t* b) {
    const uint64_t s0 = a[0] + b[0];
    const uint64_t c0 = s0 < a[0] ? 1u : 0u;
    const uint64_t t1 = a[1] + b[1];
    const uint64_t c1 = t1 < a[1] ? 1u : 0u;
    const uint64_t s1 = t1 + c0;
    const uint64_t c2 = s1 < t1 ? 1u : 0u;
    a[0] = s0; a[1] = s1; a[2] = a[2] + b[2] + c1 + c2;
}

// a <- a merged with b: associative and commutative; an accumulator without a value (count 0) is all zeros.
CBX_HD void agg_merge(cbx_aggregate_value& a, const cbx_aggregate_value& b) {
    if (b.count == 0) return;
    if (a.count == 0) { a = b; return; }
    a.count += b.count;
    if (flt_cmp128((int64_t)b.min_hi, b.min_lo, (int64_t)a.min_hi, a.min_lo) < 0) { a.min_hi = b.min_hi; a.min_lo = b.min_lo; }
    if (flt_cmp128((int64_t)b.max_hi, b.max_lo, (int64_t)a.max_hi, a.max_lo) > 0) { a.max_hi = b.max_hi; a.max_lo = b.max_lo; }
    agg_add192(a.sum, b.sum);
}

// One value into the accumulator: count always (min / max / sum mean nothing without it), the others as
// the term's function mask asks (zero otherwise).
CBX_HD void agg_accumulate(cbx_aggregate_value& acc, const AggTerm& tm, bool valid, int64_t hi, uint64_t lo) {
    if (!valid) return;
    cbx_aggregate_value one;
    one.count = 1;
    const bool mn = (tm.funcs & CBX_AGG_MIN) != 0, mx = (tm.funcs & CBX_AGG_MAX) != 0, sm = (tm.funcs & CBX_AGG_SUM) != 0;
    one.min_lo = mn ? lo : 0; one.min_hi = mn ? (uint64_t)hi : 0;
    one.max_lo = mx ? lo : 0; one.max_hi = mx ? (uint64_t)hi : 0;
    one.sum[0] = sm ? lo : 0; one.sum[1] = sm ? (uint64_t)hi : 0; one.sum[2] = sm ? (uint64_t)(hi >> 63) : 0;
    agg_merge(acc, one);
}

#ifndef CBX_FILTER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernels (included by cbx_capi.hip after cbx_filter.h)
// ------------------------------------------------------------------------------------------
constexpr int kAggThreads = 256;          // 4 waves = 4 tiles per workgroup and round
constexpr int kAggWaves = kAggThreads / 64;
constexpr int kAggCombineThreads = 512;   // 32 parts x 16 terms
constexpr int kAggCombineParts = kAggCombineThreads / CBX_AGG_MAX_TERMS;

struct AggArgs {
    FilterArgs src;                        // the three sources of the filter stage (keep / counts / seg_out unused)
    const CBX_CONST AggProg* agg;
    int32_t has_filter, reserved;
    cbx_aggregate_result* slabs;           // [gridDim.x]: one partial result per workgroup
};

__device__ __forceinline__ uint64_t agg_xor64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// The tile's accumulator of one term, the same in every lane: xor butterflies over the 64 lanes.  Lanes
// without a value carry the identity of each function; n_valid > 0.  A 64-bit column (wide == 0, hi is
// lo's sign) reduces min / max on 64 bits and its sum on two limbs -- 64 values of 64 bits fit 70.
__device__ __forceinline__ cbx_aggregate_value agg_tile_reduce(int funcs, int wide, bool valid, int64_t hi, uint64_t lo,
                                                               int n_valid) {
    cbx_aggregate_value r;
    r.count = n_valid;
    r.min_lo = r.min_hi = r.max_lo = r.max_hi = 0;
    r.sum[0] = r.sum[1] = r.sum[2] = 0;
    if (wide) {
        if (funcs & CBX_AGG_MIN) {
            int64_t h = valid ? hi : INT64_MAX;
            uint64_t l = valid ? lo : ~0ull;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const int64_t oh = (int64_t)agg_xor64((uint64_t)h, m);
                const uint64_t ol = agg_xor64(l, m);
                if (flt_cmp128(oh, ol, h, l) < 0) { h = oh; l = ol; }
            }
            r.min_hi = (uint64_t)h; r.min_lo = l;
        }
        if (funcs & CBX_AGG_MAX) {
            int64_t h = valid ? hi : INT64_MIN;
            uint64_t l = valid ? lo : 0ull;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const int64_t oh = (int64_t)agg_xor64((uint64_t)h, m);
                const uint64_t ol = agg_xor64(l, m);
                if (flt_cmp128(oh, ol, h, l) > 0) { h = oh; l = ol; }
            }
            r.max_hi = (uint64_t)h; r.max_lo = l;
        }
        if (funcs & CBX_AGG_SUM) {
            uint64_t s[3] = {valid ? lo : 0ull, valid ? (uint64_t)hi : 0ull, valid ? (uint64_t)(hi >> 63) : 0ull};
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const uint64_t o[3] = {agg_xor64(s[0], m), agg_xor64(s[1], m), agg_xor64(s[2], m)};
                agg_add192(s, o);
            }
            r.sum[0] = s[0]; r.sum[1] = s[1]; r.sum[2] = s[2];
        }
        return r;
    }
    if (funcs & CBX_AGG_MIN) {
        int64_t x = valid ? (int64_t)lo : INT64_MAX;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int64_t o = (int64_t)agg_xor64((uint64_t)x, m);
            x = o < x ? o : x;
        }
        r.min_lo = (uint64_t)x; r.min_hi = (uint64_t)(x >> 63);
    }
    if (funcs & CBX_AGG_MAX) {
        int64_t x = valid ? (int64_t)lo : INT64_MIN;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int64_t o = (int64_t)agg_xor64((uint64_t)x, m);
            x = o > x ? o : x;
        }
        r.max_lo = (uint64_t)x; r.max_hi = (uint64_t)(x >> 63);
    }
    if (funcs & CBX_AGG_SUM) {
        uint64_t s0 = valid ? lo : 0ull, s1 = valid ? (uint64_t)hi : 0ull;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint64_t o0 = agg_xor64(s0, m), o1 = agg_xor64(s1, m);
            const uint64_t t = s0 + o0;
            s1 = s1 + o1 + (t < s0 ? 1u : 0u);
            s0 = t;
        }
        r.sum[0] = s0; r.sum[1] = s1; r.sum[2] = (uint64_t)((int64_t)s1 >> 63);
    }
    return r;
}

// Every lane loads its terms' field bytes straight from HBM, as filter_test_kernel does (a staged tile
// measured 3.5 times slower there for this access pattern).  Waves never leave before the last barrier.
__global__ __launch_bounds__(kAggThreads) void aggregate_kernel(AggArgs g) {
    __shared__ uint32_t s_lut[256];
    __shared__ uint8_t s_pool[CBX_FILTER_POOL_BYTES];
    __shared__ cbx_aggregate_value s_acc[kAggWaves][CBX_AGG_MAX_TERMS];
    __shared__ int64_t s_rows[kAggWaves];
    const FilterArgs& a = g.src;
    for (int i = threadIdx.x; i < 256; i += kAggThreads) s_lut[i] = a.lut[i];
    if (g.has_filter) {
        const CBX_CONST uint32_t* pw = (const CBX_CONST uint32_t*)a.prog->pool;
        for (int i = threadIdx.x; i < CBX_FILTER_POOL_BYTES / 4; i += kAggThreads) ((uint32_t*)s_pool)[i] = pw[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = g.agg->n_terms;
    cbx_aggregate_value acc;   // lane t: term t's running accumulator of this wave
    acc.count = 0;
    acc.min_lo = acc.min_hi = acc.max_lo = acc.max_hi = 0;
    acc.sum[0] = acc.sum[1] = acc.sum[2] = 0;
    int64_t rows = 0;
    for (int64_t tile = (int64_t)blockIdx.x * kAggWaves + wave; tile < a.n_tiles; tile += (int64_t)gridDim.x * kAggWaves) {
        const int64_t i = tile * 64 + lane;
        bool keep = false;
        const uint8_t* rec = a.data;
        int avail = 0, seg = -1;
        int64_t off = 0;
        if (i < a.n) {
            avail = flt_record(a, i, off);
            rec = a.data + off;
            if (nt > 0 || g.has_filter) {   // (COUNT(*) of unfiltered records reads no record byte)
                if (a.rec_seg) seg = a.rec_seg[i];
                else if (a.segmap) seg = flt_segment(a, s_lut, rec, avail);
            }
            keep = true;
            if (g.has_filter) {
                FilterDevTab tab{a.prog};
                keep = filter_keep(tab, s_pool, rec, avail, off, a.start_off, seg, [&](uint32_t b) -> uint32_t { return s_lut[b]; });
            }
        }
        const uint64_t m = __ballot(keep);
        rows += __popcll(m);
        if (m == 0) continue;
        for (int t = 0; t < nt; t++) {
            const AggTerm tm = ldc(&g.agg->terms[t]);
            int64_t hi = 0;
            uint64_t lo = 0;
            bool valid = false;
            if (keep) valid = agg_value(tm, rec, avail, off, a.start_off, seg, hi, lo);
            const uint64_t vm = __ballot(valid);
            if (vm == 0) continue;
            const cbx_aggregate_value tv = agg_tile_reduce(tm.funcs, tm.wide, valid, hi, lo, __popcll(vm));
            if (lane == t) agg_merge(acc, tv);
        }
    }
    if (lane < CBX_AGG_MAX_TERMS) s_acc[wave][lane] = acc;
    if (lane == 0) s_rows[wave] = rows;
    __syncthreads();
    if (threadIdx.x < CBX_AGG_MAX_TERMS) {
        cbx_aggregate_value r = s_acc[0][threadIdx.x];
        for (int w = 1; w < kAggWaves; w++) agg_merge(r, s_acc[w][threadIdx.x]);
        g.slabs[blockIdx.x].values[threadIdx.x] = r;
        if (threadIdx.x == 0) {
            int64_t n = 0;
            for (int w = 0; w < kAggWaves; w++) n += s_rows[w];
            g.slabs[blockIdx.x].n_rows = n;
        }
    }
}

// One workgroup: thread (part, term) merges the slabs part, part + kAggCombineParts, ..; the parts meet in LDS.
__global__ __launch_bounds__(kAggCombineThreads) void aggregate_combine_kernel(const cbx_aggregate_result* slabs, int32_t n_slabs,
                                                                               cbx_aggregate_result* out) {
    __shared__ cbx_aggregate_value s_v[kAggCombineParts][CBX_AGG_MAX_TERMS];
    __shared__ int64_t s_n[kAggCombineParts];
    const int term = threadIdx.x % CBX_AGG_MAX_TERMS, part = threadIdx.x / CBX_AGG_MAX_TERMS;
    cbx_aggregate_value acc;
    acc.count = 0;
    acc.min_lo = acc.min_hi = acc.max_lo = acc.max_hi = 0;
    acc.sum[0] = acc.sum[1] = acc.sum[2] = 0;
    int64_t rows = 0;
    for (int w = part; w < n_slabs; w += kAggCombineParts) {
        agg_merge(acc, slabs[w].values[term]);
        if (term == 0) rows += slabs[w].n_rows;
    }
    s_v[part][term] = acc;
    if (term == 0) s_n[part] = rows;
    __syncthreads();
    if (threadIdx.x < CBX_AGG_MAX_TERMS) {
        cbx_aggregate_value r = s_v[0][threadIdx.x];
        for (int p = 1; p < kAggCombineParts; p++) agg_merge(r, s_v[p][threadIdx.x]);
        out->values[threadIdx.x] = r;
        if (threadIdx.x == 0) {
            int64_t n = 0;
            for (int p = 0; p < kAggCombineParts; p++) n += s_n[p];
            out->n_rows = n;
        }
    }
}
#endif   // CBX_FILTER_HOST_ONLY

}  // namespace cbx
