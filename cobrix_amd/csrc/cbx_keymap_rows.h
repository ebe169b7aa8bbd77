// cbx_keymap_rows.h -- fan-out joins (cbx_key_map_index_rows, cbx_join_records_expand): per-key lists of ALL the
// dimension rows of a key map, and the join stage that emits one output row per (fact row, matching dimension row).
//
// Row lists: rows[row_start[v] .. row_start[v + 1]) are the ordinals of the source rows the source filter keeps whose
// key is value v, ascending.  row_start is the exclusive 64-bit scan of n_rows, so a segment's length is n_rows[v].
//   scan:     scan64_* (three launches, the shape of device_scan over int64 inputs): row_start[n_values + 1].
//   scatter:  keymap_fill_kernel's geometry and probe; a hit at value j takes slot = cursor[j]++ (one relaxed 64-bit
//             atomic add) and stores its ordinal at rows[row_start[j] + slot] -- unless slot >= n_rows[j], which only a
//             source other than the one the map was built from can cause: nothing is written, the lane is counted.
//   sort:     which lane took which slot depends on timing; the ascending order afterwards does not.  Segments of up to
//             kRowsShortMax ordinals are sorted by one lane each (insertion sort in place, in the classify launch);
//             up to kRowsLdsMax by one workgroup through LDS; longer ones by one workgroup in global memory.  Both
//             workgroup paths run the same network, rows_bitonic: a bitonic sorter whose compare-exchanges all point
//             upwards, so a segment of any length is sorted as if padded with +inf to a power of two (pairs that reach
//             past the end are skipped) -- no segment length is refused.
//   check:    one lane per value: cursor[v] == n_rows[v] and rows[row_start[v]] == first_row[v]; mismatches are counted.
//
// Expand: the test pass is keymap_test_kernel itself, handed a map view whose payload arrays are (row_start, n_rows):
// per input record it leaves the start of its member's list (-1: no member) and the list's length.  The uint32 scan of
// the tile counts and fanout_compact_kernel give, per KEPT row k, its input ordinal, its list start and c(k); a 64-bit
// scan over the kept rows (grid sized from n_rec, the count read on the device) gives kept_base[n_kept + 1] and T.
// fanout_emit_kernel runs over T with lane = output row: c(k) >= 1 for every kept row, so kept_base is strictly
// increasing and the 64 outputs of a wave lie in at most 64 consecutive kept rows -- one wave-uniform binary search for
// the wave's first output, one coalesced load of 64 entries of kept_base, then 6 cross-lane steps per lane.  A wave's
// work is bounded by its 64 outputs whatever the fan-out of the rows around it and however many input rows the filter
// dropped.
//
// The placement rule, the cursor check, the sorting network, the in-window locate and the output-row rule are
// host/device: tests/native/fanout_host.cpp runs them on the host (CBX_FILTER_HOST_ONLY leaves the kernels out).  No
// spin, no flag, no fence; every loop is bounded; whole waves leave together after the last barrier.  Not part of the
// hipRTC bundle.
#pragma once

#include "cbx_keymap.h"

namespace cbx {

constexpr int kRowsShortMax = 16;     // longest segment one lane sorts in place
constexpr int kRowsLdsMax = 4096;     // longest segment one workgroup sorts through LDS (32 KiB of int64)
constexpr int kFxThreads = 256;       // outputs per workgroup of the emit pass

// The scatter's placement of source row `ordinal` whose key is value j: false (nothing written) when the member's
// segment is already full or would lie outside the list -- a source other than the map's.  Ops: add(p, v) -> old.
template <typename Ops>
CBX_HD bool km_place(const Ops& ops, const int64_t* row_start, const int64_t* n_rows, uint64_t* cursor, int64_t* rows,
                     int64_t cap, int64_t j, int64_t ordinal) {
    const int64_t slot = (int64_t)ops.add(cursor + j, 1ull);
    const int64_t at = row_start[j] + slot;
    if (slot < 0 || slot >= n_rows[j] || at < 0 || at >= cap) return false;
    rows[at] = ordinal;
    return true;
}

// What the check pass asks of member v once its segment is sorted.
CBX_HD bool km_cursor_ok(int64_t cursor, int64_t n_rows, int64_t first_listed, int64_t first_row) {
    return cursor == n_rows && first_listed == first_row;
}

// Pair t of one step of the sorter: merge size 2^lk, distance 2^lj; lj == lk - 1 is the merge's first step, which
// compares a block's lower half with its upper half mirrored.
CBX_HD void rows_pair(int lk, int lj, int64_t t, int64_t& a, int64_t& b) {
    if (lj == lk - 1) {
        const int64_t blk = (t >> lj) << lk, off = t & ((1ll << lj) - 1);
        a = blk + off;
        b = blk + (1ll << lk) - 1 - off;
    } else {
        a = ((t >> lj) << (lj + 1)) + (t & ((1ll << lj) - 1));
        b = a + (1ll << lj);
    }
}

// m[0 .. n) ascending, by `nthreads` cooperating threads (this one is `tid`); sync() separates the steps.
template <typename Sync>
CBX_HD void rows_bitonic(int64_t* m, int64_t n, int tid, int nthreads, Sync sync) {
    int lp = 0;
    while (lp < 62 && (1ll << lp) < n) lp++;
    const int64_t half = (1ll << lp) >> 1;
    for (int lk = 1; lk <= lp; lk++) {
        for (int lj = lk - 1; lj >= 0; lj--) {
            for (int64_t t = tid; t < half; t += nthreads) {
                int64_t a, b;
                rows_pair(lk, lj, t, a, b);
                if (b < n) {
                    const int64_t x = m[a], y = m[b];
                    if (x > y) { m[a] = y; m[b] = x; }
                }
            }
            sync();
        }
    }
}

// c(r) of a kept row whose member's list holds n_list ordinals (0: no member, which only LEFT keeps).
CBX_HD int64_t fx_count(int32_t join_type, int64_t n_list) { return join_type == CBX_JOIN_LEFT && n_list < 1 ? 1 : n_list; }

// The kept row of output o: the largest k in [0, n_kept) with kept_base[k] <= o (n_kept >= 1; kept_base[0] == 0).
CBX_HD int64_t fx_first_kept(const int64_t* kept_base, int64_t n_kept, int64_t o) {
    int64_t lo = 0, hi = n_kept;
    for (int it = 0; it < 64 && hi - lo > 1; it++) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (kept_base[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// Within a window of 64 strictly increasing bases with get(0) <= o: the largest w with get(w) <= o, in 6 steps.
template <typename Get>
CBX_HD int fx_locate(Get get, int64_t o) {
    int w = 0;
    for (int s = 32; s > 0; s >>= 1)
        if (get(w + s) <= o) w += s;
    return w;
}

// d_match of the q-th output of a kept row whose list starts at `start` (-1: the single row of an unmatched LEFT row).
CBX_HD int64_t fx_match(const int64_t* rows, int64_t n_indexed, int64_t start, int64_t q) {
    const int64_t at = start + q;
    return start >= 0 && at < n_indexed ? rows[at] : -1;
}

// What cbx_join_records_expand refuses beyond km_join_check.
inline int fx_expand_check(bool has_rows, bool has_out, int64_t out_capacity, std::string& err) {
    if (!has_rows) { err = "cbx_join_records_expand: the map has no row lists (cbx_key_map_index_rows)"; return CBX_E_STATE; }
    if (out_capacity < 0 || (!has_out && out_capacity != 0)) {
        err = "cbx_join_records_expand: out_capacity " + std::to_string(out_capacity) + " without output arrays";
        return CBX_E_ARGUMENT;
    }
    return CBX_OK;
}

inline std::string fx_capacity_message(int64_t needed, int64_t capacity) {
    return "cbx_join_records_expand: " + std::to_string(needed) + " output rows exceed out_capacity " + std::to_string(capacity);
}

// What cbx_key_map_index_rows refuses on the host.
inline int km_rows_check(bool has_map, bool same_plan, int64_t n_rec, int64_t map_n_rec, std::string& err) {
    if (!has_map) err = "cbx_key_map_index_rows: map: null";
    else if (!same_plan) err = "cbx_key_map_index_rows: source_plan is not the plan the map was built from";
    else if (n_rec != map_n_rec)
        err = "cbx_key_map_index_rows: " + std::to_string(n_rec) + " source records, the map was built from " + std::to_string(map_n_rec);
    else return CBX_OK;
    return CBX_E_ARGUMENT;
}

constexpr const char* kRowsSourceDiffers = "cbx_key_map_index_rows: source differs from the one the map was built from";

#ifndef CBX_FILTER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernels (included by cbx_capi.hip after cbx_keymap.h)
// ------------------------------------------------------------------------------------------
enum { KR_BAD_SLOTS = 0, KR_MISMATCH = 1, KR_N_LDS = 2, KR_N_GLOBAL = 3, KR_TOTAL = 4, KR_WORDS = 8 };
enum { FX_TOTAL = 0, FX_N_KEPT = 1, FX_MAX_C = 2, FX_WORDS = 8 };

constexpr int kScan64Items = 4;
constexpr int kScan64Tile = kScanBlock * kScan64Items;

// Exclusive scan of n int64 values into out[0 .. n] (out[n] is the total), n read on the device when n_dev is given
// (the grid is then sized from an upper bound and the blocks past n write zeros / nothing).
__global__ __launch_bounds__(kScanBlock) void scan64_reduce_kernel(const int64_t* in, int64_t n_host, const int64_t* n_dev,
                                                                   int64_t* block_sums) {
    __shared__ int64_t s_w[kScanBlock / kWave];
    const int64_t n = n_dev ? *n_dev : n_host;
    const int64_t b0 = (int64_t)blockIdx.x * kScan64Tile + (int64_t)threadIdx.x * kScan64Items;
    int64_t sum = 0;
#pragma unroll
    for (int i = 0; i < kScan64Items; i++) sum += b0 + i < n ? in[b0 + i] : 0;
    int64_t total;
    block_excl_scan64(sum, s_w, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// (the block sums are scanned by scan_block_sums_kernel)
__global__ __launch_bounds__(kScanBlock) void scan64_apply_kernel(const int64_t* in, int64_t n_host, const int64_t* n_dev,
                                                                  const int64_t* block_sums, int64_t* out, uint64_t* total_out) {
    __shared__ int64_t s_w[kScanBlock / kWave];
    const int64_t n = n_dev ? *n_dev : n_host;
    const int64_t b0 = (int64_t)blockIdx.x * kScan64Tile + (int64_t)threadIdx.x * kScan64Items;
    int64_t v[kScan64Items];
    int64_t sum = 0;
#pragma unroll
    for (int i = 0; i < kScan64Items; i++) {
        v[i] = b0 + i < n ? in[b0 + i] : 0;
        sum += v[i];
    }
    int64_t total;
    int64_t ex = block_excl_scan64(sum, s_w, &total) + block_sums[blockIdx.x];
#pragma unroll
    for (int i = 0; i < kScan64Items; i++) {
        if (b0 + i <= n) out[b0 + i] = ex;
        if (b0 + i == n && total_out) { total_out[0] = (uint64_t)ex; total_out[1] = (uint64_t)n; }
        ex += v[i];
    }
}

struct KmRowsArgs {
    FilterArgs a;                       // the source records (keep / counts / seg_out unused)
    const CBX_CONST KmDevMap* map;      // grp: the SOURCE plan's keys
    int32_t has_filter, reserved;
    const int64_t* row_start;           // [n_values + 1]
    uint64_t* cursor;                   // [n_values], zeroed
    int64_t* rows;                      // [cap]
    int64_t cap;
    uint64_t* hdr;                      // KR_*
};

struct KmRowsDevOps {
    __device__ __forceinline__ uint64_t add(uint64_t* p, uint64_t v) const {
        return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// keymap_fill_kernel with km_place in the place of km_update.
__global__ __launch_bounds__(kFltThreads) void keymap_rows_scatter_kernel(KmRowsArgs g) {
    __shared__ uint32_t s_lut[256];
    __shared__ uint8_t s_pool[CBX_FILTER_POOL_BYTES];
    const FilterArgs& a = g.a;
    for (int i = threadIdx.x; i < 256; i += kFltThreads) s_lut[i] = a.lut[i];
    if (g.has_filter) {
        const CBX_CONST uint32_t* pw = (const CBX_CONST uint32_t*)a.prog->pool;
        for (int i = threadIdx.x; i < CBX_FILTER_POOL_BYTES / 4; i += kFltThreads) ((uint32_t*)s_pool)[i] = pw[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const KmRowsDevOps ops;
    const int64_t* n_rows = ldc(&g.map->n_rows);
    auto lutf = [&](uint32_t b) -> uint32_t { return s_lut[b]; };
    for (int64_t tile = (int64_t)blockIdx.x * (kFltThreads / 64) + wave; tile < a.n_tiles;
         tile += (int64_t)gridDim.x * (kFltThreads / 64)) {
        const int64_t i = tile * 64 + lane;
        if (i >= a.n) continue;
        const GrpRec me = grp_record(a, s_lut, i);
        if (g.has_filter) {
            FilterDevTab ftab{a.prog};
            if (!filter_keep(ftab, s_pool, me.rec, me.avail, me.head, a.start_off, me.seg, lutf)) continue;
        }
        const int64_t j = keymap_lookup(g.map, s_lut, me.rec, me.avail, me.head, me.seg, a.start_off);
        if (j >= 0 && !km_place(ops, g.row_start, n_rows, g.cursor, g.rows, g.cap, j, i))
            (void)__hip_atomic_fetch_add(g.hdr + KR_BAD_SLOTS, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One lane per value: short segments are sorted here, the others go to the list of their path.
__global__ __launch_bounds__(256) void keymap_rows_classify_kernel(const int64_t* row_start, int64_t n_values, int64_t* rows,
                                                                   int64_t cap, int64_t* lds_list, int64_t* global_list,
                                                                   uint64_t* hdr) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_values) return;
    const int64_t s = row_start[v], len = row_start[v + 1] - s;
    if (s < 0 || len < 0 || s + len > cap) return;   // (the check pass reports it)
    if (len <= kRowsShortMax) {
        for (int i = 1; i < (int)len; i++) {
            const int64_t x = rows[s + i];
            int p = i;
            for (; p > 0 && rows[s + p - 1] > x; p--) rows[s + p] = rows[s + p - 1];
            rows[s + p] = x;
        }
    } else if (len <= kRowsLdsMax) {
        lds_list[__hip_atomic_fetch_add(hdr + KR_N_LDS, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = v;
    } else {
        global_list[__hip_atomic_fetch_add(hdr + KR_N_GLOBAL, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = v;
    }
}

// One workgroup per listed member (grid-stride over the list, whose length the classify launch left in *n_list).
__global__ __launch_bounds__(256) void keymap_rows_sort_lds_kernel(const int64_t* row_start, const int64_t* list,
                                                                   const uint64_t* n_list, int64_t* rows) {
    __shared__ int64_t s_rows[kRowsLdsMax];
    const int64_t n = (int64_t)*n_list;
    for (int64_t m = blockIdx.x; m < n; m += gridDim.x) {
        const int64_t v = list[m], s = row_start[v];
        int64_t len = row_start[v + 1] - s;
        if (len > kRowsLdsMax) len = kRowsLdsMax;   // (never: the classify launch listed it)
        for (int i = threadIdx.x; i < (int)len; i += 256) s_rows[i] = rows[s + i];
        __syncthreads();
        rows_bitonic(s_rows, len, (int)threadIdx.x, 256, [] { __syncthreads(); });
        for (int i = threadIdx.x; i < (int)len; i += 256) rows[s + i] = s_rows[i];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void keymap_rows_sort_global_kernel(const int64_t* row_start, const int64_t* list,
                                                                      const uint64_t* n_list, int64_t* rows) {
    const int64_t n = (int64_t)*n_list;
    for (int64_t m = blockIdx.x; m < n; m += gridDim.x) {
        const int64_t v = list[m], s = row_start[v];
        rows_bitonic(rows + s, row_start[v + 1] - s, (int)threadIdx.x, 256, [] { __syncthreads(); });
    }
}

__global__ __launch_bounds__(256) void keymap_rows_check_kernel(const int64_t* first_row, const int64_t* n_rows,
                                                                const int64_t* row_start, const uint64_t* cursor,
                                                                const int64_t* rows, int64_t cap, int64_t n_values, uint64_t* hdr) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (v < n_values) {
        const int64_t s = row_start[v];
        bad = s < 0 || s >= cap || !km_cursor_ok((int64_t)cursor[v], n_rows[v], rows[s], first_row[v]);
        if (v == 0) hdr[KR_TOTAL] = (uint64_t)row_start[n_values];
    }
    const uint64_t bm = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && bm)
        (void)__hip_atomic_fetch_add(hdr + KR_MISMATCH, (uint64_t)__popcll(bm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Per kept row, in source order: its input ordinal, the start of its list and c.  keymap_emit_kernel's geometry.
__global__ __launch_bounds__(kFltThreads) void fanout_compact_kernel(const uint64_t* keep, const int64_t* base, int64_t n_tiles,
                                                                     const int64_t* start_tmp, const int64_t* rows_tmp,
                                                                     int32_t join_type, int64_t* kept_ord, int64_t* kept_start,
                                                                     int64_t* kept_c, uint64_t* hdr) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (kFltThreads / 64) + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const uint64_t m = keep[tile];
    int64_t c = 0;
    if ((m >> lane) & 1) {
        const int64_t i = tile * 64 + lane;
        const int64_t k = base[tile] + __popcll(m & ((1ull << lane) - 1ull));
        c = fx_count(join_type, rows_tmp[i]);
        kept_ord[k] = i;
        kept_start[k] = start_tmp[i];
        kept_c[k] = c;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int64_t o = __shfl_xor(c, d, 64);
        c = o > c ? o : c;
    }
    if (lane == 0 && c > 0) (void)__hip_atomic_fetch_max(hdr + FX_MAX_C, (uint64_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct FxEmitArgs {
    FilterArgs a;                  // the fact records (seg_out: the test pass's segments)
    const int64_t* kept_base;      // [n_kept + 1]
    const int64_t* kept_ord;       // [n_kept]
    const int64_t* kept_start;     // [n_kept]
    const int64_t* rows;           // the map's lists
    int64_t n_kept, n_out, n_indexed, first_record_id;
    cbx_selection in, out;
    int32_t has_in, n_state;
    int64_t* d_match;
    int64_t* d_fact_row;           // may be nullptr
};

// Lane = output row.  Every lane of a wave that owns an output stays to the end: the window is read across lanes.
__global__ __launch_bounds__(kFxThreads) void fanout_emit_kernel(FxEmitArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t o = (int64_t)blockIdx.x * kFxThreads + threadIdx.x, o0 = o - lane;
    if (o0 >= g.n_out) return;   // whole waves leave
    const int64_t k0 = fx_first_kept(g.kept_base, g.n_kept, o0);
    const int64_t kw = k0 + lane < g.n_kept ? k0 + lane : g.n_kept;
    const int64_t kb = g.kept_base[kw];
    const int w = fx_locate([&](int x) -> int64_t { return __shfl(kb, x, 64); }, o);
    const int64_t bw = __shfl(kb, w, 64);
    if (o >= g.n_out) return;   // (after the last cross-lane read)
    const int64_t k = k0 + w, q = o - bw;
    const int64_t i = g.kept_ord[k];
    g.d_match[o] = fx_match(g.rows, g.n_indexed, g.kept_start[k], q);
    if (g.d_fact_row) g.d_fact_row[o] = i;
    const FilterArgs& a = g.a;
    if (g.has_in) {
        g.out.rec_off[o] = g.in.rec_off[i];
        g.out.rec_len[o] = g.in.rec_len[i];
        g.out.record_id[o] = g.in.record_id[i];
        g.out.segment[o] = g.in.segment[i];
        if (g.n_state > 0 && g.in.seg_state && g.out.seg_state)
            for (int l = 0; l < g.n_state; l++) g.out.seg_state[o * g.n_state + l] = g.in.seg_state[i * g.n_state + l];
        return;
    }
    int64_t off;
    flt_record(a, i, off);
    g.out.rec_off[o] = a.rec_off ? a.rec_off[i] : off;
    g.out.rec_len[o] = a.rec_off ? a.rec_len[i] : a.stride;
    g.out.record_id[o] = g.first_record_id + i;
    g.out.segment[o] = a.segmap ? a.seg_out[i] : -1;
}
#endif   // CBX_FILTER_HOST_ONLY

}  // namespace cbx
