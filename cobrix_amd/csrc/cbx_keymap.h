// cbx_keymap.h -- lookup joins (cbx_key_map_create_from_records, cbx_join_records, cbx_select_ordinals): a key set
// whose members carry the ordinal of the dimension row they came from, and the keyed filter stage that also emits,
// per kept fact row, the matching dimension row.
//
// A key map is the set S of cbx_keyset_from.h plus two arrays over its values: first_row[j], the smallest ordinal
// among the source rows the source filter keeps whose key is value j, and n_rows[j], the number of such rows.
//   fill:   one pass over the source records in the geometry of keyset_distinct_kernel (256 threads, lane = record,
//           grid-stride under max_workgroups, LUT and literal pool in LDS), launched after the set is complete: the
//           table and the value array are read with ordinary loads.  The row filter first; a kept lane probes the
//           FINISHED SET with the SOURCE plan's GrpProg -- ks_value_hash of a value equals grp_key_hash of any record
//           carrying that key, the scales of a numeric pair are equal, and ks_record_equals streams the record through
//           its own plan's code page against the stored UTF-8 bytes -- and on a hit at value j does one 64-bit atomic
//           min on first_row[j] (initialised to INT64_MAX) and one 64-bit atomic add on n_rows[j], both relaxed and
//           agent-scope.  A minimum and a sum: the result depends neither on the grid nor on which lane came first.
//           A source row with a null key, or one whose key was dropped, finds no member.
//   stats:  one lane per value: members with n_rows > 1, the largest n_rows, members no row reached (an internal
//           error: every member came from a kept row); one atomic per wave and counter.
//   test:   keyset_test_kernel followed, for lanes still kept, by the map probe with the PROBE plan's GrpProg: the
//           keep word and the tile count as there, and match_tmp[i] (rows_tmp[i] when asked) for kept lanes.
//   emit:   filter_emit_kernel, unchanged, writes the selection; keymap_emit_kernel compacts match_tmp / rows_tmp
//           with the same keep words and scanned bases.
//   gather: ordinals_gather_kernel, one lane per ordinal: the selection row filter_emit_kernel writes for that
//           source record.
// The probe (key decode, hash, table walk, compare) is one out-of-line call shared by both sides, as keyset_probe is:
// inlined into a tile loop beside filter_keep the string compare is what took group_accumulate_kernel to 256 VGPRs.
// No spin, no flag, no fence; every probe loop is bounded by the capacity; whole waves leave together after the only
// barrier.
//
// ks_find, the payload update rule, the join verdict and the ordinal gather's row are host/device:
// tests/native/keymap_host.cpp runs them on the host (CBX_FILTER_HOST_ONLY leaves the kernels out).  Not part of the
// hipRTC bundle.
#pragma once

#include "cbx_keyset_from.h"

namespace cbx {

constexpr int64_t kKmNoRow = INT64_MAX;   // first_row of a member no source row has reached yet

// ks_member returning the value's index: -1 when the table does not hold the record's key (non-null, hashed by
// ks_record_key with the same Tab).
template <typename Tab, typename LutFn>
CBX_HD int64_t ks_find(const Tab& tab, const KsTable& t, const GrpKeyVal* kv, const GrpRec& me, int start_off, LutFn lut,
                       uint64_t hash) {
    const uint64_t mask = t.capacity - 1, fp = hash >> 32;
    for (uint64_t p = 0; p < t.capacity; p++) {
        const uint64_t w = t.slots[(hash + p) & mask];
        if (w == 0) return -1;
        if ((w >> 32) != fp) continue;
        const int64_t j = (int64_t)(w & 0xFFFFFFFFull) - 1;
        if (ks_record_equals(tab, kv, me, start_off, lut, t.vals + j * t.n_keys, t.bytes + j * (int64_t)t.str_stride, t.str_off))
            return j;
    }
    return -1;
}

// The member a record's key is: its value index, -1 for a null key component or a key that is no member.  Tab is the
// key program of the record's OWN plan (the probe plan's for a fact row, the source plan's for a dimension row).
template <typename Tab, typename LutFn>
CBX_HD int64_t km_lookup(const Tab& tab, const KsTable& t, const GrpRec& me, int start_off, LutFn lut) {
    GrpKeyVal kv[CBX_GROUP_MAX_KEYS];
    uint64_t hash;
    if (!ks_record_key(tab, me, start_off, lut, kv, hash)) return -1;
    return ks_find(tab, t, kv, me, start_off, lut, hash);
}

// The payload update of source row `ordinal` whose key is value j.  Ops: min64(p, v), add(p, v).
template <typename Ops>
CBX_HD void km_update(const Ops& ops, int64_t* first_row, int64_t* n_rows, int64_t j, int64_t ordinal) {
    ops.min64(first_row + j, ordinal);
    (void)ops.add((uint64_t*)(n_rows + j), 1ull);
}

// The join verdict of a record the cbx_filter and every set keep (K is true): m = first_row of its member or -1,
// rows = n_rows of that member or 0; true when the join type keeps the record.
template <typename Tab, typename LutFn>
CBX_HD bool km_verdict(int32_t join_type, const Tab& tab, const KsTable& t, const int64_t* first_row, const int64_t* n_rows,
                       const GrpRec& me, int start_off, LutFn lut, int64_t& m, int64_t& rows) {
    const int64_t j = km_lookup(tab, t, me, start_off, lut);
    m = j >= 0 ? first_row[j] : -1;
    rows = j >= 0 ? n_rows[j] : 0;
    return join_type == CBX_JOIN_LEFT || m >= 0;
}

// What cbx_join_records refuses about the map, the join type and the match array before anything else is looked at
// (CBX_E_ARGUMENT, reason in err).
inline int km_join_check(bool has_map, bool map_of_plan, int32_t join_type, bool has_match, int32_t n_sets, bool has_sets,
                         std::string& err) {
    if (!has_map) err = "cbx_join_records: map: null";
    else if (!map_of_plan) err = "cbx_join_records: map: built for another probe plan";
    else if (join_type != CBX_JOIN_INNER && join_type != CBX_JOIN_LEFT)
        err = "cbx_join_records: join_type " + std::to_string(join_type) + " is neither CBX_JOIN_INNER nor CBX_JOIN_LEFT";
    else if (!has_match) err = "cbx_join_records: d_match must not be NULL";
    else if (n_sets < 0 || n_sets > CBX_GROUP_MAX_KEYS || (n_sets > 0 && !has_sets))
        err = "cbx_join_records: 0 to " + std::to_string(CBX_GROUP_MAX_KEYS) + " key sets";
    else return CBX_OK;
    return CBX_E_ARGUMENT;
}

// The selection row of source record `ord` of n: false (a zero-length record at offset 0) when it lies outside.
struct KmRow {
    int64_t rec_off, record_id;
    int32_t rec_len, segment;
};
CBX_HD bool km_ordinal_row(int64_t ord, int64_t n, const int64_t* rec_off, const int32_t* rec_len, int32_t stride,
                           int64_t first_record_id, KmRow& r) {
    r.rec_off = 0; r.rec_len = 0; r.record_id = -1; r.segment = -1;
    if (ord < 0 || ord >= n) return false;
    r.rec_off = rec_off ? rec_off[ord] : ord * (int64_t)stride;
    r.rec_len = rec_off ? rec_len[ord] : stride;
    r.record_id = first_record_id + ord;
    return true;
}

#ifndef CBX_FILTER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernels (included by cbx_capi.hip after cbx_keyset_from.h)
// ------------------------------------------------------------------------------------------
enum { KM_DUPLICATES = 0, KM_MAX_ROWS = 1, KM_UNFILLED = 2, KM_WORDS = 8 };

// The map as a kernel sees it, in the call's block beside the programs: the set's table, the key program of the
// records that probe it, the payload.
struct KmDevMap {
    KsTable t;
    const CBX_CONST GrpProg* grp;
    int64_t* first_row;            // [n_values]
    int64_t* n_rows;               // [n_values]
};
static_assert(sizeof(KmDevMap) % 4 == 0, "KmDevMap is a dword struct");

struct KmFillArgs {
    FilterArgs a;                       // the source records (keep / counts / seg_out unused)
    const CBX_CONST KmDevMap* map;      // grp: the SOURCE plan's keys
    int32_t has_filter, reserved;
};

struct KmJoinArgs {
    const CBX_CONST KmDevMap* map;      // grp: the PROBE plan's keys (the set's own program)
    int64_t* match_tmp;                 // [n] first_row of a kept record's member, -1 none
    int64_t* rows_tmp;                  // [n] n_rows of that member; nullptr: not asked for
    int32_t join_type, reserved;
};

// The value index of a record's key in the map's set, -1 none.  Out of line, as keyset_probe is and for its reason.
// (The map's address is wave-uniform; a call passes it in vector registers, so it is made scalar again here.)
__device__ __noinline__ int64_t keymap_lookup(const CBX_CONST KmDevMap* m, const uint32_t* s_lut, const uint8_t* rec, int avail,
                                              int64_t head, int seg, int start_off) {
    const uint64_t mp = (uint64_t)m;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)mp), hi = __builtin_amdgcn_readfirstlane((uint32_t)(mp >> 32));
    const CBX_CONST KmDevMap* sm = (const CBX_CONST KmDevMap*)(((uint64_t)hi << 32) | lo);
    const KsTable t = ldc(&sm->t);
    const GrpDevTab tab{ldc(&sm->grp)};
    const GrpRec me{rec, avail, head, seg};
    return km_lookup(tab, t, me, start_off, [&](uint32_t b) -> uint32_t { return s_lut[b]; });
}

__global__ __launch_bounds__(256) void keymap_init_kernel(int64_t* first_row, int64_t* n_rows, int64_t n_values) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_values) return;
    first_row[j] = kKmNoRow;
    n_rows[j] = 0;
}

// Whole waves stay in the tile loop together; the only barrier is the one after the LDS tables are filled.
__global__ __launch_bounds__(kFltThreads) void keymap_fill_kernel(KmFillArgs g) {
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
    const GrpDevOps ops{nullptr, 0};
    int64_t* first_row = ldc(&g.map->first_row);
    int64_t* n_rows = ldc(&g.map->n_rows);
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
        if (j >= 0) km_update(ops, first_row, n_rows, j, i);
    }
}

// One lane per value of a payload the fill pass completed (the launch before: ordinary loads).
__global__ __launch_bounds__(256) void keymap_stats_kernel(const int64_t* first_row, const int64_t* n_rows, int64_t n_values,
                                                           uint64_t* hdr) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t rows = 0;
    bool unfilled = false;
    if (j < n_values) {
        rows = n_rows[j];
        unfilled = rows < 1 || first_row[j] == kKmNoRow;
    }
    const uint64_t dm = __ballot(rows > 1), um = __ballot(unfilled);
    for (int d = 32; d > 0; d >>= 1) {
        const int64_t o = __shfl_xor(rows, d, 64);
        rows = o > rows ? o : rows;
    }
    if ((threadIdx.x & 63) == 0) {
        if (dm) (void)__hip_atomic_fetch_add(hdr + KM_DUPLICATES, (uint64_t)__popcll(dm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (um) (void)__hip_atomic_fetch_add(hdr + KM_UNFILLED, (uint64_t)__popcll(um), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rows > 0) (void)__hip_atomic_fetch_max(hdr + KM_MAX_ROWS, (uint64_t)rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// keyset_test_kernel, then the map probe for lanes still kept.
__global__ __launch_bounds__(kFltThreads) void keymap_test_kernel(KsArgs g, KmJoinArgs jn) {
    __shared__ uint32_t s_lut[256];
    __shared__ uint8_t s_pool[CBX_FILTER_POOL_BYTES];
    const FilterArgs& a = g.a;
    for (int i = threadIdx.x; i < 256; i += kFltThreads) s_lut[i] = a.lut[i];
    if (g.has_filter) {
        const CBX_CONST uint32_t* pw = (const CBX_CONST uint32_t*)a.prog->pool;
        for (int i = threadIdx.x; i < CBX_FILTER_POOL_BYTES / 4; i += kFltThreads) ((uint32_t*)s_pool)[i] = pw[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (kFltThreads / 64) + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;   // whole waves leave (after the only barrier)
    const int64_t i = tile * 64 + lane;
    bool keep = false;
    if (i < a.n) {
        int64_t off;
        const int avail = flt_record(a, i, off);
        const uint8_t* rec = a.data + off;
        int seg = -1;
        if (a.rec_seg) seg = a.rec_seg[i];
        else if (a.segmap) {
            seg = flt_segment(a, s_lut, rec, avail);
            a.seg_out[i] = (int16_t)seg;   // the emit pass takes it from here: the record is read once
        }
        keep = true;
        if (g.has_filter) {
            FilterDevTab tab{a.prog};
            keep = filter_keep(tab, s_pool, rec, avail, off, a.start_off, seg, [&](uint32_t b) -> uint32_t { return s_lut[b]; });
        }
        for (int s = 0; s < g.n_sets && keep; s++) keep = keyset_probe(g.sets + s, s_lut, rec, avail, off, seg, a.start_off);
        if (keep) {
            const int64_t j = keymap_lookup(jn.map, s_lut, rec, avail, off, seg, a.start_off);
            const int64_t m = j >= 0 ? ldc(&jn.map->first_row)[j] : -1;
            keep = jn.join_type == CBX_JOIN_LEFT || m >= 0;
            if (keep) {
                jn.match_tmp[i] = m;
                if (jn.rows_tmp) jn.rows_tmp[i] = j >= 0 ? ldc(&jn.map->n_rows)[j] : 0;
            }
        }
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) {
        a.keep[tile] = m;
        a.counts[tile] = (uint32_t)__popcll(m);
    }
}

// match_tmp / rows_tmp of the kept records, compacted as filter_emit_kernel compacts the selection.
__global__ __launch_bounds__(kFltThreads) void keymap_emit_kernel(const uint64_t* keep, const int64_t* base, int64_t n_tiles,
                                                                  const int64_t* match_tmp, const int64_t* rows_tmp,
                                                                  int64_t* d_match, int64_t* d_match_rows) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (kFltThreads / 64) + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const uint64_t m = keep[tile];
    if (!((m >> lane) & 1)) return;
    const int64_t i = tile * 64 + lane;
    const int64_t o = base[tile] + __popcll(m & ((1ull << lane) - 1ull));
    d_match[o] = match_tmp[i];
    if (d_match_rows) d_match_rows[o] = rows_tmp[i];
}

// Row j of `out`: what filter_emit_kernel writes for source record ord[j].  An ordinal outside [0, a.n) gives a
// zero-length record at offset 0 (record id -1, no segment, no root).
__global__ __launch_bounds__(256) void ordinals_gather_kernel(FilterArgs a, const int64_t* ord, int64_t n_ord, cbx_selection in,
                                                              int32_t has_in, int32_t n_state, int64_t first_record_id,
                                                              cbx_selection out) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_ord) return;
    const int64_t i = ord[o];
    KmRow r;
    const bool inside = km_ordinal_row(i, a.n, a.rec_off, a.rec_len, a.stride, first_record_id, r);
    if (has_in) {
        if (inside) { r.record_id = in.record_id[i]; r.segment = in.segment[i]; }
        if (n_state > 0 && in.seg_state && out.seg_state)
            for (int l = 0; l < n_state; l++) out.seg_state[o * n_state + l] = inside ? in.seg_state[i * n_state + l] : (l ? -2 : -1);
    } else if (inside && a.segmap) {
        int64_t off;
        const int avail = flt_record(a, i, off);
        r.segment = flt_segment(a, a.lut, a.data + off, avail);
    }
    out.rec_off[o] = r.rec_off;
    out.rec_len[o] = r.rec_len;
    out.record_id[o] = r.record_id;
    out.segment[o] = r.segment;
}
#endif   // CBX_FILTER_HOST_ONLY

}  // namespace cbx
