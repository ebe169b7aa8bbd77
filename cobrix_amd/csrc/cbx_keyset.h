// cbx_keyset.h -- key-set filters (cbx_key_set_create, cbx_filter_records_keyed): a persistent set of key values on
// the device and a filter test pass that probes it -- WHERE (k1..kK) IN (set) / k NOT IN (set) for sets past the 64
// literals of a cbx_filter (a semi join against a dimension's keys, Spark's runtime In filters).
//
// Table: open addressing with linear probing over `capacity` slots (the power of two >= 2 * max(1, n_values)).  A
// slot is one 64-bit word: 0 (empty), or the high 32 bits of the key's hash (the fingerprint) in the high half and
// the value's index + 1 in the low half.  THE KEY STORAGE IS THE UPLOADED VALUE ARRAY (cbx_key_value tuples and the
// string bytes beside them): a prober that meets a word with its own fingerprint compares its key with value
// `index` there, so unlike the group table (whose slot names a record that is decoded again on every probe) a probe
// that does not match costs one 8-byte load and one compare of 32 bits.
//   build: one lane per value.  The lane hashes its tuple, probes, claims an empty slot with one device-scope
//          64-bit compare-and-swap, and on an occupied slot with an equal fingerprint compares its tuple with the
//          occupant's tuple in the value array -- which was uploaded before the launch, so no lane ever waits for
//          another lane's store.  This is the discipline of cbx_group.h, kept here: there is no "being written"
//          state, no spin, no flag and no fence, and every probe loop is bounded by the capacity.  n_distinct is the
//          number of successful claims, max_probe an atomic max of the slots a lane visited.
//   test:  the geometry of filter_test_kernel (256 threads, lane = record, 4 tiles per workgroup, LUT and literal
//          pool in LDS, term tables through the constant address space).  The cbx_filter is evaluated first, the
//          sets are probed only for lanes still kept: the record's key is canonicalised by grp_key_hash (agg_value
//          for numerics, grp_str_load and the streaming LUT walk for strings -- no second decoder), the fingerprint
//          is compared before the key, numerics compare as (hi, lo), strings by streaming the record's span
//          through the code page against the stored bytes (flt_str_cmp).  The table is read-only here and was
//          built by an earlier launch: ordinary global loads.  The keep word and the tile count are balloted as in
//          filter_test_kernel; the scan and filter_emit_kernel are the filter stage's own.
// The value-side hash (ks_value_hash) equals grp_key_hash of a record carrying that key: grp_mix over (lo, hi + 2)
// for a numeric, the FNV of the UTF-8 bytes and len + 1 for a string.
//
// keyset_layout, the hashes, insert and the membership test are host/device: tests/native/keyset_host.cpp runs them
// on the host (CBX_FILTER_HOST_ONLY leaves the kernels out).  Not part of the hipRTC bundle.
#pragma once

#include "cbx_group.h"

namespace cbx {

// The set as the kernels see it (device pointers; the host shim fills it with host pointers).
struct KsTable {
    const uint64_t* slots;         // [capacity]
    const cbx_key_value* vals;     // [n_values][n_keys]
    const uint8_t* bytes;          // [n_values][str_stride]
    uint64_t capacity;
    int64_t n_values;
    int32_t n_keys, str_stride;
    int32_t str_off[CBX_GROUP_MAX_KEYS];
};

struct KsLayout {
    int64_t capacity;
    int64_t device_bytes;          // program + header + slots + values + string bytes
    size_t o_hdr, o_slots, o_vals, o_bytes;
    int32_t str_stride;
    int32_t str_off[CBX_GROUP_MAX_KEYS];
};

// Strides, capacity and device block of a set of n_values tuples over the keys of P (group_build's result);
// str_stride / str_off as the caller gave them (they must be the group layout's).  CBX_E_ARGUMENT, reason in err.
inline int keyset_layout(const cbx_field* fields, const cbx_group_by* gb, int64_t n_values, int32_t str_stride,
                         const int32_t* str_off, KsLayout* L, std::string& err) {
    memset(L, 0, sizeof(*L));
    if (n_values < 0) { err = "cbx_key_set_create: n_values must not be negative"; return CBX_E_ARGUMENT; }
    int32_t off = 0;
    for (int k = 0; k < gb->n_keys; k++) {
        const cbx_field& cf = fields[gb->fields[k]];
        L->str_off[k] = off;
        if (cf.kind == CBX_K_STRING || cf.kind == CBX_K_STRING_ASCII) {
            if (!str_off || str_off[k] != off) {
                err = "cbx_key_set_create: key " + std::to_string(k) + ": str_off is not the group layout's (" + std::to_string(off) + ")";
                return CBX_E_ARGUMENT;
            }
            off += 3 * cf.size;
        }
    }
    L->str_stride = off;
    if (str_stride != off) {
        err = "cbx_key_set_create: str_stride is not the group layout's (" + std::to_string(off) + ")";
        return CBX_E_ARGUMENT;
    }
    const int64_t limit = CBX_GROUP_MAX_WORKSPACE_BYTES;
    const int64_t per_value = 16 + (int64_t)sizeof(cbx_key_value) * gb->n_keys + off;   // two slots and the tuple
    if (n_values > limit / per_value) {
        err = "cbx_key_set_create: n_values needs a workspace above " + std::to_string(limit) + " bytes";
        return CBX_E_ARGUMENT;
    }
    int64_t cap = 2;
    while (cap < 2 * n_values) cap <<= 1;
    L->capacity = cap;
    L->o_hdr = (sizeof(GrpProg) + 63) & ~(size_t)63;
    L->o_slots = L->o_hdr + 64;
    L->o_vals = L->o_slots + 8 * (size_t)cap;
    L->o_bytes = L->o_vals + sizeof(cbx_key_value) * (size_t)gb->n_keys * (size_t)n_values;
    L->device_bytes = (int64_t)(L->o_bytes + (size_t)off * (size_t)n_values + 64);
    if (L->device_bytes > limit) {
        err = "cbx_key_set_create: n_values needs a workspace above " + std::to_string(limit) + " bytes";
        return CBX_E_ARGUMENT;
    }
    return CBX_OK;
}

// Every string value's length lies in [0, 3 x the field size].
inline int keyset_check_values(const GrpProg& P, const cbx_key_value* vals, int64_t n_values, std::string& err) {
    for (int k = 0; k < P.n_keys; k++) {
        if (!P.keys[k].is_str) continue;
        const int32_t cap = 3 * P.keys[k].f.size;
        for (int64_t i = 0; i < n_values; i++) {
            const int32_t n = vals[i * P.n_keys + k].str_len;
            if (n < 0 || n > cap) {
                err = "cbx_key_set_create: value " + std::to_string(i) + " key " + std::to_string(k) + ": str_len " +
                      std::to_string(n) + " outside 0.." + std::to_string(cap);
                return CBX_E_ARGUMENT;
            }
        }
    }
    return CBX_OK;
}

// The hash of value tuple v (string bytes at vb + str_off[k]): grp_key_hash of a record carrying that key.
template <typename Tab>
CBX_HD uint64_t ks_value_hash(const Tab& tab, const cbx_key_value* v, const uint8_t* vb, const int32_t* str_off) {
    uint64_t h = 0x243F6A8885A308D3ull;
    const int nk = tab.n_keys();
    for (int k = 0; k < nk; k++) {
        if (tab.key(k).is_str) {
            const uint8_t* s = vb + str_off[k];
            const uint64_t len = (uint64_t)v[k].str_len;
            uint64_t g = 0xCBF29CE484222325ull;
            for (uint64_t i = 0; i < len; i++) g = (g ^ s[i]) * 0x100000001B3ull;
            h = grp_mix(grp_mix(h, g), len + 1);
        } else {
            h = grp_mix(grp_mix(h, v[k].lo), v[k].hi + 2);
        }
    }
    return h ^ (h >> 32);
}

// Are value tuples a and b one member?
template <typename Tab>
CBX_HD bool ks_values_equal(const Tab& tab, const cbx_key_value* a, const uint8_t* ab, const cbx_key_value* b,
                            const uint8_t* bb, const int32_t* str_off) {
    const int nk = tab.n_keys();
    for (int k = 0; k < nk; k++) {
        if (tab.key(k).is_str) {
            if (a[k].str_len != b[k].str_len) return false;
            const uint8_t *x = ab + str_off[k], *y = bb + str_off[k];
            for (int i = 0; i < a[k].str_len; i++) if (x[i] != y[i]) return false;
        } else if (a[k].lo != b[k].lo || a[k].hi != b[k].hi) {
            return false;
        }
    }
    return true;
}

CBX_HD uint64_t ks_word(uint64_t hash, int64_t index) { return (hash & 0xFFFFFFFF00000000ull) | (uint64_t)(index + 1); }

// Value i into the table: true when it claimed a slot (a new member), false when the table already holds an equal
// tuple.  Ops: load(p) and cas(p, want) (the word found, 0 when the claim succeeded) on slot words.  probes: slots
// visited.  The capacity is at least twice the number of values, so the loop always ends in one of the two.
template <typename Tab, typename Ops>
CBX_HD bool ks_insert(const Tab& tab, Ops& ops, uint64_t* slots, const KsTable& t, int64_t i, int64_t& probes) {
    const int nk = t.n_keys;
    const cbx_key_value* v = t.vals + i * nk;
    const uint8_t* vb = t.bytes + i * (int64_t)t.str_stride;
    const uint64_t hash = ks_value_hash(tab, v, vb, t.str_off), mask = t.capacity - 1;
    const uint64_t mine = ks_word(hash, i);
    for (uint64_t p = 0; p < t.capacity; p++) {
        const uint64_t idx = (hash + p) & mask;
        probes = (int64_t)p + 1;
        uint64_t w = ops.load(slots + idx);
        if (w == 0) {
            w = ops.cas(slots + idx, mine);
            if (w == 0) return true;
        }
        if ((w >> 32) != (mine >> 32)) continue;
        const int64_t j = (int64_t)(w & 0xFFFFFFFFull) - 1;
        if (ks_values_equal(tab, v, vb, t.vals + j * nk, t.bytes + j * (int64_t)t.str_stride, t.str_off)) return false;
    }
    return false;   // (not reached)
}

// Is record me's key (non-null; numeric values in kv) value tuple v?  Numerics first, then the strings streamed.
template <typename Tab, typename LutFn>
CBX_HD bool ks_record_equals(const Tab& tab, const GrpKeyVal* kv, const GrpRec& me, int start_off, LutFn lut,
                             const cbx_key_value* v, const uint8_t* vb, const int32_t* str_off) {
    const int nk = tab.n_keys();
    bool strs = false;
    for (int k = 0; k < nk; k++) {
        if (tab.key(k).is_str) { strs = true; continue; }
        if (kv[k].lo != v[k].lo || (uint64_t)kv[k].hi != v[k].hi) return false;
    }
    if (!strs) return true;
    for (int k = 0; k < nk; k++) {
        const AggTerm tm = tab.key(k);
        if (!tm.is_str) continue;
        FltBytes b;
        StrSpan s;
        if (!grp_str_load(tm, me, start_off, lut, b, s)) return false;
        const int kind = tm.f.kind;
        bool starts;
        if (flt_str_cmp(b, s, vb + str_off[k], v[k].str_len, [&](uint32_t x) -> uint32_t { return grp_lut(kind, lut, x); },
                        starts) != 0)
            return false;
    }
    return true;
}

// The key of record me: false when a component is null, else its hash (and the numerics' values in kv).
template <typename Tab, typename LutFn>
CBX_HD bool ks_record_key(const Tab& tab, const GrpRec& me, int start_off, LutFn lut, GrpKeyVal* kv, uint64_t& hash) {
    hash = grp_key_hash(tab, me, start_off, lut, kv);
    const int nk = tab.n_keys();
    bool null = false;
    for (int k = 0; k < CBX_GROUP_MAX_KEYS; k++) null |= k < nk && kv[k].null != 0;
    return !null;
}

// Does the table hold the record's key (non-null, hashed by ks_record_key)?
template <typename Tab, typename LutFn>
CBX_HD bool ks_member(const Tab& tab, const KsTable& t, const GrpKeyVal* kv, const GrpRec& me, int start_off, LutFn lut,
                      uint64_t hash) {
    const uint64_t mask = t.capacity - 1, fp = hash >> 32;
    for (uint64_t p = 0; p < t.capacity; p++) {
        const uint64_t w = t.slots[(hash + p) & mask];
        if (w == 0) return false;
        if ((w >> 32) != fp) continue;
        const int64_t j = (int64_t)(w & 0xFFFFFFFFull) - 1;
        if (ks_record_equals(tab, kv, me, start_off, lut, t.vals + j * t.n_keys, t.bytes + j * (int64_t)t.str_stride, t.str_off))
            return true;
    }
    return false;
}

// One set's verdict on a record: IN keeps members, NOT IN keeps non-members; a null key component is kept by neither.
template <typename Tab, typename LutFn>
CBX_HD bool ks_keep(const Tab& tab, const KsTable& t, bool negate, const GrpRec& me, int start_off, LutFn lut) {
    GrpKeyVal kv[CBX_GROUP_MAX_KEYS];
    uint64_t hash;
    if (!ks_record_key(tab, me, start_off, lut, kv, hash)) return false;
    return ks_member(tab, t, kv, me, start_off, lut, hash) != negate;
}

#ifndef CBX_FILTER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernels (included by cbx_capi.hip after cbx_group.h)
// ------------------------------------------------------------------------------------------
constexpr int kKsBuildThreads = 256;

struct KsDevSet {
    KsTable t;
    const CBX_CONST GrpProg* grp;
    int32_t negate, reserved;
};

static_assert(sizeof(KsDevSet) % 4 == 0, "KsDevSet is a dword struct");

struct KsArgs {
    FilterArgs a;
    int32_t has_filter, n_sets;
    const CBX_CONST KsDevSet* sets;   // [n_sets], in the call's block beside the filter program
};

struct KsDevOps {
    __device__ __forceinline__ uint64_t load(uint64_t* p) const {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint64_t cas(uint64_t* p, uint64_t want) const {
        uint64_t expected = 0;
        __hip_atomic_compare_exchange_strong(p, &expected, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;   // 0: claimed; else the winner's word
    }
};

// hdr: [0] successful claims, [1] the longest probe sequence.  The slot words were zeroed on the stream before.
__global__ __launch_bounds__(kKsBuildThreads) void keyset_build_kernel(KsTable t, const CBX_CONST GrpProg* grp, uint64_t* slots,
                                                                       uint64_t* hdr) {
    const int64_t i = (int64_t)blockIdx.x * kKsBuildThreads + threadIdx.x;
    bool claimed = false;
    int64_t probes = 0;
    if (i < t.n_values) {
        const GrpDevTab tab{grp};
        KsDevOps ops;
        claimed = ks_insert(tab, ops, slots, t, i, probes);
    }
    const uint64_t m = __ballot(claimed);
    for (int d = 32; d > 0; d >>= 1) {
        const int64_t o = __shfl_xor(probes, d, 64);
        probes = o > probes ? o : probes;
    }
    if ((threadIdx.x & 63) == 0) {
        if (m) (void)__hip_atomic_fetch_add(hdr, (uint64_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (probes) (void)__hip_atomic_fetch_max(hdr + 1, (uint64_t)probes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One set's verdict, out of line: the key kinds differ per set, and inlined four times over the test kernel's body
// the string compare costs waves (the group kernel's 256 VGPRs are the known trap).
// (The set's address is wave-uniform; a call passes it in vector registers, so it is made scalar again here and
// the set's descriptor and key terms come through scalar loads.)
__device__ __noinline__ bool keyset_probe(const CBX_CONST KsDevSet* s, const uint32_t* s_lut, const uint8_t* rec, int avail,
                                          int64_t head, int seg, int start_off) {
    const uint64_t sp = (uint64_t)s;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)sp), hi = __builtin_amdgcn_readfirstlane((uint32_t)(sp >> 32));
    const KsDevSet S = ldc((const CBX_CONST KsDevSet*)(((uint64_t)hi << 32) | lo));
    const GrpDevTab tab{S.grp};
    const GrpRec me{rec, avail, head, seg};
    return ks_keep(tab, S.t, S.negate != 0, me, start_off, [&](uint32_t b) -> uint32_t { return s_lut[b]; });
}

__global__ __launch_bounds__(kFltThreads) void keyset_test_kernel(KsArgs g) {
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
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) {
        a.keep[tile] = m;
        a.counts[tile] = (uint32_t)__popcll(m);
    }
}
#endif   // CBX_FILTER_HOST_ONLY

}  // namespace cbx
