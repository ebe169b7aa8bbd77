// cbx_keyset_from.h -- key sets built on the device from the records of a second file
// (cbx_key_set_create_from_records): the distinct keys of a dimension file become the set a fact file is filtered
// with, without a trip of the keys through the host.
//
// Two plans meet here.  The SOURCE plan (the dimension: its copybook, code page, trimming policy and row filter)
// decodes the keys; the PROBE plan (the fact file) owns the set and defines what a key value may be.  The canonical
// key is the one of cbx_group.h and cbx_keyset.h -- a numeric the signed 128-bit value at the column's output scale,
// a string the UTF-8 bytes of the trimmed field -- so a pair of numeric columns with equal scales and a pair of
// string columns compare without arithmetic, whatever their encodings and widths.
//   distinct: one pass over the source records in the geometry of filter_test_kernel (256 threads, lane = record,
//             4 tiles per workgroup at a time, LUT and literal pool in LDS, grid-stride under max_workgroups).  The
//             row filter first, then grp_key_hash with the source plan's GrpProg; a record with a null key component
//             is counted and skipped; the rest find or claim a slot of a table of bare 64-bit words (0: empty, else
//             representative record + 1).  This is the find-or-claim half of group_accumulate_kernel: no GrpAcc, no
//             LDS cache, no per-term work.  The discipline of cbx_group.h holds: a slot's key is the key of the
//             immutable record it names, so there is no "being written" state, no spin, no flag, no fence, and every
//             probe loop is bounded by the capacity; claimed() raises the overflow flag past max_values and stopped()
//             lets later lanes leave.  The key decoders (ksf_key) and the representative compare (ksf_rep_equal) are
//             out of line, called side by side from the tile loop.
//   convert:  one lane per slot.  An occupied slot decodes its representative's key, applies the probe columns'
//             bounds (precomputed 128-bit limits, UTF-8 byte and character limits: the device only compares), takes
//             a dense index (ballot, one atomic add per wave) and writes the cbx_key_value tuple and the string
//             bytes into the new set's value array in keyset_layout's layout for the probe keys.  A value the probe
//             columns can never hold is counted and left out.
//   build:    keyset_build_kernel of cbx_keyset.h, unchanged, over that array: it is complete before the launch.
// Host waits: three.  One after the distinct pass (claims, overflow flag, the row counts: it sizes the set's block
// for at most that many values), one after the convert pass (keyset_build_kernel takes the number of values by
// value, and dropped values make it smaller than the claims; it also gives the table the capacity cbx_key_set_create
// would choose for those values), and the one cbx_key_set_create ends with.
//
// keyset_from_build (compatibility, bounds), the conversion rule and find-or-claim on bare slots are host/device:
// tests/native/keyset_from_host.cpp runs them on the host (CBX_FILTER_HOST_ONLY leaves the kernels out).  Not part of
// the hipRTC bundle.
#pragma once

#include <vector>

#include "cbx_keyset.h"

namespace cbx {

// What probe key k can hold.  Numeric: min <= value <= max as signed 128-bit numbers; string: UTF-8 bytes and
// characters.
struct KsfBound {
    int64_t min_hi;
    uint64_t min_lo;
    int64_t max_hi;
    uint64_t max_lo;
    int32_t max_bytes, max_chars;
    int32_t reserved[2];
};
static_assert(sizeof(KsfBound) == 48, "KsfBound is a dword struct");

struct KsfProg {
    GrpProg src;                            // the source plan's keys
    KsfBound bound[CBX_GROUP_MAX_KEYS];     // the probe plan's limits
};

struct KsfHostTab {
    const KsfProg* p;
    CBX_HD int n_keys() const { return p->src.n_keys; }
    CBX_HD AggTerm key(int k) const { return p->src.keys[k]; }
    CBX_HD KsfBound bound(int k) const { return p->bound[k]; }
};

inline int ksf_scale_of(const cbx_field& f) {
    return (f.out_type == CBX_O_DEC64 || f.out_type == CBX_O_DEC128) ? f.out_scale : 0;
}

// Both key tables -> the probe plan's GrpProg (the set's program), the source plan's with the bounds.  Each side is
// refused as group_build refuses, its wording prefixed by the side; then the pairs: CBX_E_ARGUMENT for a different
// number of keys or a string against a numeric, CBX_E_UNSUPPORTED for different scales.
inline int keyset_from_build(const cbx_field* pf, int32_t n_pf, bool p_walk, const cbx_group_by* pk, const cbx_field* sf,
                             int32_t n_sf, bool s_walk, const cbx_group_by* sk, GrpProg* probe, KsfProg* out,
                             std::string& err) {
    std::vector<AggProg> none(1);
    memset(none.data(), 0, sizeof(AggProg));
    memset(out, 0, sizeof(*out));
    int rb = group_build(pf, n_pf, p_walk, pk, none[0], probe, err);
    if (rb != CBX_OK) { err = "probe: " + err; return rb; }
    rb = group_build(sf, n_sf, s_walk, sk, none[0], &out->src, err);
    if (rb != CBX_OK) { err = "source: " + err; return rb; }
    if (pk->n_keys != sk->n_keys) {
        err = "cbx_key_set_create_from_records: " + std::to_string(pk->n_keys) + " probe keys against " +
              std::to_string(sk->n_keys) + " source keys";
        return CBX_E_ARGUMENT;
    }
    for (int k = 0; k < pk->n_keys; k++) {
        const cbx_field& a = pf[pk->fields[k]];
        const cbx_field& b = sf[sk->fields[k]];
        const std::string at = "cbx_key_set_create_from_records: key " + std::to_string(k) + ": ";
        KsfBound& B = out->bound[k];
        if (probe->keys[k].is_str != out->src.keys[k].is_str) {
            err = at + "a string column against a numeric one";
            return CBX_E_ARGUMENT;
        }
        if (probe->keys[k].is_str) {
            B.max_bytes = 3 * a.size;
            B.max_chars = a.size;
            continue;
        }
        if (ksf_scale_of(a) != ksf_scale_of(b)) {
            err = at + "scales " + std::to_string(ksf_scale_of(a)) + " and " + std::to_string(ksf_scale_of(b)) + " differ";
            return CBX_E_UNSUPPORTED;
        }
        unsigned __int128 top;   // the largest value the probe column holds
        if (a.out_type == CBX_O_DEC64 || a.out_type == CBX_O_DEC128) {
            if (a.out_precision < 0 || a.out_precision > 38) {
                err = at + "probe precision " + std::to_string(a.out_precision) + " outside 0..38";
                return CBX_E_ARGUMENT;
            }
            top = 1;
            for (int d = 0; d < a.out_precision; d++) top *= 10;
            top -= 1;
            const __int128 lo = -(__int128)top;
            B.min_hi = (int64_t)(lo >> 64); B.min_lo = (uint64_t)lo;
        } else {
            const int bits = a.out_type == CBX_O_I32 ? 31 : 63;
            top = (((unsigned __int128)1) << bits) - 1;
            const __int128 lo = -(__int128)top - 1;
            B.min_hi = (int64_t)(lo >> 64); B.min_lo = (uint64_t)lo;
        }
        B.max_hi = (int64_t)(top >> 64); B.max_lo = (uint64_t)top;
    }
    return CBX_OK;
}

// Where the probe keys' string bytes lie inside a value's stride (the group layout keyset_layout checks): the stride.
inline int32_t keyset_from_strides(const cbx_field* pf, const cbx_group_by* pk, const GrpProg& probe, int32_t* str_off) {
    int32_t stride = 0;
    for (int k = 0; k < CBX_GROUP_MAX_KEYS; k++) {
        str_off[k] = k < probe.n_keys ? stride : 0;
        if (k < probe.n_keys && probe.keys[k].is_str) stride += 3 * pf[pk->fields[k]].size;
    }
    return stride;
}

// The table of a set of n_values tuples inside a block laid out for n_claims >= n_values of them: the capacity
// cbx_key_set_create would have chosen for n_values (the block's slot area is the larger one; it is zeroed whole).
inline int64_t keyset_from_set_capacity(int64_t n_values) {
    int64_t cap = 2;
    while (cap < 2 * n_values) cap <<= 1;
    return cap;
}

// Slots and bytes of the distinct table; CBX_E_ARGUMENT (reason in err) when max_values or the table is out of range.
inline int keyset_from_capacity(int64_t max_values, int64_t* capacity, std::string& err) {
    if (max_values < 1) { err = "cbx_key_set_create_from_records: max_values must be at least 1"; return CBX_E_ARGUMENT; }
    const int64_t limit = CBX_GROUP_MAX_WORKSPACE_BYTES;
    if (max_values > limit / 16) {
        err = "cbx_key_set_create_from_records: max_values needs a workspace above " + std::to_string(limit) + " bytes";
        return CBX_E_ARGUMENT;
    }
    int64_t cap = 2;
    while (cap < 2 * max_values) cap <<= 1;
    if (8 * cap > limit) {
        err = "cbx_key_set_create_from_records: max_values needs a workspace above " + std::to_string(limit) + " bytes";
        return CBX_E_ARGUMENT;
    }
    *capacity = cap;
    return CBX_OK;
}

// Does the table hold record i's key (non-null, hashed by grp_key_hash) -- claimed for it if not?  Ops: load, cas,
// stopped, claimed, exhausted as grp_find_or_claim's; same(j): is the key of record j this record's key.  False
// when the record was dropped (the overflow flag is up, or the probe sequence is exhausted, which raises it).
template <typename Ops, typename Same>
CBX_HD bool ksf_find_or_claim(Ops& ops, uint64_t* slots, uint64_t capacity, uint64_t hash, int64_t i, Same same) {
    const uint64_t mask = capacity - 1;
    for (uint64_t p = 0; p < capacity; p++) {
        const uint64_t idx = (hash + p) & mask;
        uint64_t w = ops.load(slots + idx);
        if (w == 0) {
            if (ops.stopped()) return false;
            w = ops.cas(slots + idx, (uint64_t)i + 1);
            if (w == 0) { ops.claimed(); return true; }
        }
        if (same((int64_t)(w - 1))) return true;
    }
    ops.exhausted();
    return false;
}

// Is the key of record a the key of record b?  (NULL equals NULL only; the table holds no null key.)  Both records are
// decoded here -- the numerics first, then the strings streamed through the code page as grp_str_eq does -- so a
// caller keeps no key values alive across its probe loop.
template <typename Tab, typename LutFn>
CBX_HD bool ksf_records_equal(const Tab& tab, const GrpRec& a, const GrpRec& b, int start_off, LutFn lut) {
    const int nk = tab.n_keys();
    bool strs = false;
    for (int k = 0; k < nk; k++) {
        const AggTerm tm = tab.key(k);
        if (tm.is_str) { strs = true; continue; }
        int64_t ah = 0, bh = 0;
        uint64_t al = 0, bl = 0;
        const bool va = agg_value(tm, a.rec, a.avail, a.head, start_off, a.seg, ah, al);
        const bool vb = agg_value(tm, b.rec, b.avail, b.head, start_off, b.seg, bh, bl);
        if (va != vb || (va && (ah != bh || al != bl))) return false;
    }
    if (!strs) return true;
    for (int k = 0; k < nk; k++) {
        const AggTerm tm = tab.key(k);
        if (!tm.is_str) continue;
        FltBytes x, y;
        StrSpan sx, sy;
        const bool va = grp_str_load(tm, a, start_off, lut, x, sx), vb = grp_str_load(tm, b, start_off, lut, y, sy);
        if (va != vb) return false;
        if (va && !grp_str_eq(tm.f.kind, x, sx, y, sy, lut)) return false;
    }
    return true;
}

CBX_HD bool ksf_less(int64_t ahi, uint64_t alo, int64_t bhi, uint64_t blo) { return ahi < bhi || (ahi == bhi && alo < blo); }

// The key of record r (every component non-null) as the probe columns' value tuple: false when a component is one
// they can never hold.  String lengths are counted here, the bytes go out with ksf_value_bytes.
template <typename Tab, typename LutFn>
CBX_HD bool ksf_value(const Tab& tab, const GrpRec& r, int start_off, LutFn lut, cbx_key_value* v) {
    const int nk = tab.n_keys();
    bool ok = true;
    for (int k = 0; k < nk; k++) {
        const AggTerm tm = tab.key(k);
        const KsfBound b = tab.bound(k);
        cbx_key_value c;
        c.lo = c.hi = 0; c.str_len = 0; c.reserved = 0;
        if (tm.is_str) {
            FltBytes fb;
            StrSpan s;
            if (!grp_str_load(tm, r, start_off, lut, fb, s)) ok = false;
            int n = 0, chars = 0;
            for (int i = s.begin; i < s.end; i++) {
                uint32_t e = grp_lut(tm.f.kind, lut, fb[i]);
                for (int l = (int)((e >> 24) & 3); l > 0; l--) { n++; chars += (e & 0xC0u) != 0x80u ? 1 : 0; e >>= 8; }
            }
            c.str_len = n;
            ok = ok && n <= b.max_bytes && chars <= b.max_chars;
        } else {
            int64_t hi = 0;
            uint64_t lo = 0;
            if (!agg_value(tm, r.rec, r.avail, r.head, start_off, r.seg, hi, lo)) ok = false;
            c.lo = lo; c.hi = (uint64_t)hi;
            ok = ok && !ksf_less(hi, lo, b.min_hi, b.min_lo) && !ksf_less(b.max_hi, b.max_lo, hi, lo);
        }
        v[k] = c;
    }
    return ok;
}

// The string keys' UTF-8 bytes of a record ksf_value kept, at bytes + str_off[k] (the probe keys' layout).
template <typename Tab, typename LutFn>
CBX_HD void ksf_value_bytes(const Tab& tab, const GrpRec& r, int start_off, LutFn lut, const int32_t* str_off, uint8_t* bytes) {
    const int nk = tab.n_keys();
    for (int k = 0; k < nk; k++) {
        const AggTerm tm = tab.key(k);
        if (!tm.is_str) continue;
        FltBytes fb;
        StrSpan s;
        if (!grp_str_load(tm, r, start_off, lut, fb, s)) continue;
        uint8_t* o = bytes + str_off[k];
        int n = 0;
        for (int i = s.begin; i < s.end; i++) {
            uint32_t e = grp_lut(tm.f.kind, lut, fb[i]);
            for (int l = (int)((e >> 24) & 3); l > 0; l--) { o[n++] = (uint8_t)(e & 0xFFu); e >>= 8; }
        }
    }
}

#ifndef CBX_FILTER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernels (included by cbx_capi.hip after cbx_keyset.h)
// ------------------------------------------------------------------------------------------
// header words of the distinct table
enum { KSF_CLAIMS = 0, KSF_OVERFLOW = 1, KSF_NULL_ROWS = 2, KSF_ROWS = 3, KSF_VALUES = 4, KSF_DROPPED = 5, KSF_WORDS = 8 };

struct KsfArgs {
    FilterArgs a;                       // the source records (keep / counts / seg_out unused)
    const CBX_CONST KsfProg* prog;
    uint64_t* slots;                    // [capacity] 0 or representative record + 1
    uint64_t* hdr;                      // [KSF_WORDS]
    uint64_t capacity;
    int64_t max_values;
    int32_t has_filter, reserved;
};

struct KsfOut {                         // the new set's value array
    cbx_key_value* vals;
    uint8_t* bytes;
    int32_t n_keys, str_stride;
    int32_t str_off[CBX_GROUP_MAX_KEYS];
};

struct KsfDevTab {
    const CBX_CONST KsfProg* p;
    __device__ __forceinline__ int n_keys() const { return p->src.n_keys; }
    __device__ __forceinline__ AggTerm key(int k) const { return ldc(&p->src.keys[k]); }
    __device__ __forceinline__ KsfBound bound(int k) const { return ldc(&p->bound[k]); }
};

// Is the key of record `rep` the key of the record at `rec`?  Out of line: the string compare of grp_key_equal
// inlined into the probe loop is what took group_accumulate_kernel to 256 VGPRs.  Both records are decoded here, so
// the caller passes no key values and keeps none alive across its probe loop.
// (The program's address is wave-uniform; a call passes it in vector registers, so it is made scalar again here.)
__device__ __noinline__ bool ksf_rep_equal(const CBX_CONST KsfProg* prog, const uint32_t* s_lut, const uint8_t* rec, int avail,
                                           int64_t head, int seg, const uint8_t* r_rec, int r_avail, int64_t r_head, int r_seg,
                                           int start_off) {
    const uint64_t pp = (uint64_t)prog;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)pp), hi = __builtin_amdgcn_readfirstlane((uint32_t)(pp >> 32));
    const CBX_CONST KsfProg* sp = (const CBX_CONST KsfProg*)(((uint64_t)hi << 32) | lo);
    const GrpDevTab tab{&sp->src};
    const GrpRec me{rec, avail, head, seg}, rep{r_rec, r_avail, r_head, r_seg};
    return ksf_records_equal(tab, me, rep, start_off, [&](uint32_t b) -> uint32_t { return s_lut[b]; });
}

// The key of a record the filter kept: its hash, and whether every component is non-null.  Out of line as keyset_probe
// is, for the same reason: inlined into the tile loop beside filter_keep, the four key decoders took the kernel to 209
// VGPRs and 2 waves per SIMD.  The two calls are made from the kernel itself, side by side: a call inside a call
// stacks the callers' live registers on the callee's (a nested variant was at 138-182 VGPRs).
struct KsfKey {
    uint64_t hash;
    uint32_t live, reserved;
};
__device__ __noinline__ KsfKey ksf_key(const CBX_CONST KsfProg* prog, const uint32_t* s_lut, const uint8_t* rec, int avail,
                                       int64_t head, int seg, int start_off) {
    const uint64_t pp = (uint64_t)prog;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)pp), hi = __builtin_amdgcn_readfirstlane((uint32_t)(pp >> 32));
    const CBX_CONST KsfProg* sp = (const CBX_CONST KsfProg*)(((uint64_t)hi << 32) | lo);
    const GrpDevTab tab{&sp->src};
    const GrpRec me{rec, avail, head, seg};
    GrpKeyVal kv[CBX_GROUP_MAX_KEYS];   // (not returned: the compare decodes the record again)
    KsfKey r{0, 0, 0};
    r.live = ks_record_key(tab, me, start_off, [&](uint32_t b) -> uint32_t { return s_lut[b]; }, kv, r.hash) ? 1u : 0u;
    return r;
}

// Whole waves stay in the tile loop together; the only barrier is the one after the LDS tables are filled.
// (Left to itself the allocator takes 129 VGPRs, one past the 128 of four waves per SIMD: the bound is asked for.)
__global__ __launch_bounds__(kFltThreads) __attribute__((amdgpu_waves_per_eu(4))) void keyset_distinct_kernel(KsfArgs g) {
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
    const GrpDevOps ops{g.hdr, g.max_values};
    auto lutf = [&](uint32_t b) -> uint32_t { return s_lut[b]; };
    uint64_t n_rows = 0, n_null = 0;   // this wave's counts (wave-uniform): one atomic add each when the loop ends
    for (int64_t tile = (int64_t)blockIdx.x * (kFltThreads / 64) + wave; tile < a.n_tiles;
         tile += (int64_t)gridDim.x * (kFltThreads / 64)) {
        // What stays alive across the two calls is kept small (each value costs a callee-saved register, and those lie
        // high in the file): the record is named by its offset alone, its index is tile * 64 + lane again.
        bool keep = false;
        int64_t head = 0;
        int avail = 0, seg = -1;
        if (tile * 64 + lane < a.n) {
            const GrpRec me = grp_record(a, s_lut, tile * 64 + lane);
            head = me.head; avail = me.avail; seg = me.seg;
            keep = true;
            if (g.has_filter) {
                FilterDevTab ftab{a.prog};
                keep = filter_keep(ftab, s_pool, me.rec, me.avail, me.head, a.start_off, me.seg, lutf);
            }
        }
        const uint64_t km = __ballot(keep);
        if (km == 0) continue;
        n_rows += (uint64_t)__popcll(km);
        bool live = false;
        uint64_t hash = 0;
        if (keep) {
            const KsfKey key = ksf_key(g.prog, s_lut, a.data + head, avail, head, seg, a.start_off);
            live = key.live != 0;
            hash = key.hash;
        }
        n_null += (uint64_t)__popcll(__ballot(keep && !live));
        if (live)
            (void)ksf_find_or_claim(ops, g.slots, g.capacity, hash, tile * 64 + lane, [&](int64_t j) -> bool {
                const GrpRec rep = grp_record(a, s_lut, j);
                return ksf_rep_equal(g.prog, s_lut, a.data + head, avail, head, seg, rep.rec, rep.avail, rep.head, rep.seg,
                                     a.start_off);
            });
    }
    if (lane == 0) {
        if (n_rows) (void)__hip_atomic_fetch_add(g.hdr + KSF_ROWS, n_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_null) (void)__hip_atomic_fetch_add(g.hdr + KSF_NULL_ROWS, n_null, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One lane per slot of the distinct table (built by the launch before: ordinary loads).  The value array holds at
// least as many tuples as slots were claimed, so every dense index lies inside it.
__global__ __launch_bounds__(kFltThreads) void keyset_convert_kernel(KsfArgs g, KsfOut o) {
    __shared__ uint32_t s_lut[256];
    const FilterArgs& a = g.a;
    for (int i = threadIdx.x; i < 256; i += kFltThreads) s_lut[i] = a.lut[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t idx = (uint64_t)blockIdx.x * kFltThreads + threadIdx.x;
    const uint64_t w = idx < g.capacity ? g.slots[idx] : 0;
    const KsfDevTab tab{g.prog};
    auto lutf = [&](uint32_t b) -> uint32_t { return s_lut[b]; };
    cbx_key_value v[CBX_GROUP_MAX_KEYS];
    GrpRec rep{a.data, 0, 0, -1};
    bool ok = false;
    if (w != 0) {
        rep = grp_record(a, s_lut, (int64_t)(w - 1));
        ok = ksf_value(tab, rep, a.start_off, lutf, v);
    }
    const uint64_t km = __ballot(ok), dm = __ballot(w != 0 && !ok);
    uint64_t base = 0;
    if (lane == 0) {
        if (km) base = __hip_atomic_fetch_add(g.hdr + KSF_VALUES, (uint64_t)__popcll(km), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dm) (void)__hip_atomic_fetch_add(g.hdr + KSF_DROPPED, (uint64_t)__popcll(dm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    base = __shfl(base, 0, 64);
    if (!ok) return;
    const uint64_t at = base + (uint64_t)__popcll(km & ((1ull << lane) - 1));
    const int nk = o.n_keys;
    for (int k = 0; k < nk; k++) o.vals[at * (uint64_t)nk + k] = v[k];
    if (o.str_stride > 0) ksf_value_bytes(tab, rep, a.start_off, lutf, o.str_off, o.bytes + at * (uint64_t)o.str_stride);
}
#endif   // CBX_FILTER_HOST_ONLY

}  // namespace cbx
