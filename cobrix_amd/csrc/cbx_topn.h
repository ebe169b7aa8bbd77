// cbx_topn.h -- Top-N pushdown (cbx_top_n_records): ORDER BY up to four keys LIMIT n, and the plain LIMIT,
// selected from the records' bytes with the row filter of cbx_filter.h fused in front.
//
// The order as one byte string.  A record's COMPOSITE KEY is a byte string compared with memcmp.  Per sort
// key, in order: one null byte (0: NULL under NULLS FIRST, 2: NULL under NULLS LAST, 1: a value; DESC never
// inverts it), then the payload -- zeros for a NULL; a numeric value as big-endian two's complement with
// the sign bit flipped, 4 / 8 / 16 bytes for an int32 / int64-or-DEC64 / DEC128 column; a string as its
// UTF-8 bytes zero-padded to 3 * size followed by one byte holding the UTF-8 length (so "ab" < "ab\0" is
// exact); DESC inverts every payload byte of a value.  The string is zero-padded to a multiple of 8, and one
// more 8-byte word follows: the big-endian source index.  With it all composite keys are distinct.
// Word `level` of that string, read big-endian, is a uint64 whose numeric order is the byte order: topn_word
// computes it without materialising the string (up to 392 bytes) -- a level decodes only the keys that
// overlap its 8 bytes, a numeric key once, a string key by streaming its span through the code page.
//
// Passes (launched by cbx_top_n_records, cbx_capi.hip):
//   key:      grid, LDS (code page + literal pool) and record addressing of filter_test_kernel, lane = record.
//             filter_keep fused; the ballot is the tile's LIVE word (also the initial keep word); every live
//             lane stores word 0 into the workspace, 8 bytes per source record.
//   select:   the need-th smallest word among the candidates (level 0: the live records; later: a tie list),
//             8 bits at a time from the top.  topn_hist_kernel (grid-stride, at most max_workgroups
//             workgroups) counts the words matching the prefix found so far into 256 LDS bins, then adds its
//             non-empty bins to the round's global bins with one integer atomic each -- integer adds commute,
//             so the counts are exact whatever the order.  topn_pick_kernel (one wave) scans the bins, fixes
//             the next digit and updates `need` in the device state block; no host wait between the rounds.
//   classify: candidates with word < T enter the keep words; those with word == T are the tie class: kept
//             whole when exactly `need` of them remain, else left to the next level.
//   tie:      the tie class's indices are appended to a list (one atomic per wave) and word level + 1 of each
//             is computed
//             (the list's order is unspecified and irrelevant: selection is by value, the keep bit by index).
//   count:    popcount of every keep word; then the library's scan and the unchanged filter_emit_kernel.
// The host reads the state block once per level (one wait each) and once the final count.
//
// topn_build, topn_word and the pick step (topn_pick_digit) are host/device: tests/native/topn_host.cpp
// runs them on the host (CBX_FILTER_HOST_ONLY leaves the kernels out).  Not part of the hipRTC bundle.
#pragma once

#include "cbx_group.h"

namespace cbx {

struct TopnKey {
    AggTerm t;                // funcs unused; is_str / fast / wide as for a term
    int32_t flags;            // cbx_sort_flags
    int32_t begin;            // byte offset of the key's null byte in the composite key
    int32_t width;            // payload bytes: 4 / 8 / 16, or 3 * size + 1 for a string
    int32_t reserved;
};
static_assert(sizeof(TopnKey) % 4 == 0, "TopnKey is a dword struct");

struct TopnProg {
    int32_t n_keys;
    int32_t n_words;          // 8-byte words of the keys' bytes; word n_words is the source index
    int32_t reserved[2];
    TopnKey keys[CBX_TOPN_MAX_KEYS];
};

// cbx_sort_order + the plan's field table -> TopnProg.  Status and reason as aggregate_build.
inline int topn_build(const cbx_field* fields, int32_t n_fields, bool walk_plan, const cbx_sort_order* so,
                      TopnProg* out, std::string& err) {
    if (!so || so->n_keys < 0 || so->n_keys > CBX_TOPN_MAX_KEYS) {
        err = "cbx_sort_order: 0 to " + std::to_string(CBX_TOPN_MAX_KEYS) + " sort keys";
        return CBX_E_ARGUMENT;
    }
    TopnProg& P = *out;
    memset(&P, 0, sizeof(P));
    P.n_keys = so->n_keys;
    int32_t pos = 0;
    for (int k = 0; k < so->n_keys; k++) {
        const int fi = so->keys[k].field;
        const std::string at = "cbx_sort_order: key " + std::to_string(k) + ": ";
        if (fi < 0 || fi >= n_fields) { err = at + "field index out of range"; return CBX_E_ARGUMENT; }
        if (so->keys[k].flags & ~(CBX_SORT_DESC | CBX_SORT_NULLS_LAST)) { err = at + "unknown flag bits"; return CBX_E_ARGUMENT; }
        for (int u = 0; u < k; u++)
            if (so->keys[u].field == fi) { err = at + "field repeated"; return CBX_E_ARGUMENT; }
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
            err = at + "COMP-1 / COMP-2 key (NaN ordering is not modelled)";
            return CBX_E_UNSUPPORTED;
        case CBX_K_HEX: case CBX_K_RAW: case CBX_K_UTF16_BE: case CBX_K_UTF16_LE:
            err = at + "UTF-16, HEX and RAW fields are not ordered on the GPU";
            return CBX_E_UNSUPPORTED;
        default:
            err = at + "generated columns are not ordered on the GPU";
            return CBX_E_UNSUPPORTED;
        }
        TopnKey& d = P.keys[k];
        d.t.f = make_field(cf);
        d.t.op = make_numop(d.t.f, 0, cf.offset, nullptr, nullptr, 0);
        d.t.funcs = 0;
        d.t.is_str = is_str;
        const int v = d.t.f.variant;
        d.t.fast = (v == V_BCD8 || v == V_BCD16 || v == V_BIN8 || v == V_ZONED16) ? v : 0;
        d.t.wide = cf.out_type == CBX_O_DEC128;
        d.flags = so->keys[k].flags;
        d.begin = pos;
        d.width = is_str ? 3 * cf.size + 1 : cf.out_type == CBX_O_DEC128 ? 16 : cf.out_type == CBX_O_I32 ? 4 : 8;
        pos += 1 + d.width;
    }
    P.n_words = (pos + 7) / 8;
    return CBX_OK;
}

// composite-key words that hold bytes of key k
inline int topn_words_of_key(const TopnProg& P, int k) {
    const TopnKey& d = P.keys[k];
    return (d.begin + d.width) / 8 - d.begin / 8 + 1;
}

struct TopnHostTab {
    const TopnProg* p;
    CBX_HD int n_keys() const { return p->n_keys; }
    CBX_HD int n_words() const { return p->n_words; }
    CBX_HD TopnKey key(int k) const { return p->keys[k]; }
};

// Key k's bytes that fall into the window [w0, w0 + 8) of the composite key, at their big-endian places.
template <typename LutFn>
CBX_HD uint64_t topn_key_bits(const TopnKey& k, int w0, const GrpRec& r, int start_off, LutFn lut) {
    const int rel0 = w0 - k.begin;          // key-relative position of the window's first byte
    const bool desc = (k.flags & CBX_SORT_DESC) != 0;
    const uint32_t null_byte = (k.flags & CBX_SORT_NULLS_LAST) ? 2u : 0u;
    uint64_t word = 0;
    // byte b of the key (0: the null byte, 1 + q: payload byte q) into the window
    auto put = [&](int rel, uint32_t b) {
        const int j = rel - rel0;
        if (j >= 0 && j < 8) word |= (uint64_t)(b & 0xFFu) << (56 - 8 * j);
    };
    const uint32_t inv = desc ? 0xFFu : 0u;
    if (k.t.is_str) {
        FltBytes b;
        StrSpan s;
        if (!grp_str_load(k.t, r, start_off, lut, b, s)) { put(0, null_byte); return word; }
        put(0, 1u);
        const int kind = k.t.f.kind;
        int j = 0;
        for (int i = s.begin; i < s.end; i++) {
            uint32_t e = grp_lut(kind, lut, b[i]);
            for (int l = (int)((e >> 24) & 3); l > 0; l--) { put(1 + j, (e & 0xFFu) ^ inv); e >>= 8; j++; }
        }
        if (desc) {   // the padding of a value inverts with it
            for (int q = 0; q < 8; q++) {
                const int rel = rel0 + q;
                if (rel >= 1 + j && rel < k.width) put(rel, 0xFFu);
            }
        }
        put(k.width, (uint32_t)j ^ inv);    // payload byte width - 1: the UTF-8 length
        return word;
    }
    int64_t hi;
    uint64_t lo;
    if (!agg_value(k.t, r.rec, r.avail, r.head, start_off, r.seg, hi, lo)) { put(0, null_byte); return word; }
    put(0, 1u);
    // the payload as a 128-bit big-endian number, left-aligned: (ph, pl)
    uint64_t ph, pl = 0;
    if (k.width == 16) { ph = (uint64_t)hi ^ 0x8000000000000000ull; pl = lo; }
    else if (k.width == 8) ph = lo ^ 0x8000000000000000ull;
    else ph = ((uint64_t)(uint32_t)lo ^ 0x80000000ull) << 32;
    if (desc) { ph = ~ph; pl = ~pl; }
    for (int q = 0; q < 8; q++) {
        const int p = rel0 + q - 1;         // payload byte index of window byte q
        if (p < 0 || p >= k.width) continue;
        const uint64_t src = p < 8 ? ph >> (56 - 8 * p) : pl >> (56 - 8 * (p - 8));
        word |= (src & 0xFFull) << (56 - 8 * q);
    }
    return word;
}

// Word `level` of record r's composite key; word n_words is the source index.
template <typename Tab, typename LutFn>
CBX_HD uint64_t topn_word(const Tab& tab, int level, const uint8_t* rec, int avail, int64_t head, int start_off, int seg,
                          int64_t index, LutFn lut) {
    static_assert(CBX_TOPN_MAX_KEYS == 4, "the keys are written out one by one");
    if (level >= tab.n_words()) return (uint64_t)index;
    const GrpRec r{rec, avail, head, seg};
    const int w0 = 8 * level, nk = tab.n_keys();
    uint64_t word = 0;
    for (int k = 0; k < nk; k++) {
        const TopnKey key = tab.key(k);
        if (key.begin < w0 + 8 && key.begin + 1 + key.width > w0) word |= topn_key_bits(key, w0, r, start_off, lut);
    }
    return word;
}

// One round of the select over n bin counts (the kernel: a lane's 4 bins; the host: all 256): the bin holding
// the need-th smallest (1-based) of the counted words and how many lie below it.  total >= need >= 1.
CBX_HD int topn_pick_digit(const uint32_t* bins, int n, uint64_t need, uint64_t& below) {
    uint64_t acc = 0;
    for (int d = 0; d < n; d++) {
        if (acc + bins[d] >= need) { below = acc; return d; }
        acc += bins[d];
    }
    below = acc;
    return n - 1;   // (not reached when total >= need)
}

// The device state block of a call (64-bit words), zeroed before the first level.
enum TopnState {
    TS_PREFIX = 0,     // the digits fixed so far, at their places; after round 7 the threshold T
    TS_NEED = 1,       // rows still to take among the candidates matching the prefix
    TS_TIES = 2,       // after round 7: candidates equal to T
    TS_ALL = 3,        // level 0: need >= live, every live record is kept
    TS_TOTAL = 4,      // candidates of this level (level 0: the live records)
    TS_LIST = 5,       // append cursor of the next level's tie list
    TS_WORDS = 8
};

#ifndef CBX_FILTER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernels (included by cbx_capi.hip after cbx_group.h)
// ------------------------------------------------------------------------------------------
constexpr int kTopnThreads = 256;

struct TopnDevTab {
    const CBX_CONST TopnProg* p;
    __device__ __forceinline__ int n_keys() const { return p->n_keys; }
    __device__ __forceinline__ int n_words() const { return p->n_words; }
    __device__ __forceinline__ TopnKey key(int k) const { return ldc(&p->keys[k]); }
};

struct TopnArgs {
    FilterArgs src;                        // the three sources of the filter stage; keep / counts / seg_out as there
    const CBX_CONST TopnProg* topn;
    int32_t has_filter;
    int32_t want_words;                    // 0: limit >= n_rec, the keep words are the live words
    uint64_t* live;                        // [n_tiles] records the filter kept
    uint64_t* words;                       // [n] level-0 word of every live record
};

// the candidates of one select level
struct TopnCand {
    const uint64_t* words;                 // level 0: [n] by record; later: [count] by list position
    const uint64_t* live;                  // level 0: the live words; nullptr: a tie list
    const int32_t* list;                   // later levels: record index of every candidate
    int64_t count;                         // level 0: n; later: the list's length
    uint64_t* state;                       // TopnState
    uint32_t* bins;                        // [8][256] one set of global bins per round
};

__global__ __launch_bounds__(kFltThreads) void topn_key_kernel(TopnArgs g) {
    __shared__ uint32_t s_lut[256];
    __shared__ uint8_t s_pool[CBX_FILTER_POOL_BYTES];
    const FilterArgs& a = g.src;
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
            a.seg_out[i] = (int16_t)seg;   // the tie and emit passes take it from here
        }
        auto lutf = [&](uint32_t b) -> uint32_t { return s_lut[b]; };
        keep = true;
        if (g.has_filter) {
            FilterDevTab tab{a.prog};
            keep = filter_keep(tab, s_pool, rec, avail, off, a.start_off, seg, lutf);
        }
        if (keep && g.want_words) {
            TopnDevTab tt{g.topn};
            g.words[i] = topn_word(tt, 0, rec, avail, off, a.start_off, seg, i, lutf);
        }
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) {
        g.live[tile] = m;
        a.keep[tile] = m;
    }
}

// Round `round` of a level: candidates whose top 8 * round bits equal the prefix, counted by their next 8 bits.
__global__ __launch_bounds__(kTopnThreads) void topn_hist_kernel(TopnCand c, int32_t round) {
    __shared__ uint32_t s_bins[256];
    s_bins[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    if (c.state[TS_ALL] == 0) {            // (uniform: written by the round-0 pick, before this launch)
        const uint64_t prefix = c.state[TS_PREFIX];
        const int shift = 56 - 8 * round;
        const uint64_t mask = round == 0 ? 0ull : ~0ull << (64 - 8 * round);
        const int64_t step = (int64_t)gridDim.x * kTopnThreads;
        // whole waves iterate together: the shuffles below need every lane
        for (int64_t base = (int64_t)blockIdx.x * kTopnThreads + (threadIdx.x & ~63); base < c.count; base += step) {
            const int64_t i = base + lane;
            bool match = false;
            int d = 0;
            if (i < c.count && (!c.live || ((c.live[i >> 6] >> (i & 63)) & 1))) {
                const uint64_t w = c.words[i];
                match = ((w ^ prefix) & mask) == 0;
                d = (int)((w >> shift) & 0xFF);
            }
            const uint64_t act = __ballot(match);
            if (act == 0) continue;
            const int leader = __ffsll((long long)act) - 1;
            const int d0 = __shfl(d, leader, 64);
            const uint64_t same = __ballot(match && d == d0);
            if (same == act) {             // one digit in the whole wave (constant and low-cardinality keys)
                if (lane == leader) atomicAdd(&s_bins[d0], (uint32_t)__popcll(act));
            } else if (match) {
                atomicAdd(&s_bins[d], 1u);
            }
        }
    }
    __syncthreads();
    const uint32_t v = s_bins[threadIdx.x];
    if (v) atomicAdd(&c.bins[round * 256 + threadIdx.x], v);
}

// One wave: lane l owns bins 4l .. 4l + 3 of the round.
__global__ __launch_bounds__(64) void topn_pick_kernel(TopnCand c, int32_t round, int32_t level) {
    const int lane = threadIdx.x;
    if (c.state[TS_ALL] != 0) return;
    const uint32_t* bins = c.bins + round * 256;
    const uint32_t b0 = bins[4 * lane], b1 = bins[4 * lane + 1], b2 = bins[4 * lane + 2], b3 = bins[4 * lane + 3];
    const uint64_t own = (uint64_t)b0 + b1 + b2 + b3;
    uint64_t incl = own;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, m, 64);
        const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), m, 64);
        if (lane >= m) incl += ((uint64_t)hi << 32) | lo;
    }
    const uint64_t need = c.state[TS_NEED];
    const uint64_t total = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(incl >> 32), 63, 64) << 32) |
                           (uint32_t)__shfl((int)(uint32_t)incl, 63, 64);
    if (round == 0) {
        if (lane == 0) c.state[TS_TOTAL] = total;
        if (level == 0 && need >= total) {         // limit >= live: everything live is kept, no select
            if (lane == 0) c.state[TS_ALL] = 1;
            return;
        }
    }
    const uint64_t hit = __ballot(incl >= need);   // total >= need >= 1: not empty
    const int owner = __ffsll((long long)hit) - 1;
    if (lane != owner) return;
    const uint32_t b[4] = {b0, b1, b2, b3};
    const uint64_t before = incl - own;    // counted in the lanes below
    uint64_t below;
    const int d = topn_pick_digit(b, 4, need - before, below);
    c.state[TS_PREFIX] |= (uint64_t)(4 * lane + d) << (56 - 8 * round);
    c.state[TS_NEED] = need - before - below;
    if (round == 7) c.state[TS_TIES] = b[d];
}

__device__ __forceinline__ bool topn_take(const uint64_t* state, uint64_t w) {
    if (state[TS_ALL]) return true;
    const uint64_t t = state[TS_PREFIX];
    return w < t || (w == t && state[TS_TIES] == state[TS_NEED]);
}

// Level 0: the keep word of every tile, whole.
__global__ __launch_bounds__(kTopnThreads) void topn_classify_tiles_kernel(TopnCand c, int64_t n_tiles, uint64_t* keep) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kTopnThreads / 64);
    for (int64_t tile = (int64_t)blockIdx.x * (kTopnThreads / 64) + (threadIdx.x >> 6); tile < n_tiles; tile += waves) {
        const int64_t i = tile * 64 + lane;
        bool k = false;
        if (i < c.count && ((c.live[tile] >> lane) & 1)) k = topn_take(c.state, c.words[i]);
        const uint64_t m = __ballot(k);
        if (lane == 0) keep[tile] = m;
    }
}

// Later levels: the chosen members of the tie list enter their tiles' keep words.
__global__ __launch_bounds__(kTopnThreads) void topn_classify_list_kernel(TopnCand c, uint64_t* keep) {
    const int64_t step = (int64_t)gridDim.x * kTopnThreads;
    for (int64_t j = (int64_t)blockIdx.x * kTopnThreads + threadIdx.x; j < c.count; j += step) {
        if (!topn_take(c.state, c.words[j])) continue;
        const int64_t i = c.list[j];
        atomicOr((unsigned long long*)&keep[i >> 6], 1ull << (i & 63));
    }
}

// The tie class of level `level` - 1 (candidates equal to T) becomes the next level's list, with word `level`.
__global__ __launch_bounds__(kTopnThreads) void topn_tie_kernel(TopnArgs g, TopnCand c, int32_t level, int64_t cap,
                                                                int32_t* list_out, uint64_t* words_out) {
    __shared__ uint32_t s_lut[256];
    const FilterArgs& a = g.src;
    for (int i = threadIdx.x; i < 256; i += kTopnThreads) s_lut[i] = a.lut[i];
    __syncthreads();
    const uint64_t t = c.state[TS_PREFIX];
    const int lane = threadIdx.x & 63;
    const int64_t step = (int64_t)gridDim.x * kTopnThreads;
    // whole waves iterate together: one append per wave (the ballot's popcount), not one per record -- a class
    // of millions of records would otherwise queue that many atomics on one address
    for (int64_t base = (int64_t)blockIdx.x * kTopnThreads + (threadIdx.x & ~63); base < c.count; base += step) {
        const int64_t j = base + lane;
        const bool hit = j < c.count && (!c.live || ((c.live[j >> 6] >> (j & 63)) & 1)) && c.words[j] == t;
        const uint64_t m = __ballot(hit);
        if (m == 0) continue;
        const int leader = __ffsll((long long)m) - 1;
        unsigned long long first = 0;
        if (lane == leader) first = atomicAdd((unsigned long long*)&c.state[TS_LIST], (unsigned long long)__popcll(m));
        first = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(first >> 32), leader, 64) << 32) |
                (uint32_t)__shfl((int)(uint32_t)first, leader, 64);
        if (!hit) continue;
        const int64_t i = c.live ? j : (int64_t)c.list[j];
        const int64_t o = (int64_t)first + __popcll(m & ((1ull << lane) - 1ull));
        if (o >= cap) continue;            // (not reached: cap is the counted size of the class)
        int64_t off;
        const int avail = flt_record(a, i, off);
        const uint8_t* rec = a.data + off;
        const int seg = a.rec_seg ? a.rec_seg[i] : a.segmap ? (int)a.seg_out[i] : -1;
        TopnDevTab tt{g.topn};
        list_out[o] = (int32_t)i;
        words_out[o] = topn_word(tt, level, rec, avail, off, a.start_off, seg, i, [&](uint32_t b) -> uint32_t { return s_lut[b]; });
    }
}

__global__ __launch_bounds__(kTopnThreads) void topn_count_kernel(const uint64_t* keep, int64_t n_tiles, uint32_t* counts) {
    const int64_t t = (int64_t)blockIdx.x * kTopnThreads + threadIdx.x;
    if (t < n_tiles) counts[t] = (uint32_t)__popcll(keep[t]);
}
#endif   // CBX_FILTER_HOST_ONLY

}  // namespace cbx
