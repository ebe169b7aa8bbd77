// cbx_gather.h -- the direct projected decode (cbx_plan_options.direct_decode).
//
// A column projection (the host's requiredColumns) leaves a plan with a few fields of a wide record.
// The staged decode kernels fetch a fixed-length tile's whole byte span into LDS whatever the plan
// holds; the filter stage measured that decoding a field per lane straight from HBM beats that when
// few fields are touched (cbx_filter.h, "One input path").  This kernel is that access pattern with
// value stores instead of a compare:
//   one lane per record, 64 records per tile, 4 tiles per workgroup; every op (one per projected
//   field) decodes its field from the record's bytes in HBM -- the SWAR forms on the 8 or 16 bytes
//   that END at the field's end where at least 16 bytes are readable in front of that end, the byte
//   loop otherwise and for the lanes the SWAR form defers (no deferral bitmap, no fixup pass) --
//   and stores the tile's 64 values as whole lines, its validity word from a wave ballot.
//   Strings go to the string-view layout only: values of at most 12 bytes inline in the view,
//   longer ones at 4-byte-aligned positions of the tile's region of the slot (one wave scan).  An
//   EBCDIC / ASCII field of at most 32 bytes is held in registers and composed in the lane's LDS slot.
// Eligible plans: no record walk, no OCCURS, no list layout, no Seg_Id level columns, string columns
// in the view layout (gather_build / cbx_plan_direct_eligible); others run the staged kernels.
//
// The per-record core (gather_numeric, gather_str_locate / _span / _write) is CBX_HD:
// tests/native/gather_host.cpp runs it on the host (CBX_GATHER_HOST_ONLY leaves the kernel out).
// Not part of the hipRTC bundle.
#pragma once

#include <string.h>

#include <string>
#include <vector>

#include "cbx_filter.h"   // FltBytes / flt_load_bytes: a short string field held in registers

namespace cbx {

enum GatherKind : int32_t { G_NUMERIC = 0, G_STRING = 1, G_RECORD_ID = 2, G_FILE_ID = 3 };

// One projected field, pre-resolved by the host: descriptor, fast-path constants, what to do.
struct GatherOp {
    Field f;
    NumOp op;                 // SWAR decoder constants (fast != 0)
    int32_t fast;             // Variant of the SWAR decoder (V_BCD8 / V_BCD16 / V_BIN8 / V_ZONED16), 0: byte loop
    int32_t what;             // GatherKind
};
static_assert(sizeof(GatherOp) % 8 == 0, "GatherOp is a dword struct");

// The plan's field table -> op table.  Returns false (reason in why) when a field is outside what the
// direct kernel decodes.
inline bool gather_build(const cbx_field* fields, int32_t n_fields, std::vector<GatherOp>& out, std::string& why) {
    out.clear();
    for (int i = 0; i < n_fields; i++) {
        const cbx_field& cf = fields[i];
        const std::string at = "field " + std::to_string(i) + ": ";
        if (cf.flags & CBX_F_LIST) { why = at + "list layout"; return false; }
        if (cf.n_dims > 0) { why = at + "inside an OCCURS"; return false; }
        GatherOp g;
        memset(&g, 0, sizeof(g));
        g.f = make_field(cf);
        g.op = make_numop(g.f, 0, cf.offset, nullptr, nullptr, 0);
        const int v = g.f.variant;
        g.fast = (v == V_BCD8 || v == V_BCD16 || v == V_BIN8 || v == V_ZONED16) ? v : 0;
        g.what = v == V_STRING ? G_STRING : v == V_RECORD_ID ? G_RECORD_ID : v == V_FILE_ID ? G_FILE_ID : G_NUMERIC;
        out.push_back(g);
    }
    return true;
}

// 8 bytes at p (any alignment), little-endian
CBX_HD uint64_t gth_le64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// The numeric field of op g of the record at rec (avail bytes, decoded at +start_off, active segment
// seg), decoded exactly as the filter stage's filter_term_true does.  Null when the field reaches past
// the record's end or its segment is not the record's.  head: bytes readable in front of rec (the SWAR
// decoders load the 8 / 16 bytes that END at the field's end); no byte outside [rec - head, rec + avail)
// is read.
CBX_HD Val gather_numeric(const GatherOp& g, const uint8_t* rec, int avail, int64_t head, int start_off, int seg) {
    const Field& f = g.f;
    const bool seg_ok = f.segment < 0 || f.segment == seg;
    const int o = start_off + f.offset;
    Val v = null_val();
    if (seg_ok && o + f.size <= avail) {
        const uint8_t* p = rec + o;
        bool defer = true;
        if (g.fast && head + o + f.size >= 16) {
            defer = false;
            const uint64_t r1 = gth_le64(p + f.size - 8);
            switch (g.fast) {
            case V_BCD8: v = bcd8_raw<0>(g.op, r1); break;
            case V_BCD16: v = bcd16_raw<0>(g.op, r1, gth_le64(p + f.size - 16)); break;
            case V_BIN8: v = bin8_raw<0>(g.op, r1); break;
            default: v = zoned16_raw<0>(g.op, r1, gth_le64(p + f.size - 16), defer); break;
            }
        }
        if (defer) v = decode_numeric(f, p);   // forms the SWAR decoders leave to the byte loop, COMP-1 / COMP-2
    }
    return v;
}

// The string field of op g: false when null (it starts past the record's end, or its segment is not
// the record's); else o = its offset in the record and n = min(size, avail - o) the bytes the record
// holds of it (a short record cuts the value: Primitive.decodeTypeValue).
CBX_HD bool gather_str_locate(const GatherOp& g, int avail, int start_off, int seg, int& o, int& n) {
    const Field& f = g.f;
    o = start_off + f.offset;
    n = 0;
    if (!(f.segment < 0 || f.segment == seg) || o > avail) return false;
    n = f.size < avail - o ? f.size : avail - o;
    return true;
}

// An EBCDIC / ASCII string of at most kFltRegBytes bytes is loaded into registers once (8-byte loads,
// flt_load_bytes): the trim scans, the length pass and the write walk the field four times, and a byte
// load from HBM per step made a string op several times the cost of a numeric one.  Longer fields and
// the other kinds (HEX, RAW, UTF-16) are read through the pointer.
CBX_HD bool gather_str_in_regs(const GatherOp& g) {
    return g.f.size <= kFltRegBytes && (g.f.kind == CBX_K_STRING || g.f.kind == CBX_K_STRING_ASCII);
}

// The kept range of the field's n bytes at p (a pointer or FltBytes) with the UTF-8 length, and its
// sp.utf8_len UTF-8 bytes written to out.
template <typename BP, typename LutFn>
CBX_HD StrSpan gather_str_span(const GatherOp& g, BP p, int n, LutFn lut) {
    const int kind = g.f.kind;
    return string_span(kind, g.f.trim, p, n, [&](uint32_t b) -> uint32_t { return kind == CBX_K_STRING_ASCII ? ascii_lut(b) : lut(b); });
}
template <typename BP, typename LutFn>
CBX_HD void gather_str_write(const GatherOp& g, BP p, const StrSpan& sp, uint8_t* out, LutFn lut) {
    const int kind = g.f.kind;
    string_write(kind, p, sp, out, [&](uint32_t b) -> uint32_t { return kind == CBX_K_STRING_ASCII ? ascii_lut(b) : lut(b); });
}

#ifndef CBX_GATHER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernel (included by cbx_capi.hip after cbx_kernels.hip)
// ------------------------------------------------------------------------------------------
constexpr int kGthThreads = 256;   // 4 waves = 4 tiles per workgroup
constexpr int kGthSlotDwords = 3 * kFltRegBytes / 4 + 1;   // 96 bytes, padded to an odd dword count (LDS banks)

struct GatherArgs {
    const uint8_t* data;
    int64_t n_bytes;
    const int64_t* rec_off;      // framed records / the rows of a selection; nullptr: fixed-length records
    const int32_t* rec_len;
    const int32_t* rec_seg;      // a selection's active segments; nullptr: from the segment map
    const int64_t* rec_id;       // a selection's Record_Ids; nullptr: first_record_id + record index
    const int64_t* rec_id_base;  // cbx_plan_set_record_base, nullptr: 0
    int64_t n;
    int64_t n_tiles;
    int64_t first_record_id;
    int32_t stride;              // fixed-length records
    int32_t start_off;
    int32_t file_id;
    int32_t n_ops;
    int32_t seg_col;             // column receiving the active segment index, -1 none
    int32_t reserved;
    const CBX_CONST GatherOp* ops;
    const CBX_CONST cbx_segment_map* segmap;   // nullptr: none
    const CBX_CONST Field* fields;
    const CBX_CONST DevColumn* cols;
    const CBX_CONST int64_t* view_geo;         // per column: view tile bytes, tiles per data buffer
    const uint32_t* lut;
};

// record i of the source: offset from data and the bytes it may read (never past the data)
__device__ __forceinline__ int gth_record(const GatherArgs& a, int64_t i, int64_t& off) {
    int64_t len;
    if (a.rec_off) { off = a.rec_off[i]; len = a.rec_len[i]; }
    else { off = i * (int64_t)a.stride; len = a.stride; }
    if (off < 0 || off > a.n_bytes) { off = 0; len = 0; }
    if (len > a.n_bytes - off) len = a.n_bytes - off;
    return len < 0 ? 0 : (int)len;
}

// The op table is read through the constant address space with wave-uniform indices (scalar loads),
// the code page from LDS.  Every store of a tile covers whole lines: 64 values / views (st_out), one
// validity word; lanes past n vote 0, so no buffer needs zeroing.
__global__ __launch_bounds__(kGthThreads) void gather_kernel(GatherArgs a) {
    __shared__ uint32_t s_lut[256];
    // a lane's slot for the UTF-8 bytes of a register-path string (<= kFltRegBytes bytes, each at most 3
    // UTF-8 bytes) or the inline bytes (<= 12) of any other
    __shared__ uint32_t s_slot[kGthThreads][kGthSlotDwords];
    for (int i = threadIdx.x; i < 256; i += kGthThreads) s_lut[i] = a.lut[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (kGthThreads / 64) + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;   // whole waves leave (after the only barrier)
    const int64_t i = tile * 64 + lane;
    const bool active = i < a.n;
    int64_t off = 0;
    int avail = 0, seg = -1;
    if (active) {
        avail = gth_record(a, i, off);
        if (a.rec_seg) seg = a.rec_seg[i];
        else if (a.segmap) {
            const int k = segment_key(a.segmap, s_lut, a.fields, a.data + off, avail, a.start_off);
            seg = k >= 0 ? a.segmap->key_segment[k] : -1;
        }
    }
    const uint8_t* rec = a.data + off;
    if (a.seg_col >= 0) {
        const DevColumn c = ldc(a.cols + a.seg_col);
        st_out(gp((int32_t*)c.values) + tile * 64 + lane, seg);
        const uint64_t m = __ballot(active);
        if (lane == 0) gp(c.validity)[tile] = m;
    }
    auto lutf = [&](uint32_t b) -> uint32_t { return s_lut[b]; };
    for (int k = 0; k < a.n_ops; k++) {
        const GatherOp g = ldc(a.ops + k);
        const DevColumn col = ldc(a.cols + g.f.column);
        bool ok = active;
        if (g.what == G_STRING) {
            const int64_t tile_cap = a.view_geo[2 * g.f.column], tiles_per_buf = a.view_geo[2 * g.f.column + 1];
            int o = 0, n = 0;
            ok = active && gather_str_locate(g, avail, a.start_off, seg, o, n);
            const bool regs = gather_str_in_regs(g);   // wave-uniform
            const uint8_t* p = rec + o;
            FltBytes fb{{0, 0, 0, 0}};
            StrSpan sp{0, 0, 0};
            if (ok) {
                if (regs) { fb = flt_load_bytes(p, n, g.f.size, off + o); sp = gather_str_span(g, fb, n, lutf); }
                else sp = gather_str_span(g, p, n, lutf);
            }
            const int len = ok ? sp.utf8_len : 0;
            const bool lng = len > 12;
            uint32_t tot;
            const uint32_t ex = wave_excl_scan32(lng ? (uint32_t)((len + 3) & ~3) : 0u, lane, tot);
            u32x4 v{(uint32_t)len, 0u, 0u, 0u};
            uint32_t* s = s_slot[threadIdx.x];
            // the tile's region of the slot holds 64 values of the column's widest, each rounded to 4 bytes
            uint8_t* dst = col.data + tile * tile_cap + ex;
            if (len > 0 && (regs || !lng)) {   // composed in the lane's LDS slot
                s[0] = s[1] = s[2] = 0u;       // inline bytes are zero padded
                if (regs) gather_str_write(g, fb, sp, (uint8_t*)s, lutf);
                else gather_str_write(g, p, sp, (uint8_t*)s, lutf);
                if (lng)                       // ... and copied out in dwords (the rounding bytes are the slot's)
                    for (int q = 0; 4 * q < len; q++) gp((uint32_t*)dst)[q] = s[q];
                v.y = s[0]; v.z = s[1]; v.w = s[2];
            } else if (lng) {
                gather_str_write(g, p, sp, dst, lutf);
                // the view's prefix: the lane's own first bytes, written above through the vector memory path
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                v.y = *gp((const uint32_t*)dst);
            }
            if (lng) {
                v.z = (uint32_t)(tile >> __builtin_ctzll((unsigned long long)tiles_per_buf));
                v.w = (uint32_t)((tile & (tiles_per_buf - 1)) * tile_cap + ex);
            }
            st_out(gp((u32x4*)col.values) + tile * 64 + lane, v);
        } else {
            Val x = null_val();
            if (g.what == G_NUMERIC) {
                if (active) x = gather_numeric(g, rec, avail, off, a.start_off, seg);
                ok = x.valid;
            } else if (g.what == G_RECORD_ID) {
                const int64_t rid = a.rec_id ? (active ? a.rec_id[i] : 0)
                                             : a.first_record_id + (a.rec_id_base ? *a.rec_id_base : 0) + i;
                x = Val{(uint64_t)rid, 0, true};
            } else {
                x = Val{(uint64_t)(int64_t)a.file_id, 0, true};
            }
            store_w<0>(col.values, tile, lane, x, g.f.out_type);
        }
        const uint64_t m = __ballot(ok);
        if (lane == 0) gp(col.validity)[tile] = m;
    }
}
#endif   // CBX_GATHER_HOST_ONLY

}  // namespace cbx
