// cbx_filter.h -- row filters pushed down in front of the decode (cbx_filter_records).
//
// The reference filters rows after RecordExtractors.extractRecord on a lazy iterator (Spark's
// FilterExec over the relation's RDD); here a decode writes every column of every record, so a
// filter evaluated after it pays the whole output side.  This stage evaluates a predicate table
// (cbx_filter: conjunctive normal form, SQL three-valued logic) on the records' bytes and emits the
// surviving records as a selection for cbx_decode_selected:
//   test: one lane per record, 64 records per tile.  Each term's field is decoded straight from the
//         record's bytes in HBM with the decoders of cbx_decode.h (the SWAR forms on an 8- or
//         16-byte load where the field has one, the byte loop for lanes they defer), compared, the
//         terms combined per group; a wave ballot gives the tile's keep word and its popcount.
//   scan: the library's scan passes over the tile counts (cbx_kernels.hip).
//   emit: lane r of tile t writes its row at base[t] + popcount(keep & lanes below r).
// Strings are compared streaming: the trimmed span as string_span takes it, then each byte's code-page
// entry (table in LDS) yields 0..3 UTF-8 bytes compared with the literal as they are produced --
// no per-lane buffer, no field-size limit.  ENDS_WITH walks the span backwards the same way; CONTAINS tries
// every output byte as a start and verifies it from the span again (flt_str_ends, flt_str_contains).
//
// The per-record evaluator (filter_keep) is CBX_HD: tests/native/filter_host.cpp runs it on the
// host (CBX_FILTER_HOST_ONLY leaves the kernels out).  Not part of the hipRTC bundle.
#pragma once

#include <string.h>

#include <string>

#include "cbx_decode.h"

namespace cbx {

// One term, pre-resolved by the host: the field's descriptor, its fast-path constants, the op.
struct FilterTerm {
    Field f;
    NumOp op;                 // SWAR decoder constants (fast != 0)
    int32_t code;             // cbx_filter_op
    int32_t group;
    int32_t lit_begin, lit_count;
    int32_t is_str;           // compared as UTF-8 bytes (else as a 128-bit value)
    int32_t fast;             // Variant of the SWAR decoder (V_BCD8 / V_BCD16 / V_BIN8 / V_ZONED16), 0: byte loop
    int32_t reserved[2];
};
static_assert(sizeof(FilterTerm) % 8 == 0, "FilterTerm is a dword struct");

struct FilterProg {
    int32_t n_terms, n_lits, pool_bytes, reserved;
    FilterTerm terms[CBX_FILTER_MAX_TERMS];
    cbx_filter_literal lits[CBX_FILTER_MAX_LITERALS];
    uint8_t pool[CBX_FILTER_POOL_BYTES];
};

// cbx_filter + the plan's field table -> FilterProg.  Returns CBX_OK, CBX_E_ARGUMENT (malformed table)
// or CBX_E_UNSUPPORTED (a field the stage does not evaluate), the reason in err.
inline int filter_build(const cbx_field* fields, int32_t n_fields, bool walk_plan, const cbx_filter* fl,
                        FilterProg* out, std::string& err) {
    if (!fl || fl->n_terms < 0 || fl->n_terms > CBX_FILTER_MAX_TERMS || fl->n_literals < 0 ||
        fl->n_literals > CBX_FILTER_MAX_LITERALS || fl->pool_bytes < 0 || fl->pool_bytes > CBX_FILTER_POOL_BYTES) {
        err = "cbx_filter: table sizes out of range";
        return CBX_E_ARGUMENT;
    }
    FilterProg& P = *out;
    memset(&P, 0, sizeof(P));
    P.n_terms = fl->n_terms; P.n_lits = fl->n_literals; P.pool_bytes = fl->pool_bytes;
    for (int i = 0; i < fl->n_literals; i++) {
        const cbx_filter_literal& l = fl->literals[i];
        if (l.str_off < 0 || l.str_len < 0 || (int64_t)l.str_off + l.str_len > fl->pool_bytes) {
            err = "cbx_filter: literal " + std::to_string(i) + " lies outside the pool";
            return CBX_E_ARGUMENT;
        }
        P.lits[i] = l;
    }
    memcpy(P.pool, fl->pool, (size_t)fl->pool_bytes);
    for (int t = 0; t < fl->n_terms; t++) {
        const cbx_filter_term& s = fl->terms[t];
        const std::string at = "cbx_filter: term " + std::to_string(t) + ": ";
        if (s.field < 0 || s.field >= n_fields) { err = at + "field index out of range"; return CBX_E_ARGUMENT; }
        if (s.op < CBX_OP_EQ || s.op > CBX_OP_NOT_CONTAINS) { err = at + "unknown op"; return CBX_E_ARGUMENT; }
        if (t > 0 && s.group < fl->terms[t - 1].group) { err = at + "groups must not decrease"; return CBX_E_ARGUMENT; }
        const bool null_op = s.op == CBX_OP_IS_NULL || s.op == CBX_OP_IS_NOT_NULL;
        const bool set_op = s.op == CBX_OP_IN || s.op == CBX_OP_NOT_IN;
        const bool pre_op = s.op == CBX_OP_STARTS_WITH || s.op == CBX_OP_NOT_STARTS_WITH;
        if (s.lit_count < 0 || (null_op && s.lit_count != 0) || (!null_op && !set_op && s.lit_count != 1) ||
            (s.lit_count > 0 && (s.lit_begin < 0 || (int64_t)s.lit_begin + s.lit_count > fl->n_literals))) {
            err = at + "literal range";
            return CBX_E_ARGUMENT;
        }
        const cbx_field& cf = fields[s.field];
        if (walk_plan) { err = at + "record-walk plan: fields lie at data-dependent offsets"; return CBX_E_UNSUPPORTED; }
        if (cf.n_dims > 0) { err = at + "field inside an OCCURS"; return CBX_E_UNSUPPORTED; }
        bool is_str = false;
        switch (cf.kind) {
        case CBX_K_STRING: case CBX_K_STRING_ASCII: is_str = true; break;
        case CBX_K_BCD: case CBX_K_BINARY: case CBX_K_ZONED: case CBX_K_ASCII_NUM: break;
        case CBX_K_FLOAT: case CBX_K_DOUBLE:
            if (!null_op) { err = at + "comparison on a COMP-1 / COMP-2 field"; return CBX_E_UNSUPPORTED; }
            break;
        case CBX_K_HEX: case CBX_K_RAW: case CBX_K_UTF16_BE: case CBX_K_UTF16_LE:
            err = at + "UTF-16, HEX and RAW fields are not filtered on the GPU";
            return CBX_E_UNSUPPORTED;
        default:
            err = at + "generated columns are not filtered on the GPU";
            return CBX_E_UNSUPPORTED;
        }
        if (pre_op && !is_str) { err = at + "STARTS_WITH on a numeric field"; return CBX_E_ARGUMENT; }
        if (s.op >= CBX_OP_ENDS_WITH && !is_str) {
            err = at + (s.op <= CBX_OP_NOT_ENDS_WITH ? "ENDS_WITH" : "CONTAINS") + " on a numeric field";
            return CBX_E_ARGUMENT;
        }
        FilterTerm& d = P.terms[t];
        d.f = make_field(cf);
        d.op = make_numop(d.f, 0, cf.offset, nullptr, nullptr, 0);
        d.code = s.op; d.group = s.group; d.lit_begin = s.lit_begin; d.lit_count = s.lit_count;
        d.is_str = is_str;
        const int v = d.f.variant;
        d.fast = (v == V_BCD8 || v == V_BCD16 || v == V_BIN8 || v == V_ZONED16) ? v : 0;
    }
    return CBX_OK;
}

// table access on the host (the kernels read the same tables with scalar loads: FilterDevTab)
struct FilterHostTab {
    const FilterProg* p;
    CBX_HD int n_terms() const { return p->n_terms; }
    CBX_HD FilterTerm term(int t) const { return p->terms[t]; }
    CBX_HD cbx_filter_literal lit(int i) const { return p->lits[i]; }
};

// 8 bytes at p (any alignment), little-endian
CBX_HD uint64_t flt_le64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// The column's output value as a signed 128-bit number (hi, lo): int32 / int64 / DEC64 columns hold
// the low 32 / 64 bits of the decoded value.
CBX_HD void flt_widen(const Val& v, int out_type, int64_t& hi, uint64_t& lo) {
    if (out_type == CBX_O_DEC128) { hi = (int64_t)v.hi; lo = v.lo; return; }
    const int64_t x = out_type == CBX_O_I32 ? (int64_t)(int32_t)(uint32_t)v.lo : (int64_t)v.lo;
    lo = (uint64_t)x;
    hi = x >> 63;
}

CBX_HD int flt_cmp128(int64_t ahi, uint64_t alo, int64_t bhi, uint64_t blo) {
    if (ahi != bhi) return ahi < bhi ? -1 : 1;
    if (alo != blo) return alo < blo ? -1 : 1;
    return 0;
}

CBX_HD bool flt_rel(int code, int c) {
    switch (code) {
    case CBX_OP_EQ: return c == 0;
    case CBX_OP_NE: return c != 0;
    case CBX_OP_LT: return c < 0;
    case CBX_OP_LE: return c <= 0;
    case CBX_OP_GT: return c > 0;
    default: return c >= 0;   // CBX_OP_GE
    }
}

// The decoded string (span s of the field bytes p) against a literal of ll bytes, in unsigned byte
// order, as its UTF-8 bytes are produced; starts: the literal is a prefix of the string.
template <typename BP, typename LutFn>
CBX_HD int flt_str_cmp(BP p, const StrSpan& s, const uint8_t* lit, int ll, LutFn lut, bool& starts) {
    int j = 0;
    for (int i = s.begin; i < s.end; i++) {
        const uint32_t e = lut(p[i]);
        const int l = (int)((e >> 24) & 3);
        for (int k = 0; k < l; k++) {
            if (j >= ll) { starts = true; return 1; }
            const uint32_t b = (e >> (8 * k)) & 0xFFu, c = lit[j];
            if (b != c) { starts = false; return b < c ? -1 : 1; }
            j++;
        }
    }
    starts = j >= ll;
    return starts ? 0 : -1;
}

// Is the literal a suffix of the decoded string?  The span is walked backwards, each entry's bytes
// produced last to first and compared with the literal from its end.
template <typename BP, typename LutFn>
CBX_HD bool flt_str_ends(BP p, const StrSpan& s, const uint8_t* lit, int ll, LutFn lut) {
    int j = ll;   // literal bytes still to match
    for (int i = s.end - 1; i >= s.begin && j > 0; i--) {
        const uint32_t e = lut(p[i]);
        for (int k = (int)((e >> 24) & 3) - 1; k >= 0 && j > 0; k--) {
            if (((e >> (8 * k)) & 0xFFu) != lit[j - 1]) return false;
            j--;
        }
    }
    return j == 0;
}

// Do the literal's bytes occur in the decoded string?  Exact for arbitrary literal bytes: every output
// byte is a candidate start, the bytes inside an entry's output included (a literal may begin with the
// continuation bytes of a character), so nothing is assumed of the code-page table.  A candidate whose
// first byte matches is verified by producing the bytes after it again from the span -- the candidate
// after a failed one is the next output byte, so no start is skipped ("aab" in "aaab") and no state of a
// partial match is kept: no per-lane buffer, no failure table.  A verification that runs out of string
// ends the search: no later start has more bytes left.
template <typename BP, typename LutFn>
CBX_HD bool flt_str_contains(BP p, const StrSpan& s, const uint8_t* lit, int ll, LutFn lut) {
    if (ll == 0) return true;
    const uint32_t c0 = lit[0];
    for (int i = s.begin; i < s.end; i++) {
        const uint32_t e = lut(p[i]);
        const int l = (int)((e >> 24) & 3);
        for (int k0 = 0; k0 < l; k0++) {
            if (((e >> (8 * k0)) & 0xFFu) != c0) continue;
            uint32_t ee = e;
            int ii = i, el = l, k = k0 + 1, j = 1;
            while (j < ll) {
                if (k >= el) {
                    if (++ii >= s.end) return false;
                    ee = lut(p[ii]);
                    el = (int)((ee >> 24) & 3);
                    k = 0;
                    continue;
                }
                if (((ee >> (8 * k)) & 0xFFu) != lit[j]) break;
                j++; k++;
            }
            if (j >= ll) return true;
        }
    }
    return false;
}

// A string field of at most kFltRegBytes bytes held in registers: the trim scans and the compare walk
// the field several times, and a byte load from HBM per step made the string term the slowest one
// (3.5 ms per 50 M SYN200 records against 1.1 ms for a COMP-3 term, measured).  Longer fields are read
// through the pointer: no size limit, no per-lane buffer in memory.
constexpr int kFltRegBytes = 32;
struct FltBytes {
    uint64_t q[kFltRegBytes / 8];
    CBX_HD uint32_t operator[](int i) const {
        // All four words are read before one is chosen.  Written as `i < 8 ? q[0] : q[1]` each arm is a load of
        // its own, and with enough callers the compiler merges the arms into ONE load at a variable address:
        // the image then lives in scratch memory (measured: the string term's test pass 1.92 -> 3.28 ms per
        // 50 M SYN200 records).  Selecting among values leaves nothing to merge.
        const uint64_t a = q[0], b = q[1], c = q[2], d = q[3];
        const uint64_t w = i < 16 ? (i < 8 ? a : b) : (i < 24 ? c : d);
        return (uint32_t)(w >> (8 * (i & 7))) & 0xFFu;
    }
};

// bytes [0, n) of p, n <= size <= kFltRegBytes; back: bytes readable in front of p.  Whole words are
// 8-byte loads; the last, partial word is the 8 bytes that END at p + n, shifted down.
CBX_HD FltBytes flt_load_bytes(const uint8_t* p, int n, int size, int64_t back) {
    FltBytes r;
#pragma unroll
    for (int k = 0; k < kFltRegBytes / 8; k++) {
        uint64_t w = 0;
        const int m = n - 8 * k;
        if (8 * k < size) {
            if (m >= 8) {
                w = flt_le64(p + 8 * k);
            } else if (m > 0) {
                if (back + n >= 8) w = flt_le64(p + n - 8) >> (8 * (8 - m));
                else for (int j = 0; j < m; j++) w |= (uint64_t)p[8 * k + j] << (8 * j);
            }
        }
        r.q[k] = w;
    }
    return r;
}

// The kept byte range of an EBCDIC / ASCII string field: string_span (cbx_decode.h) without its pass over
// the span for the UTF-8 length, which a comparison does not need.
template <typename BP, typename LutFn>
CBX_HD StrSpan flt_trim_span(int trim, BP p, int n, LutFn lut) {
    const bool tl = trim == CBX_TRIM_LEFT || trim == CBX_TRIM_BOTH;
    const bool tr = trim == CBX_TRIM_RIGHT || trim == CBX_TRIM_BOTH;
    int b = 0, e = n;
    if (tl) while (b < e && (lut(p[b]) >> 31)) b++;
    if (tr) while (e > b && (lut(p[e - 1]) >> 31)) e--;
    return StrSpan{b, e, 0};
}

// A string term over the field bytes p[0, n): trimmed span, then the literals.
template <typename Tab, typename BP, typename LutFn>
CBX_HD bool flt_str_term(const Tab& tab, const FilterTerm& tm, const uint8_t* pool, BP p, int n, LutFn lutf) {
    const int code = tm.code;
    const StrSpan s = flt_trim_span(tm.f.trim, p, n, lutf);
    if (code >= CBX_OP_ENDS_WITH) {   // suffix / substring: one literal
        const cbx_filter_literal l = tab.lit(tm.lit_begin);
        const bool hit = code <= CBX_OP_NOT_ENDS_WITH ? flt_str_ends(p, s, pool + l.str_off, l.str_len, lutf)
                                                      : flt_str_contains(p, s, pool + l.str_off, l.str_len, lutf);
        return hit == (code == CBX_OP_ENDS_WITH || code == CBX_OP_CONTAINS);
    }
    bool any = false;
    for (int k = 0; k < tm.lit_count; k++) {
        const cbx_filter_literal l = tab.lit(tm.lit_begin + k);
        bool starts;
        const int c = flt_str_cmp(p, s, pool + l.str_off, l.str_len, lutf, starts);
        switch (code) {
        case CBX_OP_IN: case CBX_OP_NOT_IN: any |= c == 0; break;
        case CBX_OP_STARTS_WITH: return starts;
        case CBX_OP_NOT_STARTS_WITH: return !starts;
        default: return flt_rel(code, c);
        }
    }
    return code == CBX_OP_IN ? any : !any;
}

// Is term tm TRUE for the record at rec (avail bytes, decoded at +start_off, active segment seg)?
// Unknown (a null value under a comparison) and false both answer no.  head: bytes readable in
// front of rec (the SWAR decoders load the 8 / 16 bytes that END at the field's end).
template <typename Tab, typename LutFn>
CBX_HD bool filter_term_true(const Tab& tab, const FilterTerm& tm, const uint8_t* pool, const uint8_t* rec, int avail,
                             int64_t head, int start_off, int seg, LutFn lut) {
    const Field& f = tm.f;
    const bool seg_ok = f.segment < 0 || f.segment == seg;
    const int o = start_off + f.offset;
    const int code = tm.code;
    if (tm.is_str) {
        // Primitive.decodeTypeValue: a string starting within the record is cut at its end
        const bool ok = seg_ok && o <= avail;
        if (code == CBX_OP_IS_NULL) return !ok;
        if (code == CBX_OP_IS_NOT_NULL) return ok;
        if (!ok) return false;
        const int n = f.size < avail - o ? f.size : avail - o;
        const uint8_t* p = rec + o;
        const int kind = f.kind;
        auto lutf = [&](uint32_t b) -> uint32_t { return kind == CBX_K_STRING_ASCII ? ascii_lut(b) : lut(b); };
        if (f.size <= kFltRegBytes) return flt_str_term(tab, tm, pool, flt_load_bytes(p, n, f.size, head + o), n, lutf);
        return flt_str_term(tab, tm, pool, p, n, lutf);
    }
    // numerics: null when the field reaches past the record's end
    const bool in = seg_ok && o + f.size <= avail;
    Val v = null_val();
    if (in) {
        const uint8_t* p = rec + o;
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
        if (defer) v = decode_numeric(f, p);   // forms the SWAR decoders leave to the byte loop
    }
    if (code == CBX_OP_IS_NULL) return !v.valid;
    if (code == CBX_OP_IS_NOT_NULL) return v.valid;
    if (!v.valid) return false;
    int64_t hi;
    uint64_t lo;
    flt_widen(v, f.out_type, hi, lo);
    bool any = false;
    for (int k = 0; k < tm.lit_count; k++) {
        const cbx_filter_literal l = tab.lit(tm.lit_begin + k);
        const int c = flt_cmp128(hi, lo, (int64_t)l.hi, l.lo);
        if (code != CBX_OP_IN && code != CBX_OP_NOT_IN) return flt_rel(code, c);
        any |= c == 0;
    }
    return code == CBX_OP_IN ? any : !any;
}

// Does the filter keep the record?  Groups are AND-ed, a group's terms OR-ed; with no NOT node a
// group is true exactly when one of its terms is, so unknown needs no third state here.
template <typename Tab, typename LutFn>
CBX_HD bool filter_keep(const Tab& tab, const uint8_t* pool, const uint8_t* rec, int avail, int64_t head,
                        int start_off, int seg, LutFn lut) {
    const int nt = tab.n_terms();
    bool keep = true, grp = false;
    int cur = 0;
    for (int t = 0; t < nt; t++) {
        const FilterTerm tm = tab.term(t);
        if (t > 0 && tm.group != cur) { keep &= grp; grp = false; }
        cur = tm.group;
        grp |= filter_term_true(tab, tm, pool, rec, avail, head, start_off, seg, lut);
    }
    if (nt > 0) keep &= grp;
    return keep;
}

#ifndef CBX_FILTER_HOST_ONLY
// ------------------------------------------------------------------------------------------
// Kernels (included by cbx_capi.hip after cbx_kernels.hip / cbx_select.h)
// ------------------------------------------------------------------------------------------
constexpr int kFltThreads = 256;   // 4 waves = 4 tiles per workgroup

// the term and literal tables through the constant address space: wave-uniform indices, scalar loads
struct FilterDevTab {
    const CBX_CONST FilterProg* p;
    __device__ __forceinline__ int n_terms() const { return p->n_terms; }
    __device__ __forceinline__ FilterTerm term(int t) const { return ldc(&p->terms[t]); }
    __device__ __forceinline__ cbx_filter_literal lit(int i) const { return ldc(&p->lits[i]); }
};

struct FilterArgs {
    const uint8_t* data;
    int64_t n_bytes;
    const int64_t* rec_off;    // framed records / the rows of a selection; nullptr: fixed-length records
    const int32_t* rec_len;
    const int32_t* rec_seg;    // a selection's active segments; nullptr: from the segment map
    int64_t n;
    int64_t n_tiles;
    int32_t stride;            // fixed-length records
    int32_t start_off;
    const CBX_CONST FilterProg* prog;
    const CBX_CONST cbx_segment_map* segmap;   // nullptr: none
    const CBX_CONST Field* fields;
    const uint32_t* lut;
    uint64_t* keep;            // [n_tiles] keep word of every tile
    uint32_t* counts;          // [n_tiles + 1] kept records per tile (the last entry stays 0)
    int16_t* seg_out;          // [n] active segment of every record, written when it comes from the segment map
};

// record i of the source: base pointer and the bytes it may read (never past the data)
__device__ __forceinline__ int flt_record(const FilterArgs& a, int64_t i, int64_t& off) {
    int64_t len;
    if (a.rec_off) { off = a.rec_off[i]; len = a.rec_len[i]; }
    else { off = i * (int64_t)a.stride; len = a.stride; }
    if (off < 0 || off > a.n_bytes) { off = 0; len = 0; }
    if (len > a.n_bytes - off) len = a.n_bytes - off;
    return len < 0 ? 0 : (int)len;
}

// active segment-redefine index of a record the plan's segment map gives (as sel_emit_kernel)
__device__ __forceinline__ int flt_segment(const FilterArgs& a, const uint32_t* lut, const uint8_t* rec, int avail) {
    if (!a.segmap) return -1;
    const int k = segment_key(a.segmap, lut, a.fields, rec, avail, a.start_off);
    return k >= 0 ? a.segmap->key_segment[k] : -1;
}

// One input path: every lane loads its terms' field bytes straight from HBM.  A second path that first
// staged a fixed-length tile's whole byte span in LDS (coalesced 16-byte loads) was built and measured:
// 3.9 ms against 1.1 ms per 50 M SYN200 records for one COMP-3 term, 5.0 against 2.3 for three terms
// -- it reads every byte where a predicate touches a few cache lines of a record -- so it was dropped.
__global__ __launch_bounds__(kFltThreads) void filter_test_kernel(FilterArgs a) {
    __shared__ uint32_t s_lut[256];
    __shared__ uint8_t s_pool[CBX_FILTER_POOL_BYTES];
    for (int i = threadIdx.x; i < 256; i += kFltThreads) s_lut[i] = a.lut[i];
    const CBX_CONST uint32_t* pw = (const CBX_CONST uint32_t*)a.prog->pool;
    for (int i = threadIdx.x; i < CBX_FILTER_POOL_BYTES / 4; i += kFltThreads) ((uint32_t*)s_pool)[i] = pw[i];
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
        FilterDevTab tab{a.prog};
        keep = filter_keep(tab, s_pool, rec, avail, off, a.start_off, seg, [&](uint32_t b) -> uint32_t { return s_lut[b]; });
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) {
        a.keep[tile] = m;
        a.counts[tile] = (uint32_t)__popcll(m);
    }
}

__global__ __launch_bounds__(kFltThreads) void filter_emit_kernel(FilterArgs a, const int64_t* base, cbx_selection in,
                                                                  int32_t has_in, int32_t n_state, int64_t first_record_id,
                                                                  cbx_selection out) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (kFltThreads / 64) + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;
    const uint64_t m = a.keep[tile];
    if (!((m >> lane) & 1)) return;
    const int64_t i = tile * 64 + lane;
    const int64_t o = base[tile] + __popcll(m & ((1ull << lane) - 1ull));
    if (has_in) {
        out.rec_off[o] = in.rec_off[i];
        out.rec_len[o] = in.rec_len[i];
        out.record_id[o] = in.record_id[i];
        out.segment[o] = in.segment[i];
        if (n_state > 0 && in.seg_state && out.seg_state)
            for (int l = 0; l < n_state; l++) out.seg_state[o * n_state + l] = in.seg_state[i * n_state + l];
        return;
    }
    int64_t off;
    flt_record(a, i, off);
    out.rec_off[o] = a.rec_off ? a.rec_off[i] : off;
    out.rec_len[o] = a.rec_off ? a.rec_len[i] : a.stride;
    out.record_id[o] = first_record_id + i;
    out.segment[o] = a.segmap ? a.seg_out[i] : -1;
}
#endif   // CBX_FILTER_HOST_ONLY

}  // namespace cbx
