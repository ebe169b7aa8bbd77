// Stand-alone sanitizer driver for the aggregate stage's host part (aggregate_host.cpp): random records in
// heap buffers of exactly n * stride bytes -- strides that cut records inside and in front of the
// aggregated fields included -- through every function on every accepted decoder kind, with and without
// a fused filter, so an out-of-bounds read (the SWAR decoders' 8- and 16-byte loads that END at a field's
// end) or undefined arithmetic (the 192-bit limb sums, the 128-bit min / max) is reported by
// AddressSanitizer / UBSan.  Every result is also computed as one part and as seven merged parts, which
// must agree bit for bit (agg_merge is associative and the sums are exact).  Build and run on a CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -I../../include -I../../cobrix_amd/csrc aggregate_host.cpp aggregate_host_main.cpp -o aggregate_host_check
//   ./aggregate_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cobrix_hip.h"

extern "C" int cbxh_aggregate_fixed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                    const cbx_aggregate* ag, const uint32_t* lut, const uint8_t* data, int64_t n_rec,
                                    int32_t stride, int32_t start_off, int32_t segment, int32_t n_parts,
                                    cbx_aggregate_result* out, char* err, int32_t err_cap);

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

static cbx_field field(int kind, int out, int off, int size, int prec, int scale, int out_p, int out_s, int flags, int seg) {
    cbx_field f;
    memset(&f, 0, sizeof f);
    f.kind = kind; f.out_type = out; f.offset = off; f.size = size; f.precision = prec; f.scale = scale;
    f.out_precision = out_p; f.out_scale = out_s; f.flags = flags; f.trim = CBX_TRIM_BOTH; f.segment = seg; f.column = 0;
    return f;
}

int main() {
    // a 72-byte layout: binary (4 and 8 bytes), COMP-3 (8 and 16 bytes, 20 bytes: 38 digits), zoned, ASCII
    // number, EBCDIC-table string, ASCII string (under a segment redefine), COMP-2
    std::vector<cbx_field> fields = {
        field(CBX_K_BINARY, CBX_O_I32, 0, 4, 9, 0, 9, 0, CBX_F_SIGNED | CBX_F_BIG_ENDIAN | CBX_F_INTEGRAL, -1),
        field(CBX_K_BCD, CBX_O_DEC64, 4, 8, 15, 2, 15, 2, CBX_F_SIGNED, -1),
        field(CBX_K_BCD, CBX_O_DEC128, 12, 16, 30, 5, 30, 5, CBX_F_SIGNED, -1),
        field(CBX_K_ZONED, CBX_O_I32, 28, 9, 9, 0, 9, 0, CBX_F_SIGNED | CBX_F_INTEGRAL, -1),
        field(CBX_K_ASCII_NUM, CBX_O_I32, 37, 5, 5, 0, 5, 0, CBX_F_INTEGRAL, -1),
        field(CBX_K_STRING, CBX_O_STRING, 42, 12, 0, 0, 0, 0, 0, -1),
        field(CBX_K_STRING_ASCII, CBX_O_STRING, 54, 10, 0, 0, 0, 0, 0, 0),
        field(CBX_K_DOUBLE, CBX_O_F64, 0, 8, 0, 0, 0, 0, 0, -1),
        field(CBX_K_BINARY, CBX_O_I64, 64, 8, 18, 0, 18, 0, CBX_F_SIGNED | CBX_F_BIG_ENDIAN | CBX_F_INTEGRAL, -1),
        field(CBX_K_BCD, CBX_O_DEC128, 44, 20, 38, 0, 38, 0, CBX_F_SIGNED | CBX_F_INTEGRAL, -1),
        field(CBX_K_ZONED, CBX_O_DEC128, 30, 20, 20, 2, 20, 2, CBX_F_SIGNED, 0),
    };
    uint32_t lut[256];
    for (int b = 0; b < 256; b++) {
        const int len = b % 7 == 0 ? 0 : b % 5 == 0 ? 3 : b % 3 == 0 ? 2 : 1;
        lut[b] = (uint32_t)(0x41 + b % 26) | 0x8200u | 0xA30000u | ((uint32_t)len << 24) | (b % 11 == 0 ? 0x80000000u : 0u);
    }
    const int n = 512;
    long calls = 0;
    long long rows = 0, values = 0;
    for (int stride : {72, 71, 64, 63, 55, 50, 43, 42, 41, 30, 20, 12, 5, 3, 1}) {
        uint8_t* data = (uint8_t*)malloc((size_t)n * stride);
        for (int i = 0; i < n * stride; i++) {
            const uint32_t r = rnd();
            // mostly digits / packed digits / zoned digits / nines, some arbitrary bytes
            data[i] = r % 16 == 0 ? (uint8_t)(r >> 8) : r % 16 == 1 ? (uint8_t)0x99 : r % 3 == 0 ? (uint8_t)(0xF0 | ((r >> 8) % 10))
                      : r % 3 == 1 ? (uint8_t)((((r >> 8) % 10) << 4) | ((r >> 12) % 10 == 0 ? 0xC : (r >> 12) % 10))
                                   : (uint8_t)('0' + (r >> 8) % 10);
        }
        for (int fi = 0; fi < (int)fields.size(); fi++) {
            const bool count_only = fields[fi].out_type == CBX_O_STRING || fields[fi].kind == CBX_K_DOUBLE;
            for (int funcs = 1; funcs <= 15; funcs++) {
                if (count_only && funcs != CBX_AGG_COUNT) continue;
                cbx_aggregate ag;
                memset(&ag, 0, sizeof ag);
                ag.n_terms = 2;
                ag.terms[0].field = fi; ag.terms[0].funcs = funcs;
                ag.terms[1].field = (fi + 1) % 5; ag.terms[1].funcs = 15;   // (fields 0..4 take every function)
                if (ag.terms[1].field == fi) ag.n_terms = 1;
                cbx_filter fl;
                memset(&fl, 0, sizeof fl);
                fl.n_terms = 1; fl.n_literals = 1;
                fl.literals[0].lo = (uint64_t)(int64_t)((int)(rnd() % 2001) - 1000);
                fl.literals[0].hi = (uint64_t)((int64_t)fl.literals[0].lo >> 63);
                fl.terms[0].field = 0; fl.terms[0].op = CBX_OP_GE; fl.terms[0].lit_count = 1;
                char err[256];
                for (int seg = -1; seg <= 0; seg++) {
                    for (int with_filter = 0; with_filter <= 1; with_filter++) {
                        cbx_aggregate_result one, many;
                        for (int parts : {1, 7}) {
                            const int rc = cbxh_aggregate_fixed(fields.data(), (int)fields.size(), 0, with_filter ? &fl : nullptr,
                                                                &ag, lut, data, n, stride, 0, seg, parts,
                                                                parts == 1 ? &one : &many, err, sizeof err);
                            if (rc != CBX_OK) { fprintf(stderr, "field %d funcs %d: %d %s\n", fi, funcs, rc, err); return 1; }
                            calls++;
                        }
                        if (memcmp(&one, &many, sizeof one) != 0) {
                            fprintf(stderr, "field %d funcs %d stride %d: 1 part and 7 merged parts differ\n", fi, funcs, stride);
                            return 1;
                        }
                        rows += one.n_rows;
                        values += one.values[0].count;
                    }
                }
            }
        }
        free(data);
    }
    printf("aggregate host check: %ld calls, %lld rows, %lld values, no sanitizer report\n", calls, rows, values);
    return 0;
}
