// Stand-alone sanitizer driver for the filter stage's host evaluator (filter_host.cpp): random records in
// heap buffers of exactly n * stride bytes -- strides that cut records inside and in front of the
// predicate fields included -- through every op and decoder kind, so an out-of-bounds read or undefined
// arithmetic in the evaluator (the SWAR decoders' 8- and 16-byte loads that END at a field's end, the
// streaming string compare) is reported by AddressSanitizer / UBSan.  Build and run on a CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -I../../include -I../../cobrix_amd/csrc filter_host.cpp filter_host_main.cpp -o filter_host_check
//   ./filter_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cobrix_hip.h"

extern "C" int cbxh_filter_fixed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                 const uint32_t* lut, const uint8_t* data, int64_t n_rec, int32_t stride,
                                 int32_t start_off, int32_t segment, uint8_t* keep, char* err, int32_t err_cap);

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
    // a 64-byte layout: binary, COMP-3 (8 and 16 bytes), zoned, ASCII number, EBCDIC-table string, ASCII string
    std::vector<cbx_field> fields = {
        field(CBX_K_BINARY, CBX_O_I32, 0, 4, 9, 0, 9, 0, CBX_F_SIGNED | CBX_F_BIG_ENDIAN | CBX_F_INTEGRAL, -1),
        field(CBX_K_BCD, CBX_O_DEC64, 4, 8, 15, 2, 15, 2, CBX_F_SIGNED, -1),
        field(CBX_K_BCD, CBX_O_DEC128, 12, 16, 30, 5, 30, 5, CBX_F_SIGNED, -1),
        field(CBX_K_ZONED, CBX_O_I32, 28, 9, 9, 0, 9, 0, CBX_F_SIGNED | CBX_F_INTEGRAL, -1),
        field(CBX_K_ASCII_NUM, CBX_O_I32, 37, 5, 5, 0, 5, 0, CBX_F_INTEGRAL, -1),
        field(CBX_K_STRING, CBX_O_STRING, 42, 12, 0, 0, 0, 0, 0, -1),
        field(CBX_K_STRING_ASCII, CBX_O_STRING, 54, 10, 0, 0, 0, 0, 0, 0),
        field(CBX_K_DOUBLE, CBX_O_F64, 0, 8, 0, 0, 0, 0, 0, -1),
    };
    uint32_t lut[256];
    for (int b = 0; b < 256; b++) {
        // one, two and three byte entries, some trimmable, some with no output
        const int len = b % 7 == 0 ? 0 : b % 5 == 0 ? 3 : b % 3 == 0 ? 2 : 1;
        lut[b] = (uint32_t)(0x41 + b % 26) | 0x8200u | 0xA30000u | ((uint32_t)len << 24) | (b % 11 == 0 ? 0x80000000u : 0u);
    }
    const int n = 512;
    long kept = 0, calls = 0;
    for (int stride : {64, 63, 55, 50, 43, 42, 41, 30, 20, 12, 5, 3, 1}) {
        uint8_t* data = (uint8_t*)malloc((size_t)n * stride);
        for (int i = 0; i < n * stride; i++) {
            const uint32_t r = rnd();
            // mostly digits / packed digits / zoned digits, some arbitrary bytes
            data[i] = r % 16 == 0 ? (uint8_t)(r >> 8) : r % 3 == 0 ? (uint8_t)(0xF0 | ((r >> 8) % 10))
                      : r % 3 == 1 ? (uint8_t)((((r >> 8) % 10) << 4) | ((r >> 12) % 10 == 0 ? 0xC : (r >> 12) % 10))
                                   : (uint8_t)('0' + (r >> 8) % 10);
        }
        uint8_t* keep = (uint8_t*)malloc(n);
        for (int fi = 0; fi < (int)fields.size(); fi++) {
            for (int op = CBX_OP_EQ; op <= CBX_OP_NOT_STARTS_WITH; op++) {
                const bool is_str = fields[fi].out_type == CBX_O_STRING;
                const bool null_op = op == CBX_OP_IS_NULL || op == CBX_OP_IS_NOT_NULL;
                if ((op >= CBX_OP_STARTS_WITH && !is_str) || (fields[fi].kind == CBX_K_DOUBLE && !null_op)) continue;
                cbx_filter fl;
                memset(&fl, 0, sizeof fl);
                fl.n_terms = 2; fl.n_literals = 3; fl.pool_bytes = 6;
                memcpy(fl.pool, "ABCABD", 6);
                for (int k = 0; k < 3; k++) {
                    fl.literals[k].lo = (uint64_t)(int64_t)((int)(rnd() % 2001) - 1000);
                    fl.literals[k].hi = (uint64_t)((int64_t)fl.literals[k].lo >> 63);
                    fl.literals[k].str_off = k; fl.literals[k].str_len = 1 + k;
                }
                fl.terms[0].field = fi; fl.terms[0].op = op; fl.terms[0].group = 0;
                fl.terms[0].lit_begin = 0;
                fl.terms[0].lit_count = null_op ? 0 : (op == CBX_OP_IN || op == CBX_OP_NOT_IN) ? 3 : 1;
                fl.terms[1].field = 0; fl.terms[1].op = CBX_OP_IS_NOT_NULL; fl.terms[1].group = 0;   // OR-ed
                char err[256];
                for (int seg = -1; seg <= 0; seg++) {
                    const int rc = cbxh_filter_fixed(fields.data(), (int)fields.size(), 0, &fl, lut, data, n, stride, 0,
                                                     seg, keep, err, sizeof err);
                    if (rc != CBX_OK) { fprintf(stderr, "field %d op %d: %d %s\n", fi, op, rc, err); return 1; }
                    for (int i = 0; i < n; i++) kept += keep[i];
                    calls++;
                }
            }
        }
        free(keep);
        free(data);
    }
    printf("filter host check: %ld calls, %ld rows kept, no sanitizer report\n", calls, kept);
    return 0;
}
