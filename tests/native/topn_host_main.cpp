// Stand-alone sanitizer driver for the Top-N stage's host part (topn_host.cpp): random records in heap buffers
// of exactly n * stride bytes -- strides that cut records inside and in front of the key fields included --
// through every accepted key kind, every flag set, one to four keys, with and without a fused filter, so an
// out-of-bounds read (the SWAR decoders' 8- and 16-byte loads that END at a field's end, the register load of a
// string key) or undefined arithmetic (the window shifts of topn_word, the sign flips) is reported by
// AddressSanitizer / UBSan.  Every result is also checked against a direct comparison of the composite keys the
// shim returns: the chosen rows are the `limit` smallest keys.  Build and run on a CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -I../../include -I../../cobrix_amd/csrc topn_host.cpp topn_host_main.cpp -o topn_host_check
//   ./topn_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "cobrix_hip.h"

extern "C" int cbxh_topn_words(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_sort_order* so,
                               const uint32_t* lut, const uint8_t* data, int64_t n_bytes, const int64_t* rec_off,
                               const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec, int32_t stride,
                               int32_t start_off, int32_t segment, uint64_t* out_words, int64_t out_cap,
                               int32_t* levels_total, int32_t* words_per_key, char* err, int32_t err_cap);
extern "C" int cbxh_topn_select(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                const cbx_sort_order* so, const uint32_t* lut, const uint8_t* data, int64_t n_bytes,
                                const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec,
                                int32_t stride, int32_t start_off, int32_t segment, int64_t limit, int64_t* out_idx,
                                int64_t* n_out, cbx_topn_info* info, char* err, int32_t err_cap);

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
    // a 72-byte layout: binary (2, 4 and 8 bytes), COMP-3 (8 and 16 bytes, 20 bytes: 38 digits), zoned, ASCII
    // number, EBCDIC-table string of 12 and of 32 bytes, ASCII string (under a segment redefine)
    std::vector<cbx_field> fields = {
        field(CBX_K_BINARY, CBX_O_I32, 0, 4, 9, 0, 9, 0, CBX_F_SIGNED | CBX_F_BIG_ENDIAN | CBX_F_INTEGRAL, -1),
        field(CBX_K_BCD, CBX_O_DEC64, 4, 8, 15, 2, 15, 2, CBX_F_SIGNED, -1),
        field(CBX_K_BCD, CBX_O_DEC128, 12, 16, 30, 5, 30, 5, CBX_F_SIGNED, -1),
        field(CBX_K_ZONED, CBX_O_I32, 28, 9, 9, 0, 9, 0, CBX_F_SIGNED | CBX_F_INTEGRAL, -1),
        field(CBX_K_ASCII_NUM, CBX_O_I32, 37, 5, 5, 0, 5, 0, CBX_F_INTEGRAL, -1),
        field(CBX_K_STRING, CBX_O_STRING, 42, 12, 0, 0, 0, 0, 0, -1),
        field(CBX_K_STRING_ASCII, CBX_O_STRING, 54, 10, 0, 0, 0, 0, 0, 0),
        field(CBX_K_BINARY, CBX_O_I64, 64, 8, 18, 0, 18, 0, CBX_F_SIGNED | CBX_F_BIG_ENDIAN | CBX_F_INTEGRAL, -1),
        field(CBX_K_BCD, CBX_O_DEC128, 44, 20, 38, 0, 38, 0, CBX_F_SIGNED | CBX_F_INTEGRAL, -1),
        field(CBX_K_ZONED, CBX_O_DEC128, 30, 20, 20, 2, 20, 2, CBX_F_SIGNED, 0),
        field(CBX_K_STRING, CBX_O_STRING, 40, 32, 0, 0, 0, 0, 0, -1),
        field(CBX_K_BINARY, CBX_O_I32, 70, 2, 4, 0, 4, 0, CBX_F_SIGNED | CBX_F_BIG_ENDIAN | CBX_F_INTEGRAL, -1),
    };
    const int nf = (int)fields.size();
    uint32_t lut[256];
    for (int b = 0; b < 256; b++) {
        const int len = b % 7 == 0 ? 0 : b % 5 == 0 ? 3 : b % 3 == 0 ? 2 : 1;
        lut[b] = (uint32_t)(0x41 + b % 26) | 0x8200u | 0xA30000u | ((uint32_t)len << 24) | (b % 11 == 0 ? 0x80000000u : 0u);
    }
    const int n = 300;
    long calls = 0;
    long long chosen = 0, levels = 0;
    for (int stride : {72, 71, 64, 63, 55, 50, 43, 42, 41, 30, 20, 12, 5, 3, 1}) {
        uint8_t* data = (uint8_t*)malloc((size_t)n * stride);
        for (int i = 0; i < n * stride; i++) {
            const uint32_t r = rnd();
            // mostly digits / packed digits / zoned digits / nines from a small alphabet (so keys tie), some arbitrary bytes
            data[i] = r % 16 == 0 ? (uint8_t)(r >> 8) : r % 16 == 1 ? (uint8_t)0x99 : r % 3 == 0 ? (uint8_t)(0xF0 | ((r >> 8) % 3))
                      : r % 3 == 1 ? (uint8_t)((((r >> 8) % 2) << 4) | ((r >> 12) % 4 == 0 ? 0xC : (r >> 12) % 2))
                                   : (uint8_t)('0' + (r >> 8) % 2);
        }
        for (int first = 0; first < nf; first++) {
            for (int nk = 1; nk <= 4; nk++) {
                cbx_sort_order so;
                memset(&so, 0, sizeof so);
                so.n_keys = nk;
                for (int k = 0; k < nk; k++) {
                    so.keys[k].field = (first + 5 * k) % nf;      // (5 and 12 are coprime: no repeats)
                    so.keys[k].flags = (int)(rnd() % 4);
                }
                cbx_filter fl;
                memset(&fl, 0, sizeof fl);
                fl.n_terms = 1; fl.n_literals = 1;
                fl.literals[0].lo = (uint64_t)(int64_t)((int)(rnd() % 2001) - 1000);
                fl.literals[0].hi = (uint64_t)((int64_t)fl.literals[0].lo >> 63);
                fl.terms[0].field = 0; fl.terms[0].op = CBX_OP_GE; fl.terms[0].lit_count = 1;
                char err[256];
                int32_t lt = 0, wpk[4];
                std::vector<uint64_t> words((size_t)n * 60);
                for (int seg = -1; seg <= 0; seg++) {
                    int rc = cbxh_topn_words(fields.data(), nf, 0, &so, lut, data, (int64_t)n * stride, nullptr, nullptr, nullptr,
                                             n, stride, 0, seg, words.data(), (int64_t)words.size(), &lt, wpk, err, sizeof err);
                    if (rc != CBX_OK) { fprintf(stderr, "words: field %d keys %d: %d %s\n", first, nk, rc, err); return 1; }
                    for (int with_filter = 0; with_filter <= 1; with_filter++) {
                        for (int64_t limit : {(int64_t)1, (int64_t)7, (int64_t)n / 2, (int64_t)n - 1, (int64_t)n + 3}) {
                            std::vector<int64_t> idx((size_t)n);
                            int64_t n_out = 0;
                            cbx_topn_info info;
                            rc = cbxh_topn_select(fields.data(), nf, 0, with_filter ? &fl : nullptr, &so, lut, data,
                                                  (int64_t)n * stride, nullptr, nullptr, nullptr, n, stride, 0, seg, limit,
                                                  idx.data(), &n_out, &info, err, sizeof err);
                            if (rc != CBX_OK) { fprintf(stderr, "select: field %d keys %d: %d %s\n", first, nk, rc, err); return 1; }
                            calls++;
                            chosen += n_out;
                            levels += info.levels_run;
                            if (with_filter) continue;
                            // unfiltered: the chosen rows are the `limit` smallest composite keys
                            std::vector<int64_t> order((size_t)n);
                            for (int i = 0; i < n; i++) order[(size_t)i] = i;
                            std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
                                return std::lexicographical_compare(&words[(size_t)a * lt], &words[(size_t)a * lt] + lt,
                                                                    &words[(size_t)b * lt], &words[(size_t)b * lt] + lt);
                            });
                            const int64_t want = limit < n ? limit : n;
                            order.resize((size_t)want);
                            std::sort(order.begin(), order.end());
                            if (n_out != want || !std::equal(order.begin(), order.end(), idx.begin())) {
                                fprintf(stderr, "field %d keys %d stride %d limit %lld: select differs from the sorted keys\n",
                                        first, nk, stride, (long long)limit);
                                return 1;
                            }
                        }
                    }
                }
            }
        }
        free(data);
    }
    printf("topn host check: %ld calls, %lld rows chosen, %lld levels, no sanitizer report\n", calls, chosen, levels);
    return 0;
}
