// Stand-alone sanitizer driver for the suffix / substring ops of the filter stage's host evaluator
// (filter_host.cpp): one string field of 1..40 bytes (registers up to 32, the pointer beyond), the record cut
// at every length, 0..16 bytes readable in front of it, in a heap buffer of exactly front + length bytes,
// against literals of 0..5 bytes -- so an out-of-bounds read of flt_load_bytes' words that END at the cut,
// of the backward walk or of a verification that runs past the span is reported by AddressSanitizer / UBSan.
// Every answer is also compared with a naive evaluation here (trim, decode into a buffer, search).
// Build and run on a CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -I../../include -I../../cobrix_amd/csrc filter_host.cpp filter_strings_host_main.cpp -o filter_strings_host_check
//   ./filter_strings_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cobrix_hip.h"

extern "C" int cbxh_filter_framed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                  const uint32_t* lut, const uint8_t* data, int64_t n_bytes, const int64_t* rec_off,
                                  const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec, int32_t start_off,
                                  uint8_t* keep, char* err, int32_t err_cap);

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

// the decoded value of the field bytes p[0, n) under `trim`, as the contract states it
static std::vector<uint8_t> decoded(const uint32_t* lut, const uint8_t* p, int n, int trim) {
    int b = 0, e = n;
    if (trim == CBX_TRIM_LEFT || trim == CBX_TRIM_BOTH) while (b < e && (lut[p[b]] >> 31)) b++;
    if (trim == CBX_TRIM_RIGHT || trim == CBX_TRIM_BOTH) while (e > b && (lut[p[e - 1]] >> 31)) e--;
    std::vector<uint8_t> out;
    for (int i = b; i < e; i++)
        for (uint32_t k = 0; k < ((lut[p[i]] >> 24) & 3); k++) out.push_back((uint8_t)(lut[p[i]] >> (8 * k)));
    return out;
}

static bool naive(int op, const std::vector<uint8_t>& v, const uint8_t* lit, int ll) {
    bool hit = ll == 0;
    if (ll > 0 && (int)v.size() >= ll) {
        if (op == CBX_OP_ENDS_WITH || op == CBX_OP_NOT_ENDS_WITH) {
            hit = memcmp(v.data() + v.size() - ll, lit, (size_t)ll) == 0;
        } else {
            for (size_t s = 0; s + ll <= v.size() && !hit; s++) hit = memcmp(v.data() + s, lit, (size_t)ll) == 0;
        }
    }
    return (op == CBX_OP_ENDS_WITH || op == CBX_OP_CONTAINS) ? hit : !hit;
}

int main() {
    // one, two and three byte entries over a three-letter alphabet (so that literals match often and partial
    // matches restart), some trimmable, some with no output; continuation-like bytes repeat the same letters
    uint32_t lut[256];
    for (int b = 0; b < 256; b++) {
        const int len = b % 7 == 0 ? 0 : b % 5 == 0 ? 3 : b % 3 == 0 ? 2 : 1;
        lut[b] = (uint32_t)('a' + b % 3) | ((uint32_t)('a' + (b >> 2) % 3) << 8) | ((uint32_t)('a' + (b >> 4) % 2) << 16) |
                 ((uint32_t)len << 24) | (b % 4 == 0 ? 0x80000000u : 0u);
    }
    long calls = 0, kept = 0, wrong = 0, hits = 0, misses = 0;   // hits / misses: the positive ops on a non-empty literal
    for (int size = 1; size <= 40; size++) {
        cbx_field f;
        memset(&f, 0, sizeof f);
        f.kind = CBX_K_STRING; f.out_type = CBX_O_STRING; f.offset = 0; f.size = size;
        f.trim = CBX_TRIM_NONE + size % 4; f.segment = -1;
        for (int avail = 0; avail <= size; avail++) {
            for (int front = 0; front <= 16; front++) {
                const size_t total = (size_t)front + (size_t)avail;
                uint8_t* data = (uint8_t*)malloc(total ? total : 1);
                for (size_t i = 0; i < total; i++) data[i] = (uint8_t)rnd();
                const std::vector<uint8_t> v = decoded(lut, data + front, avail, f.trim);
                for (int ll = 0; ll <= 5; ll++) {
                    cbx_filter fl;
                    memset(&fl, 0, sizeof fl);
                    fl.n_terms = 1; fl.n_literals = 1; fl.pool_bytes = ll;
                    // a slice of the value (its end, its middle) or random letters
                    const int how = (int)(rnd() % 3);
                    for (int j = 0; j < ll; j++) {
                        const size_t at = how == 0 ? v.size() - (size_t)ll + j : rnd() % (v.size() + 1) + j;
                        fl.pool[j] = (how < 2 && (int)v.size() >= ll && at < v.size()) ? v[at] : (uint8_t)('a' + rnd() % 3);
                    }
                    fl.literals[0].str_off = 0; fl.literals[0].str_len = ll;
                    fl.terms[0].field = 0; fl.terms[0].lit_begin = 0; fl.terms[0].lit_count = 1;
                    for (int op = CBX_OP_ENDS_WITH; op <= CBX_OP_NOT_CONTAINS; op++) {
                        fl.terms[0].op = op;
                        const int64_t off = front;
                        const int32_t len = avail;
                        uint8_t keep = 0;
                        char err[256];
                        const int rc = cbxh_filter_framed(&f, 1, 0, &fl, lut, data, (int64_t)total, &off, &len, nullptr, 1, 0,
                                                          &keep, err, sizeof err);
                        if (rc != CBX_OK) { fprintf(stderr, "size %d op %d: %d %s\n", size, op, rc, err); return 1; }
                        const bool want = naive(op, v, fl.pool, ll);
                        if ((keep != 0) != want) {
                            if (wrong++ < 10)
                                fprintf(stderr, "size %d avail %d front %d trim %d op %d lit %.*s: got %d want %d\n", size, avail,
                                        front, f.trim, op, ll, (const char*)fl.pool, keep, (int)want);
                        }
                        kept += keep;
                        if (ll > 0 && (op == CBX_OP_ENDS_WITH || op == CBX_OP_CONTAINS)) { hits += keep; misses += !keep; }
                        calls++;
                    }
                }
                free(data);
            }
        }
    }
    if (wrong) { fprintf(stderr, "%ld wrong answers\n", wrong); return 1; }
    if (hits < calls / 50 || misses < calls / 50) { fprintf(stderr, "vacuous: %ld hits, %ld misses\n", hits, misses); return 1; }
    printf("filter strings host check: %ld calls, %ld kept, %ld hits, %ld misses, no sanitizer report\n", calls, kept, hits, misses);
    return 0;
}
