// Stand-alone sanitizer driver for the direct projected decode's host core (gather_host.cpp): random
// records in heap buffers that start exactly at the data's start and end exactly at its end -- strides
// that cut records inside and in front of every field, and framed records at odd offsets with lengths
// from 0 up -- through every decoder kind, so an out-of-bounds read or undefined arithmetic in the core
// (the SWAR decoders' 8- and 16-byte loads that END at a field's end, the string spans of cut records)
// is reported by AddressSanitizer / UBSan.  Build and run on a CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -I../../include -I../../cobrix_amd/csrc gather_host.cpp gather_host_main.cpp -o gather_host_check
//   ./gather_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cobrix_hip.h"

extern "C" int cbxh_gather(const cbx_field* fields, int32_t n_fields, const uint32_t* lut, const uint8_t* data,
                           int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg,
                           int64_t n_rec, int32_t stride, int32_t start_off, uint8_t* valid, uint64_t* lo, uint64_t* hi,
                           int64_t* str_pos, int32_t* str_len, uint8_t* heap, int64_t heap_cap, char* err, int32_t err_cap);

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
    // a 76-byte layout: binary, COMP-3 (8 and 16 bytes), zoned, ASCII number, EBCDIC-table string, ASCII
    // string (of segment 0), COMP-2 over the first bytes, HEX, RAW and UTF-16 strings
    std::vector<cbx_field> fields = {
        field(CBX_K_BINARY, CBX_O_I32, 0, 4, 9, 0, 9, 0, CBX_F_SIGNED | CBX_F_BIG_ENDIAN | CBX_F_INTEGRAL, -1),
        field(CBX_K_BCD, CBX_O_DEC64, 4, 8, 15, 2, 15, 2, CBX_F_SIGNED, -1),
        field(CBX_K_BCD, CBX_O_DEC128, 12, 16, 30, 5, 30, 5, CBX_F_SIGNED, -1),
        field(CBX_K_ZONED, CBX_O_I32, 28, 9, 9, 0, 9, 0, CBX_F_SIGNED | CBX_F_INTEGRAL, -1),
        field(CBX_K_ASCII_NUM, CBX_O_I32, 37, 5, 5, 0, 5, 0, CBX_F_INTEGRAL, -1),
        field(CBX_K_STRING, CBX_O_STRING, 42, 12, 0, 0, 0, 0, 0, -1),
        field(CBX_K_STRING_ASCII, CBX_O_STRING, 54, 10, 0, 0, 0, 0, 0, 0),
        field(CBX_K_DOUBLE, CBX_O_F64, 0, 8, 0, 0, 0, 0, 0, -1),
        field(CBX_K_HEX, CBX_O_STRING, 64, 3, 0, 0, 0, 0, 0, -1),
        field(CBX_K_RAW, CBX_O_BINARY, 67, 3, 0, 0, 0, 0, 0, -1),
        field(CBX_K_UTF16_BE, CBX_O_STRING, 70, 6, 0, 0, 0, 0, 0, -1),
    };
    const int nf = (int)fields.size();
    uint32_t lut[256];
    for (int b = 0; b < 256; b++) {
        // one, two and three byte entries, some trimmable, some with no output
        const int len = b % 7 == 0 ? 0 : b % 5 == 0 ? 3 : b % 3 == 0 ? 2 : 1;
        lut[b] = (uint32_t)(0x41 + b % 26) | 0x8200u | 0xA30000u | ((uint32_t)len << 24) | (b % 11 == 0 ? 0x80000000u : 0u);
    }
    const int n = 512;
    long calls = 0, values = 0;
    std::vector<uint8_t> valid((size_t)nf * n);
    std::vector<uint64_t> lo((size_t)nf * n), hi((size_t)nf * n);
    std::vector<int64_t> pos((size_t)nf * n);
    std::vector<int32_t> len((size_t)nf * n);
    const int64_t heap_cap = (int64_t)n * 76 * 3;
    uint8_t* heap = (uint8_t*)malloc((size_t)heap_cap);
    char err[256];
    auto fill = [](uint8_t* data, size_t bytes) {
        for (size_t i = 0; i < bytes; i++) {
            const uint32_t r = rnd();
            // mostly digits / packed digits / zoned digits, some arbitrary bytes
            data[i] = r % 16 == 0 ? (uint8_t)(r >> 8) : r % 3 == 0 ? (uint8_t)(0xF0 | ((r >> 8) % 10))
                      : r % 3 == 1 ? (uint8_t)((((r >> 8) % 10) << 4) | ((r >> 12) % 10 == 0 ? 0xC : (r >> 12) % 10))
                                   : (uint8_t)('0' + (r >> 8) % 10);
        }
    };
    // fixed-length records: the stride is the record's readable length
    for (int stride : {76, 75, 73, 70, 69, 67, 64, 63, 55, 50, 43, 42, 41, 30, 20, 12, 5, 3, 1}) {
        uint8_t* data = (uint8_t*)malloc((size_t)n * stride);
        fill(data, (size_t)n * stride);
        for (int start : {0, 1}) {
            const int rc = cbxh_gather(fields.data(), nf, lut, data, (int64_t)n * stride, nullptr, nullptr, nullptr, n, stride,
                                       start, valid.data(), lo.data(), hi.data(), pos.data(), len.data(), heap, heap_cap, err,
                                       sizeof err);
            if (rc != CBX_OK) { fprintf(stderr, "stride %d: %d %s\n", stride, rc, err); return 1; }
            for (uint8_t v : valid) values += v;
            calls++;
        }
        free(data);
    }
    // framed records: odd offsets from the buffer's first byte, lengths 0..90 (clamped to the data by the
    // shim as the kernel clamps them), some offsets outside the data, both segments
    for (int round = 0; round < 8; round++) {
        const int64_t bytes = 1 + rnd() % 20000;
        uint8_t* data = (uint8_t*)malloc((size_t)bytes);
        fill(data, (size_t)bytes);
        std::vector<int64_t> off(n);
        std::vector<int32_t> ln(n), seg(n);
        for (int i = 0; i < n; i++) {
            off[i] = i < 4 ? i : (int64_t)(rnd() % (bytes + 8)) - 2;
            ln[i] = (int32_t)(rnd() % 91);
            seg[i] = (int32_t)(rnd() % 3) - 1;
        }
        const int rc = cbxh_gather(fields.data(), nf, lut, data, bytes, off.data(), ln.data(), seg.data(), n, 0, round % 2,
                                   valid.data(), lo.data(), hi.data(), pos.data(), len.data(), heap, heap_cap, err, sizeof err);
        if (rc != CBX_OK) { fprintf(stderr, "framed round %d: %d %s\n", round, rc, err); return 1; }
        for (uint8_t v : valid) values += v;
        calls++;
        free(data);
    }
    free(heap);
    printf("gather host check: %ld calls, %ld valid values, no sanitizer report\n", calls, values);
    return 0;
}
