// TEST SHIM: runs the direct projected decode's per-record core (cobrix_amd/csrc/cbx_gather.h:
// gather_numeric, gather_str_span, gather_str_write -- the functions the GPU kernel calls per lane) on
// the host, so its values can be compared with the oracle's without a GPU.  Compiled by
// tests/test_project.py with hipcc (host path of the __host__ __device__ functions); never part of the
// product library.
#define CBX_GATHER_HOST_ONLY
#define CBX_FILTER_HOST_ONLY
#include "cbx_gather.h"

#include <vector>

using namespace cbx;

// Every field of the table over n_rec records of data[0, n_bytes): record i at rec_off[i] with rec_len[i]
// bytes (rec_off null: fixed-length records of `stride` bytes), clamped to the data as the kernel's
// gth_record does, decoded at +start_off, active segment rec_seg[i] (null: -1 for every record).  The core
// gets head = the record's offset, as the kernel passes it.  Output, field-major [n_fields][n_rec]:
//   valid; lo / hi (numerics: the value's 128 bits); str_pos / str_len (strings: their UTF-8 bytes in heap).
// Returns CBX_OK, CBX_E_UNSUPPORTED when gather_build refuses the table (reason in err), CBX_E_CAPACITY
// when the heap is too small.
extern "C" int cbxh_gather(const cbx_field* fields, int32_t n_fields, const uint32_t* lut, const uint8_t* data,
                           int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg,
                           int64_t n_rec, int32_t stride, int32_t start_off, uint8_t* valid, uint64_t* lo, uint64_t* hi,
                           int64_t* str_pos, int32_t* str_len, uint8_t* heap, int64_t heap_cap, char* err, int32_t err_cap) {
    std::vector<GatherOp> ops;
    std::string e;
    const bool ok = gather_build(fields, n_fields, ops, e);
    if (err && err_cap > 0) {
        const size_t n = e.size() < (size_t)err_cap - 1 ? e.size() : (size_t)err_cap - 1;
        memcpy(err, e.data(), n);
        err[n] = 0;
    }
    if (!ok) return CBX_E_UNSUPPORTED;
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    int64_t used = 0;
    for (int k = 0; k < n_fields; k++) {
        const GatherOp& g = ops[k];
        for (int64_t i = 0; i < n_rec; i++) {
            int64_t off = rec_off ? rec_off[i] : i * (int64_t)stride, len = rec_off ? rec_len[i] : stride;
            if (off < 0 || off > n_bytes) { off = 0; len = 0; }
            if (len > n_bytes - off) len = n_bytes - off;
            if (len < 0) len = 0;
            const uint8_t* rec = data + off;
            const int seg = rec_seg ? rec_seg[i] : -1;
            const int64_t at = (int64_t)k * n_rec + i;
            valid[at] = 0; lo[at] = hi[at] = 0; str_pos[at] = 0; str_len[at] = 0;
            if (g.what == G_STRING) {
                int o, n;
                if (!gather_str_locate(g, (int)len, start_off, seg, o, n)) continue;
                const uint8_t* p = rec + o;
                const bool regs = gather_str_in_regs(g);   // as the kernel: short EBCDIC / ASCII strings in registers
                FltBytes fb{{0, 0, 0, 0}};
                if (regs) fb = flt_load_bytes(p, n, g.f.size, off + o);
                const StrSpan sp = regs ? gather_str_span(g, fb, n, lutf) : gather_str_span(g, p, n, lutf);
                if (used + sp.utf8_len > heap_cap) return CBX_E_CAPACITY;
                if (regs) gather_str_write(g, fb, sp, heap + used, lutf);
                else gather_str_write(g, p, sp, heap + used, lutf);
                valid[at] = 1; str_pos[at] = used; str_len[at] = sp.utf8_len;
                used += sp.utf8_len;
            } else if (g.what == G_NUMERIC) {
                const Val v = gather_numeric(g, rec, (int)len, off, start_off, seg);
                valid[at] = v.valid ? 1 : 0; lo[at] = v.lo; hi[at] = v.hi;
            }
        }
    }
    return CBX_OK;
}
