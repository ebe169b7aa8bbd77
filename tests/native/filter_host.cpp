// TEST SHIM: runs the filter stage's per-record evaluator (cobrix_amd/csrc/cbx_filter.h, filter_keep:
// decode, compare, group logic -- the function the GPU kernel calls per lane) on the host, so its
// answers can be compared with a Python evaluator over the oracle's rows without a GPU.  Compiled by
// tests/test_filter.py with hipcc (host path of the __host__ __device__ functions); never part of the
// product library.
#define CBX_FILTER_HOST_ONLY
#include "cbx_filter.h"

#include <vector>

using namespace cbx;

// keep[i] = 1 when the filter keeps fixed-length record i (data + i * stride, stride bytes, decoded at
// +start_off, active segment `segment` for every record).  Returns the status filter_build gives
// (reason copied to err) or CBX_OK.
extern "C" int cbxh_filter_fixed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                 const uint32_t* lut, const uint8_t* data, int64_t n_rec, int32_t stride,
                                 int32_t start_off, int32_t segment, uint8_t* keep, char* err, int32_t err_cap) {
    std::vector<FilterProg> prog(1);
    std::string e;
    const int rc = filter_build(fields, n_fields, walk_plan != 0, fl, prog.data(), e);
    if (err && err_cap > 0) {
        const size_t n = e.size() < (size_t)err_cap - 1 ? e.size() : (size_t)err_cap - 1;
        memcpy(err, e.data(), n);
        err[n] = 0;
    }
    if (rc != CBX_OK) return rc;
    const FilterHostTab tab{prog.data()};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    for (int64_t i = 0; i < n_rec; i++) {
        const int64_t off = i * (int64_t)stride;
        keep[i] = filter_keep(tab, prog[0].pool, data + off, stride, off, start_off, segment, lutf) ? 1 : 0;
    }
    return CBX_OK;
}

// keep[i] = 1 when the filter keeps framed record i: n_bytes of data, the record at rec_off[i] with
// rec_len[i] bytes (clamped to the data as the kernel's flt_record does), decoded at +start_off, active
// segment rec_seg[i] (nullptr: -1 for every record).  filter_keep gets head = the record's offset, as
// the kernel passes it, so the 8- / 16-byte loads that end at a field's end reach back into the bytes
// in front of the record exactly where the kernel's do.
extern "C" int cbxh_filter_framed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                  const uint32_t* lut, const uint8_t* data, int64_t n_bytes, const int64_t* rec_off,
                                  const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec, int32_t start_off,
                                  uint8_t* keep, char* err, int32_t err_cap) {
    std::vector<FilterProg> prog(1);
    std::string e;
    const int rc = filter_build(fields, n_fields, walk_plan != 0, fl, prog.data(), e);
    if (err && err_cap > 0) {
        const size_t n = e.size() < (size_t)err_cap - 1 ? e.size() : (size_t)err_cap - 1;
        memcpy(err, e.data(), n);
        err[n] = 0;
    }
    if (rc != CBX_OK) return rc;
    const FilterHostTab tab{prog.data()};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    for (int64_t i = 0; i < n_rec; i++) {
        int64_t off = rec_off[i], len = rec_len[i];
        if (off < 0 || off > n_bytes) { off = 0; len = 0; }
        if (len > n_bytes - off) len = n_bytes - off;
        if (len < 0) len = 0;
        keep[i] = filter_keep(tab, prog[0].pool, data + off, (int)len, off, start_off, rec_seg ? rec_seg[i] : -1,
                              lutf) ? 1 : 0;
    }
    return CBX_OK;
}
