// TEST SHIM: runs the aggregate stage's host/device part (cobrix_amd/csrc/cbx_aggregate.h: aggregate_build,
// agg_value -- the per-record decode the GPU kernel calls per lane --, agg_accumulate and agg_merge) on the
// host, so its results can be compared with a Python evaluator over the oracle's rows without a GPU.  The
// records are accumulated in `n_parts` interleaved partial results that are then merged, so agg_merge is
// exercised as the kernels' slabs exercise it.  Compiled by tests/test_aggregate.py with hipcc (host path
// of the __host__ __device__ functions); never part of the product library.
#define CBX_FILTER_HOST_ONLY
#include "cbx_aggregate.h"

#include <vector>

using namespace cbx;

namespace {
struct Progs {
    std::vector<AggProg> agg{1};
    std::vector<FilterProg> flt{1};
    bool has_filter = false;
};

int build(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl, const cbx_aggregate* ag,
          Progs& p, char* err, int32_t err_cap) {
    std::string e;
    int rc = aggregate_build(fields, n_fields, walk_plan != 0, ag, p.agg.data(), e);
    if (rc == CBX_OK && fl) {
        rc = filter_build(fields, n_fields, walk_plan != 0, fl, p.flt.data(), e);
        p.has_filter = true;
    }
    if (err && err_cap > 0) {
        const size_t n = e.size() < (size_t)err_cap - 1 ? e.size() : (size_t)err_cap - 1;
        memcpy(err, e.data(), n);
        err[n] = 0;
    }
    return rc;
}

struct Parts {
    std::vector<cbx_aggregate_result> part;
    explicit Parts(int n) : part((size_t)(n < 1 ? 1 : n)) { memset(part.data(), 0, sizeof(cbx_aggregate_result) * part.size()); }
    void record(const Progs& p, const uint32_t* lut, int64_t i, const uint8_t* rec, int avail, int64_t head, int start_off,
                int seg) {
        cbx_aggregate_result& r = part[(size_t)i % part.size()];
        if (p.has_filter) {
            const FilterHostTab tab{p.flt.data()};
            auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
            if (!filter_keep(tab, p.flt[0].pool, rec, avail, head, start_off, seg, lutf)) return;
        }
        r.n_rows++;
        for (int t = 0; t < p.agg[0].n_terms; t++) {
            const AggTerm& tm = p.agg[0].terms[t];
            int64_t hi;
            uint64_t lo;
            const bool valid = agg_value(tm, rec, avail, head, start_off, seg, hi, lo);
            agg_accumulate(r.values[t], tm, valid, hi, lo);
        }
    }
    void finish(cbx_aggregate_result* out) const {
        *out = part[0];
        for (size_t k = 1; k < part.size(); k++) {
            out->n_rows += part[k].n_rows;
            for (int t = 0; t < CBX_AGG_MAX_TERMS; t++) agg_merge(out->values[t], part[k].values[t]);
        }
    }
};
}  // namespace

// *out = the aggregate over the fixed-length records (data + i * stride, stride bytes, decoded at
// +start_off, active segment `segment` for every record) that fl keeps (nullptr: all).  Returns the status
// aggregate_build / filter_build give (reason copied to err) or CBX_OK.
extern "C" int cbxh_aggregate_fixed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                    const cbx_aggregate* ag, const uint32_t* lut, const uint8_t* data, int64_t n_rec,
                                    int32_t stride, int32_t start_off, int32_t segment, int32_t n_parts,
                                    cbx_aggregate_result* out, char* err, int32_t err_cap) {
    Progs p;
    const int rc = build(fields, n_fields, walk_plan, fl, ag, p, err, err_cap);
    if (rc != CBX_OK) return rc;
    Parts parts(n_parts);
    for (int64_t i = 0; i < n_rec; i++) {
        const int64_t off = i * (int64_t)stride;
        parts.record(p, lut, i, data + off, stride, off, start_off, segment);
    }
    parts.finish(out);
    return CBX_OK;
}

// As above over framed records: n_bytes of data, record i at rec_off[i] with rec_len[i] bytes (clamped to the
// data as the kernel's flt_record does), active segment rec_seg[i] (nullptr: -1 for every record); head = the
// record's offset, as the kernel passes it.
extern "C" int cbxh_aggregate_framed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                     const cbx_aggregate* ag, const uint32_t* lut, const uint8_t* data, int64_t n_bytes,
                                     const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec,
                                     int32_t start_off, int32_t n_parts, cbx_aggregate_result* out, char* err,
                                     int32_t err_cap) {
    Progs p;
    const int rc = build(fields, n_fields, walk_plan, fl, ag, p, err, err_cap);
    if (rc != CBX_OK) return rc;
    Parts parts(n_parts);
    for (int64_t i = 0; i < n_rec; i++) {
        int64_t off = rec_off[i], len = rec_len[i];
        if (off < 0 || off > n_bytes) { off = 0; len = 0; }
        if (len > n_bytes - off) len = n_bytes - off;
        if (len < 0) len = 0;
        parts.record(p, lut, i, data + off, (int)len, off, start_off, rec_seg ? rec_seg[i] : -1);
    }
    parts.finish(out);
    return CBX_OK;
}
