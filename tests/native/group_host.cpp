// TEST SHIM: runs the grouped-aggregate stage's host/device part (cobrix_amd/csrc/cbx_group.h: group_build, the key
// hash, the key comparison with a slot's representative record, find-or-claim, the limb-carry add and the flush
// into a slot's accumulators) on the host, so its results can be compared with a Python evaluator over the
// oracle's rows without a GPU.  Records are processed one after the other (the compare-and-swap is a plain
// stand-in), dealt round-robin to `n_parts` tables that are then merged into one through the same find-or-claim
// and flush, as the kernels' cached partial accumulators meet in a slot.  Compiled by tests/test_group.py with
// hipcc (host path of the __host__ __device__ functions) and, with a main of its own, by
// tests/native/group_host_main.cpp under the sanitizers; never part of the product library.
#define CBX_FILTER_HOST_ONLY
#include "cbx_group.h"

#include <vector>

using namespace cbx;

namespace {
struct HostOps {
    int64_t max_groups;
    int64_t n_claimed = 0;
    bool overflow = false;
    uint64_t load(uint64_t* p) const { return *p; }
    uint64_t cas(uint64_t* p, uint64_t want) const {
        const uint64_t old = *p;
        if (old == 0) *p = want;
        return old;
    }
    bool stopped() const { return overflow; }
    void claimed() { if (++n_claimed > max_groups) overflow = true; }
    void exhausted() { overflow = true; }
    uint64_t add(uint64_t* p, uint64_t v) const { const uint64_t old = *p; *p = old + v; return old; }
    void min64(int64_t* p, int64_t v) const { if (v < *p) *p = v; }
    void max64(int64_t* p, int64_t v) const { if (v > *p) *p = v; }
};

struct Table {
    std::vector<uint64_t> slots, rows;
    std::vector<GrpAcc> acc;
    HostOps ops;
    Table(uint64_t cap, int nt, int64_t max_groups) : slots(cap, 0), rows(cap, 0), acc(cap * (size_t)nt, grp_identity()), ops{max_groups} {}
};

struct Progs {
    std::vector<AggProg> agg{1};
    std::vector<GrpProg> grp{1};
    std::vector<FilterProg> flt{1};
    bool has_filter = false;
    cbx_group_strides strides;
};

void put_err(const std::string& e, char* err, int32_t err_cap) {
    if (!err || err_cap <= 0) return;
    const size_t n = e.size() < (size_t)err_cap - 1 ? e.size() : (size_t)err_cap - 1;
    memcpy(err, e.data(), n);
    err[n] = 0;
}

int build(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl, const cbx_aggregate* ag,
          const cbx_group_by* gb, int64_t max_groups, Progs& p, char* err, int32_t err_cap) {
    std::string e;
    int rc = aggregate_build(fields, n_fields, walk_plan != 0, ag, p.agg.data(), e);
    if (rc == CBX_OK) rc = group_build(fields, n_fields, walk_plan != 0, gb, p.agg[0], p.grp.data(), e);
    if (rc == CBX_OK && fl) {
        rc = filter_build(fields, n_fields, walk_plan != 0, fl, p.flt.data(), e);
        p.has_filter = true;
    }
    if (rc == CBX_OK) rc = group_strides(fields, gb, p.agg[0].n_terms, max_groups, &p.strides, e);
    put_err(e, err, err_cap);
    return rc;
}

// src(i): record i.  Fills out / header as cbx_aggregate_grouped does.
template <typename Src>
void run(const Progs& p, const uint32_t* lut, Src src, int64_t n_rec, int32_t start_off, int32_t n_parts, int64_t max_groups,
         const cbx_group_output* out, cbx_group_header* header) {
    memset(header, 0, sizeof(*header));
    if (n_rec == 0) return;
    const int nt = p.agg[0].n_terms, nk = p.grp[0].n_keys;
    const uint64_t cap = (uint64_t)p.strides.capacity;
    const GrpHostTab tab{p.grp.data()};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    if (n_parts < 1) n_parts = 1;
    std::vector<Table> parts;
    for (int k = 0; k <= n_parts; k++) parts.emplace_back(cap, nt, max_groups);   // the last one receives the merge
    for (int64_t i = 0; i < n_rec; i++) {
        const GrpRec me = src(i);
        if (p.has_filter) {
            const FilterHostTab ftab{p.flt.data()};
            if (!filter_keep(ftab, p.flt[0].pool, me.rec, me.avail, me.head, start_off, me.seg, lutf)) continue;
        }
        Table& T = parts[(size_t)(i % n_parts)];
        GrpKeyVal kv[CBX_GROUP_MAX_KEYS];
        const uint64_t h = grp_key_hash(tab, me, start_off, lutf, kv);
        const int64_t idx = grp_find_or_claim(tab, src, T.ops, lutf, start_off, T.slots.data(), cap, h, i, kv, me);
        if (idx < 0) continue;
        T.rows[(size_t)idx]++;
        for (int t = 0; t < nt; t++) {
            const AggTerm& tm = p.agg[0].terms[t];
            int64_t hi;
            uint64_t lo;
            if (agg_value(tm, me.rec, me.avail, me.head, start_off, me.seg, hi, lo))
                grp_flush(T.ops, &T.acc[(size_t)idx * nt + t], grp_single(hi, lo), tm.funcs);
        }
    }
    Table& M = parts[(size_t)n_parts];
    for (int k = 0; k < n_parts; k++) {
        Table& T = parts[(size_t)k];
        if (T.ops.overflow) M.ops.overflow = true;
        for (uint64_t s = 0; s < cap; s++) {
            if (T.slots[s] == 0) continue;
            const int64_t i = (int64_t)(T.slots[s] - 1);
            const GrpRec me = src(i);
            GrpKeyVal kv[CBX_GROUP_MAX_KEYS];
            const uint64_t h = grp_key_hash(tab, me, start_off, lutf, kv);
            const int64_t idx = grp_find_or_claim(tab, src, M.ops, lutf, start_off, M.slots.data(), cap, h, i, kv, me);
            if (idx < 0) continue;
            M.ops.add(&M.rows[(size_t)idx], T.rows[s]);
            for (int t = 0; t < nt; t++)
                grp_flush(M.ops, &M.acc[(size_t)idx * nt + t], T.acc[s * nt + t], p.agg[0].terms[t].funcs);
        }
    }
    if (M.ops.overflow) { header->overflow = 1; return; }
    int64_t g = 0;
    for (uint64_t s = 0; s < cap; s++) {
        if (M.slots[s] == 0) continue;
        out->n_rows[g] = (int64_t)M.rows[s];
        header->n_rows += out->n_rows[g];
        for (int t = 0; t < nt; t++) out->values[g * nt + t] = grp_widen(M.acc[s * nt + t], p.agg[0].terms[t].funcs);
        grp_key_emit(tab, src((int64_t)(M.slots[s] - 1)), start_off, lutf, p.strides.str_off, out->keys + g * nk,
                     out->key_bytes + g * (int64_t)p.strides.str_stride);
        g++;
    }
    header->n_groups = g;
}
}  // namespace

// The strides group_strides gives (what cbx_group_layout returns), after the tables' validation.
extern "C" int cbxh_group_strides(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_aggregate* ag,
                                  const cbx_group_by* gb, int64_t max_groups, cbx_group_strides* strides, char* err,
                                  int32_t err_cap) {
    Progs p;
    const int rc = build(fields, n_fields, walk_plan, nullptr, ag, gb, max_groups, p, err, err_cap);
    if (rc == CBX_OK) *strides = p.strides;
    return rc;
}

// The grouped aggregate over fixed-length records (data + i * stride, stride bytes, decoded at +start_off, active
// segment `segment` for every record) that fl keeps (nullptr: all).
extern "C" int cbxh_group_fixed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                const cbx_aggregate* ag, const cbx_group_by* gb, const uint32_t* lut, const uint8_t* data,
                                int64_t n_rec, int32_t stride, int32_t start_off, int32_t segment, int32_t n_parts,
                                int64_t max_groups, const cbx_group_output* out, cbx_group_header* header, char* err,
                                int32_t err_cap) {
    Progs p;
    const int rc = build(fields, n_fields, walk_plan, fl, ag, gb, max_groups, p, err, err_cap);
    if (rc != CBX_OK) return rc;
    auto src = [&](int64_t i) -> GrpRec {
        const int64_t off = i * (int64_t)stride;
        return GrpRec{data + off, stride, off, segment};
    };
    run(p, lut, src, n_rec, start_off, n_parts, max_groups, out, header);
    return CBX_OK;
}

// As above over framed records: n_bytes of data, record i at rec_off[i] with rec_len[i] bytes (clamped to the data
// as the kernel's flt_record does), active segment rec_seg[i] (nullptr: -1 for every record).
extern "C" int cbxh_group_framed(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                 const cbx_aggregate* ag, const cbx_group_by* gb, const uint32_t* lut, const uint8_t* data,
                                 int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg,
                                 int64_t n_rec, int32_t start_off, int32_t n_parts, int64_t max_groups,
                                 const cbx_group_output* out, cbx_group_header* header, char* err, int32_t err_cap) {
    Progs p;
    const int rc = build(fields, n_fields, walk_plan, fl, ag, gb, max_groups, p, err, err_cap);
    if (rc != CBX_OK) return rc;
    auto src = [&](int64_t i) -> GrpRec {
        int64_t off = rec_off[i], len = rec_len[i];
        if (off < 0 || off > n_bytes) { off = 0; len = 0; }
        if (len > n_bytes - off) len = n_bytes - off;
        if (len < 0) len = 0;
        return GrpRec{data + off, (int)len, off, rec_seg ? rec_seg[i] : -1};
    };
    run(p, lut, src, n_rec, start_off, n_parts, max_groups, out, header);
    return CBX_OK;
}
