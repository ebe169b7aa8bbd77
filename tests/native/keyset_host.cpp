// TEST SHIM: runs the key-set stage's host/device part (cobrix_amd/csrc/cbx_keyset.h: keyset_layout, the value-side
// hash, insert with fingerprints, the record-side key, the membership test) on the host, so its results can be
// compared with a Python evaluator over the oracle's rows without a GPU.  Values are inserted one after the other
// (the compare-and-swap is a plain stand-in).  Compiled by tests/test_keyset.py with hipcc (host path of the
// __host__ __device__ functions) and, with a main of its own, by tests/native/keyset_host_main.cpp under the
// sanitizers; never part of the product library.
#define CBX_FILTER_HOST_ONLY
#include "cbx_keyset.h"

#include <vector>

using namespace cbx;

namespace {
struct HostKsOps {
    uint64_t load(uint64_t* p) const { return *p; }
    uint64_t cas(uint64_t* p, uint64_t want) const {
        const uint64_t old = *p;
        if (old == 0) *p = want;
        return old;
    }
};

void put_err(const std::string& e, char* err, int32_t err_cap) {
    if (!err || err_cap <= 0) return;
    const size_t n = e.size() < (size_t)err_cap - 1 ? e.size() : (size_t)err_cap - 1;
    memcpy(err, e.data(), n);
    err[n] = 0;
}
}  // namespace

// Exact-size copies of everything a set holds (a read past a value, its bytes or the table is a heap overflow).
struct cbxh_key_set {
    std::vector<GrpProg> prog{1};
    uint64_t* slots = nullptr;
    cbx_key_value* vals = nullptr;
    uint8_t* bytes = nullptr;
    KsTable t{};
    cbx_keyset_info info{};
    ~cbxh_key_set() { free(slots); free(vals); free(bytes); }
};

// As cbx_key_set_create, on the host.
extern "C" int cbxh_keyset_create(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_group_by* gb,
                                  const cbx_key_value* values, const uint8_t* bytes, int32_t str_stride, const int32_t* str_off,
                                  int64_t n_values, cbxh_key_set** out, char* err, int32_t err_cap) {
    std::string e;
    cbxh_key_set* S = new cbxh_key_set();
    std::vector<AggProg> none(1);
    memset(none.data(), 0, sizeof(AggProg));
    int rc = group_build(fields, n_fields, walk_plan != 0, gb, none[0], S->prog.data(), e);
    KsLayout L;
    if (rc == CBX_OK) rc = keyset_layout(fields, gb, n_values, str_stride, str_off, &L, e);
    if (rc == CBX_OK) rc = keyset_check_values(S->prog[0], values, n_values, e);
    if (rc != CBX_OK) { put_err(e, err, err_cap); delete S; return rc; }
    const int nk = S->prog[0].n_keys;
    const size_t nv = (size_t)n_values * nk, nbytes = (size_t)n_values * (size_t)L.str_stride;
    S->slots = (uint64_t*)calloc((size_t)L.capacity, 8);
    S->vals = (cbx_key_value*)malloc(nv ? nv * sizeof(cbx_key_value) : 1);
    S->bytes = (uint8_t*)malloc(nbytes ? nbytes : 1);
    if (nv) memcpy(S->vals, values, nv * sizeof(cbx_key_value));
    if (nbytes) memcpy(S->bytes, bytes, nbytes);
    KsTable& t = S->t;
    t.slots = S->slots; t.vals = S->vals; t.bytes = S->bytes;
    t.capacity = (uint64_t)L.capacity; t.n_values = n_values; t.n_keys = nk; t.str_stride = L.str_stride;
    for (int k = 0; k < CBX_GROUP_MAX_KEYS; k++) t.str_off[k] = L.str_off[k];
    const GrpHostTab tab{S->prog.data()};
    HostKsOps ops;
    int64_t distinct = 0, max_probe = 0;
    for (int64_t i = 0; i < n_values; i++) {
        int64_t probes = 0;
        if (ks_insert(tab, ops, S->slots, t, i, probes)) distinct++;
        if (probes > max_probe) max_probe = probes;
    }
    S->info.n_values = n_values; S->info.n_distinct = distinct; S->info.capacity = L.capacity;
    S->info.device_bytes = L.device_bytes; S->info.max_probe = max_probe; S->info.n_keys = nk;
    *out = S;
    return CBX_OK;
}

extern "C" void cbxh_keyset_info(const cbxh_key_set* S, cbx_keyset_info* out) { *out = S->info; }
extern "C" void cbxh_keyset_destroy(cbxh_key_set* S) { delete S; }

// The value-side hash of every value of the set.
extern "C" void cbxh_keyset_value_hashes(const cbxh_key_set* S, uint64_t* out) {
    const GrpHostTab tab{S->prog.data()};
    const KsTable& t = S->t;
    for (int64_t i = 0; i < t.n_values; i++)
        out[i] = ks_value_hash(tab, t.vals + i * t.n_keys, t.bytes + i * (int64_t)t.str_stride, t.str_off);
}

namespace {
// record i of a source: fixed-length records (stride > 0) or framed ones, clamped to the data as flt_record does
struct Source {
    const uint8_t* data;
    int64_t n_bytes;
    const int64_t* rec_off;
    const int32_t* rec_len;
    const int32_t* rec_seg;
    int32_t stride, segment;
    GrpRec operator()(int64_t i) const {
        int64_t off, len;
        if (rec_off) { off = rec_off[i]; len = rec_len[i]; }
        else { off = i * (int64_t)stride; len = stride; }
        if (off < 0 || off > n_bytes) { off = 0; len = 0; }
        if (len > n_bytes - off) len = n_bytes - off;
        if (len < 0) len = 0;
        return GrpRec{data + off, (int)len, off, rec_seg ? rec_seg[i] : segment};
    }
};
}  // namespace

// The record-side key of every record under the set's keys: its hash (grp_key_hash) and whether a component is null.
extern "C" void cbxh_keyset_record_hashes(const cbxh_key_set* S, const uint32_t* lut, const uint8_t* data, int64_t n_bytes,
                                          const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec,
                                          int32_t stride, int32_t start_off, int32_t segment, uint64_t* hashes, uint8_t* nulls) {
    const GrpHostTab tab{S->prog.data()};
    const Source src{data, n_bytes, rec_off, rec_len, rec_seg, stride, segment};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    for (int64_t i = 0; i < n_rec; i++) {
        GrpKeyVal kv[CBX_GROUP_MAX_KEYS];
        uint64_t h;
        nulls[i] = ks_record_key(tab, src(i), start_off, lutf, kv, h) ? 0 : 1;
        hashes[i] = h;
    }
}

// keep[i] as the keyed test pass decides it: the cbx_filter first (nullptr: none), then every set.
extern "C" int cbxh_keyset_keep(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                const uint32_t* lut, const uint8_t* data, int64_t n_bytes, const int64_t* rec_off,
                                const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec, int32_t stride, int32_t start_off,
                                int32_t segment, const cbxh_key_set* const* sets, const int32_t* negate, int32_t n_sets,
                                uint8_t* keep, char* err, int32_t err_cap) {
    std::vector<FilterProg> flt(1);
    if (fl) {
        std::string e;
        const int rc = filter_build(fields, n_fields, walk_plan != 0, fl, flt.data(), e);
        if (rc != CBX_OK) { put_err(e, err, err_cap); return rc; }
    }
    const Source src{data, n_bytes, rec_off, rec_len, rec_seg, stride, segment};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    for (int64_t i = 0; i < n_rec; i++) {
        const GrpRec me = src(i);
        bool k = true;
        if (fl) {
            const FilterHostTab ftab{flt.data()};
            k = filter_keep(ftab, flt[0].pool, me.rec, me.avail, me.head, start_off, me.seg, lutf);
        }
        for (int s = 0; s < n_sets && k; s++) {
            const GrpHostTab tab{sets[s]->prog.data()};
            k = ks_keep(tab, sets[s]->t, negate && negate[s] != 0, me, start_off, lutf);
        }
        keep[i] = k ? 1 : 0;
    }
    return CBX_OK;
}
