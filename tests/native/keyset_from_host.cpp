// TEST SHIM: runs the host/device part of cobrix_amd/csrc/cbx_keyset_from.h (keyset_from_build with its compatibility
// rules and bounds, find-or-claim on bare slot words, the conversion rule) on the host, in front of the key-set shim
// (keyset_host.cpp: layout, build, membership), so a set built from a second file's records can be compared with a
// Python model over the oracle's rows without a GPU.  Records are inserted one after the other (the compare-and-swap
// is a plain stand-in).  Compiled by tests/test_keyset_from.py with hipcc (host path of the __host__ __device__
// functions) and, with a main of its own, by tests/native/keyset_from_host_main.cpp under the sanitizers; never part
// of the product library.
#include "keyset_host.cpp"

#include "cbx_keyset_from.h"

namespace {
struct HostKsfOps {
    int64_t claims = 0, max_values = 0;
    bool overflow = false;
    uint64_t load(uint64_t* p) const { return *p; }
    uint64_t cas(uint64_t* p, uint64_t want) const {
        const uint64_t old = *p;
        if (old == 0) *p = want;
        return old;
    }
    bool stopped() const { return overflow; }
    void claimed() { if (++claims > max_values) overflow = true; }
    void exhausted() { overflow = true; }
};
}  // namespace

// As cbx_key_set_create_from_records, on the host: the source records (the arguments of cbxh_keyset_keep) through the
// source plan's fields and code page, the set over the probe plan's keys in *out (for cbxh_keyset_keep with the probe
// plan's records).  Exact-size heap buffers for the table and the value array.
extern "C" int cbxh_keyset_from_records(const cbx_field* pf, int32_t n_pf, int32_t p_walk, const cbx_group_by* pk,
                                        const cbx_field* sf, int32_t n_sf, int32_t s_walk, const cbx_group_by* sk,
                                        const cbx_filter* fl, const uint32_t* lut, const uint8_t* data, int64_t n_bytes,
                                        const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec,
                                        int32_t stride, int32_t start_off, int32_t segment, int64_t max_values,
                                        cbxh_key_set** out, cbx_keyset_source_info* info, char* err, int32_t err_cap) {
    *out = nullptr;
    memset(info, 0, sizeof(*info));
    std::string e;
    std::vector<GrpProg> probe(1);
    std::vector<KsfProg> ksf(1);
    std::vector<FilterProg> flt(1);
    int rc = keyset_from_build(pf, n_pf, p_walk != 0, pk, sf, n_sf, s_walk != 0, sk, probe.data(), ksf.data(), e);
    if (rc == CBX_OK && fl) rc = filter_build(sf, n_sf, s_walk != 0, fl, flt.data(), e);
    int64_t cap = 0;
    if (rc == CBX_OK) rc = keyset_from_capacity(max_values, &cap, e);
    const int nk = probe[0].n_keys;
    int32_t str_off[CBX_GROUP_MAX_KEYS] = {0, 0, 0, 0}, str_stride = 0;
    KsLayout L;
    if (rc == CBX_OK) {
        str_stride = keyset_from_strides(pf, pk, probe[0], str_off);
        rc = keyset_layout(pf, pk, max_values, str_stride, str_off, &L, e);
    }
    if (rc != CBX_OK) { put_err(e, err, err_cap); return rc; }
    info->source_capacity = cap;
    info->workspace_bytes = 8 * cap;
    uint64_t* slots = (uint64_t*)calloc((size_t)cap, 8);
    const Source src{data, n_bytes, rec_off, rec_len, rec_seg, stride, segment};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    const GrpHostTab tab{&ksf[0].src};
    HostKsfOps ops;
    ops.max_values = max_values;
    for (int64_t i = 0; i < n_rec; i++) {
        const GrpRec me = src(i);
        if (fl) {
            const FilterHostTab ftab{flt.data()};
            if (!filter_keep(ftab, flt[0].pool, me.rec, me.avail, me.head, start_off, me.seg, lutf)) continue;
        }
        info->n_rows++;
        GrpKeyVal kv[CBX_GROUP_MAX_KEYS];
        uint64_t hash;
        if (!ks_record_key(tab, me, start_off, lutf, kv, hash)) { info->n_null_rows++; continue; }
        (void)ksf_find_or_claim(ops, slots, (uint64_t)cap, hash, i, [&](int64_t j) -> bool {
            return ksf_records_equal(tab, me, src(j), start_off, lutf);
        });
    }
    if (ops.overflow) {
        free(slots);
        info->overflow = 1;
        put_err("cbx_key_set_create_from_records: more than max_values distinct source keys", err, err_cap);
        return CBX_E_CAPACITY;
    }
    // convert: the value array holds exactly the claims
    const int64_t claims = ops.claims;
    cbx_key_value* vals = (cbx_key_value*)malloc(claims * nk ? (size_t)(claims * nk) * sizeof(cbx_key_value) : 1);
    uint8_t* bytes = (uint8_t*)malloc(claims * str_stride ? (size_t)(claims * str_stride) : 1);
    const KsfHostTab ktab{ksf.data()};
    int64_t n_values = 0, dropped = 0;
    for (int64_t s = 0; s < cap; s++) {
        if (slots[s] == 0) continue;
        const GrpRec rep = src((int64_t)(slots[s] - 1));
        cbx_key_value v[CBX_GROUP_MAX_KEYS];
        if (!ksf_value(ktab, rep, start_off, lutf, v)) { dropped++; continue; }
        for (int k = 0; k < nk; k++) vals[n_values * nk + k] = v[k];
        if (str_stride > 0) ksf_value_bytes(ktab, rep, start_off, lutf, str_off, bytes + n_values * str_stride);
        n_values++;
    }
    free(slots);
    info->n_source_keys = claims;
    info->n_dropped = dropped;
    rc = cbxh_keyset_create(pf, n_pf, p_walk, pk, vals, bytes, str_stride, str_off, n_values, out, err, err_cap);
    free(vals);
    free(bytes);
    return rc;
}
