// TEST SHIM: runs the host/device part of cobrix_amd/csrc/cbx_keymap.h (ks_find, the payload update rule, the join
// verdict, the ordinal gather's row, the join's argument refusals) on the host, in front of the key-set-from-records
// shim (keyset_from_host.cpp), so a key map and a lookup join can be compared with a Python model over the oracle's
// rows without a GPU.  Records are visited one after the other (the atomics are plain stand-ins).  Compiled by
// tests/test_keymap.py with hipcc (host path of the __host__ __device__ functions) and, with a main of its own, by
// tests/native/keymap_host_main.cpp under the sanitizers; never part of the product library.
#include "keyset_from_host.cpp"

#include "cbx_keymap.h"

namespace {
struct HostKmOps {
    void min64(int64_t* p, int64_t v) const { if (v < *p) *p = v; }
    uint64_t add(uint64_t* p, uint64_t v) const { const uint64_t old = *p; *p = old + v; return old; }
};
}  // namespace

// Exact-size copies of the payload (a read past a value's entry is a heap overflow).
struct cbxh_key_map {
    cbxh_key_set* set = nullptr;
    int64_t* first_row = nullptr;
    int64_t* n_rows = nullptr;
    int64_t pin_failures = 0;
    cbx_keymap_info info{};
    ~cbxh_key_map() { if (set) cbxh_keyset_destroy(set); free(first_row); free(n_rows); }
};

// As cbx_key_map_create_from_records, on the host (the arguments of cbxh_keyset_from_records).  The fill loop also
// pins what the fill pass assumes: for every kept source row with a non-null key, ks_find through the SOURCE plan's
// GrpProg returns the member whose value tuple ksf_value produced (hash included), and -1 when ksf_value dropped it.
extern "C" int cbxh_keymap_from_records(const cbx_field* pf, int32_t n_pf, int32_t p_walk, const cbx_group_by* pk,
                                        const cbx_field* sf, int32_t n_sf, int32_t s_walk, const cbx_group_by* sk,
                                        const cbx_filter* fl, const uint32_t* lut, const uint8_t* data, int64_t n_bytes,
                                        const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec,
                                        int32_t stride, int32_t start_off, int32_t segment, int64_t max_values,
                                        cbxh_key_map** out, cbx_keymap_info* info, char* err, int32_t err_cap) {
    *out = nullptr;
    memset(info, 0, sizeof(*info));
    cbx_keyset_source_info si;
    cbxh_key_set* S = nullptr;
    int rc = cbxh_keyset_from_records(pf, n_pf, p_walk, pk, sf, n_sf, s_walk, sk, fl, lut, data, n_bytes, rec_off, rec_len, rec_seg,
                                      n_rec, stride, start_off, segment, max_values, &S, &si, err, err_cap);
    info->n_rows = si.n_rows; info->n_null_rows = si.n_null_rows; info->n_source_keys = si.n_source_keys;
    info->n_dropped = si.n_dropped; info->source_capacity = si.source_capacity; info->workspace_bytes = si.workspace_bytes;
    info->overflow = si.overflow;
    if (rc != CBX_OK) return rc;
    cbxh_key_map* M = new cbxh_key_map();
    M->set = S;
    const KsTable& t = S->t;
    const int64_t nv = t.n_values;
    M->first_row = (int64_t*)malloc(nv ? (size_t)nv * 8 : 1);
    M->n_rows = (int64_t*)malloc(nv ? (size_t)nv * 8 : 1);
    for (int64_t j = 0; j < nv; j++) { M->first_row[j] = kKmNoRow; M->n_rows[j] = 0; }
    std::string e;
    std::vector<GrpProg> probe(1);
    std::vector<KsfProg> ksf(1);
    std::vector<FilterProg> flt(1);
    rc = keyset_from_build(pf, n_pf, p_walk != 0, pk, sf, n_sf, s_walk != 0, sk, probe.data(), ksf.data(), e);
    if (rc == CBX_OK && fl) rc = filter_build(sf, n_sf, s_walk != 0, fl, flt.data(), e);
    if (rc != CBX_OK) { put_err(e, err, err_cap); delete M; return rc; }
    const Source src{data, n_bytes, rec_off, rec_len, rec_seg, stride, segment};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    const GrpHostTab stab{&ksf[0].src}, ptab{probe.data()};
    const KsfHostTab ktab{ksf.data()};
    const HostKmOps ops;
    uint8_t* vb = (uint8_t*)malloc(t.str_stride ? (size_t)t.str_stride : 1);   // one value's string bytes, exactly
    for (int64_t i = 0; i < n_rec; i++) {
        const GrpRec me = src(i);
        if (fl) {
            const FilterHostTab ftab{flt.data()};
            if (!filter_keep(ftab, flt[0].pool, me.rec, me.avail, me.head, start_off, me.seg, lutf)) continue;
        }
        const int64_t j = km_lookup(stab, t, me, start_off, lutf);
        if (j >= 0) km_update(ops, M->first_row, M->n_rows, j, i);
        // the pin
        GrpKeyVal kv[CBX_GROUP_MAX_KEYS];
        uint64_t hash;
        if (!ks_record_key(stab, me, start_off, lutf, kv, hash)) { if (j != -1) M->pin_failures++; continue; }
        cbx_key_value v[CBX_GROUP_MAX_KEYS];
        if (!ksf_value(ktab, me, start_off, lutf, v)) { if (j != -1) M->pin_failures++; continue; }
        if (t.str_stride > 0) ksf_value_bytes(ktab, me, start_off, lutf, t.str_off, vb);
        if (j < 0 || j >= nv || ks_value_hash(ptab, v, vb, t.str_off) != hash ||
            !ks_values_equal(ptab, v, vb, t.vals + j * t.n_keys, t.bytes + j * (int64_t)t.str_stride, t.str_off))
            M->pin_failures++;
    }
    free(vb);
    for (int64_t j = 0; j < nv; j++) {
        if (M->n_rows[j] > 1) M->info.n_duplicate_keys++;
        if (M->n_rows[j] > M->info.max_rows_per_key) M->info.max_rows_per_key = M->n_rows[j];
        if (M->n_rows[j] < 1 || M->first_row[j] == kKmNoRow) M->pin_failures++;   // a member no row reached
    }
    info->n_duplicate_keys = M->info.n_duplicate_keys;
    info->max_rows_per_key = M->info.max_rows_per_key;
    M->info = *info;
    *out = M;
    return CBX_OK;
}

extern "C" void cbxh_keymap_destroy(cbxh_key_map* M) { delete M; }
extern "C" const cbxh_key_set* cbxh_keymap_set(const cbxh_key_map* M) { return M->set; }
extern "C" int64_t cbxh_keymap_pin_failures(const cbxh_key_map* M) { return M->pin_failures; }
extern "C" int64_t cbxh_keymap_payload(const cbxh_key_map* M, int64_t* first_row, int64_t* n_rows) {
    const int64_t nv = M->set->t.n_values;
    for (int64_t j = 0; first_row && j < nv; j++) { first_row[j] = M->first_row[j]; n_rows[j] = M->n_rows[j]; }
    return nv;
}

// Per INPUT record what the join's test pass decides: keep[i], and for kept records match[i] / rows[i] (else -2 / -2).
extern "C" int cbxh_keymap_join(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                const uint32_t* lut, const uint8_t* data, int64_t n_bytes, const int64_t* rec_off,
                                const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec, int32_t stride, int32_t start_off,
                                int32_t segment, const cbxh_key_set* const* sets, const int32_t* negate, int32_t n_sets,
                                const cbxh_key_map* map, int32_t join_type, uint8_t* keep, int64_t* match, int64_t* rows,
                                char* err, int32_t err_cap) {
    std::string e;
    int rc = km_join_check(map != nullptr, true, join_type, match != nullptr, n_sets, sets != nullptr, e);
    std::vector<FilterProg> flt(1);
    if (rc == CBX_OK && fl) rc = filter_build(fields, n_fields, walk_plan != 0, fl, flt.data(), e);
    if (rc != CBX_OK) { put_err(e, err, err_cap); return rc; }
    const Source src{data, n_bytes, rec_off, rec_len, rec_seg, stride, segment};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    const GrpHostTab mtab{map->set->prog.data()};
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
        int64_t m = -2, r = -2;
        if (k) k = km_verdict(join_type, mtab, map->set->t, map->first_row, map->n_rows, me, start_off, lutf, m, r);
        keep[i] = k ? 1 : 0;
        match[i] = k ? m : -2;
        if (rows) rows[i] = k ? r : -2;
    }
    return CBX_OK;
}

extern "C" int cbxh_join_check(int32_t has_map, int32_t map_of_plan, int32_t join_type, int32_t has_match, int32_t n_sets,
                               int32_t has_sets, char* err, int32_t err_cap) {
    std::string e;
    const int rc = km_join_check(has_map != 0, map_of_plan != 0, join_type, has_match != 0, n_sets, has_sets != 0, e);
    put_err(e, err, err_cap);
    return rc;
}

// The rows ordinals_gather_kernel writes for a source without a selection and without a segment map.
extern "C" void cbxh_ordinal_rows(const int64_t* ord, int64_t n_ord, int64_t n, const int64_t* rec_off, const int32_t* rec_len,
                                  int32_t stride, int64_t first_record_id, int64_t* o_off, int32_t* o_len, int64_t* o_id,
                                  int32_t* o_seg) {
    for (int64_t j = 0; j < n_ord; j++) {
        KmRow r;
        (void)km_ordinal_row(ord[j], n, rec_off, rec_len, stride, first_record_id, r);
        o_off[j] = r.rec_off; o_len[j] = r.rec_len; o_id[j] = r.record_id; o_seg[j] = r.segment;
    }
}
