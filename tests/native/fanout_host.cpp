// TEST SHIM: runs the host/device part of cobrix_amd/csrc/cbx_keymap_rows.h (the scatter's placement rule with its
// bound check, the cursor check, the sorting network, the wave-first search, the in-window locate, the output-row
// rule, the refusals) on the host, in front of the key-map shim (keymap_host.cpp), so row lists and a fan-out join can
// be compared with a Python model over the oracle's rows without a GPU.  The scatter visits the source records LAST
// TO FIRST, so every segment longer than one arrives unsorted and the network has work to do; the expand walks the
// outputs in "waves" of 64 exactly as fanout_emit_kernel does.  Compiled by tests/test_fanout.py with hipcc (host path
// of the __host__ __device__ functions) and, with a main of its own, by tests/native/fanout_host_main.cpp under the
// sanitizers; never part of the product library.
#include "keymap_host.cpp"

#include "cbx_keymap_rows.h"

// Exact-size copies (a write one entry past a member's segment at the end of the list is a heap overflow).
struct cbxh_row_lists {
    int64_t n_values = 0, cap = 0, bad_slots = 0, mismatches = 0;
    int64_t* row_start = nullptr;   // [n_values + 1]
    int64_t* rows = nullptr;        // [cap]
    uint64_t* cursor = nullptr;     // [n_values]
    ~cbxh_row_lists() { free(row_start); free(rows); free(cursor); }
};

// As cbx_key_map_index_rows, on the host, over ANY source with the source plan's layout (the arguments of
// cbxh_keymap_from_records).  The lists are returned whatever the check finds: bad_slots / mismatches say what the
// device call would turn into CBX_E_STATE.
extern "C" int cbxh_fanout_index_rows(const cbxh_key_map* M, const cbx_field* pf, int32_t n_pf, int32_t p_walk,
                                      const cbx_group_by* pk, const cbx_field* sf, int32_t n_sf, int32_t s_walk,
                                      const cbx_group_by* sk, const cbx_filter* fl, const uint32_t* lut, const uint8_t* data,
                                      int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg,
                                      int64_t n_rec, int32_t stride, int32_t start_off, int32_t segment, cbxh_row_lists** out,
                                      char* err, int32_t err_cap) {
    *out = nullptr;
    std::string e;
    std::vector<GrpProg> probe(1);
    std::vector<KsfProg> ksf(1);
    std::vector<FilterProg> flt(1);
    int rc = keyset_from_build(pf, n_pf, p_walk != 0, pk, sf, n_sf, s_walk != 0, sk, probe.data(), ksf.data(), e);
    if (rc == CBX_OK && fl) rc = filter_build(sf, n_sf, s_walk != 0, fl, flt.data(), e);
    if (rc != CBX_OK) { put_err(e, err, err_cap); return rc; }
    const KsTable& t = M->set->t;
    const int64_t nv = t.n_values;
    cbxh_row_lists* R = new cbxh_row_lists();
    R->n_values = nv;
    R->row_start = (int64_t*)malloc((size_t)(nv + 1) * 8);
    R->cursor = (uint64_t*)malloc(nv ? (size_t)nv * 8 : 1);
    int64_t total = 0;
    for (int64_t j = 0; j < nv; j++) { R->row_start[j] = total; total += M->n_rows[j]; R->cursor[j] = 0; }
    R->row_start[nv] = total;
    R->cap = total;
    R->rows = (int64_t*)malloc(total ? (size_t)total * 8 : 1);
    for (int64_t i = 0; i < total; i++) R->rows[i] = -1;
    const Source src{data, n_bytes, rec_off, rec_len, rec_seg, stride, segment};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    const GrpHostTab stab{&ksf[0].src};
    const HostKmOps ops;
    for (int64_t i = n_rec - 1; i >= 0; i--) {
        const GrpRec me = src(i);
        if (fl) {
            const FilterHostTab ftab{flt.data()};
            if (!filter_keep(ftab, flt[0].pool, me.rec, me.avail, me.head, start_off, me.seg, lutf)) continue;
        }
        const int64_t j = km_lookup(stab, t, me, start_off, lutf);
        if (j >= 0 && !km_place(ops, R->row_start, M->n_rows, R->cursor, R->rows, R->cap, j, i)) R->bad_slots++;
    }
    for (int64_t j = 0; j < nv; j++)
        rows_bitonic(R->rows + R->row_start[j], R->row_start[j + 1] - R->row_start[j], 0, 1, [] {});
    for (int64_t j = 0; j < nv; j++)
        if (!km_cursor_ok((int64_t)R->cursor[j], M->n_rows[j], R->rows[R->row_start[j]], M->first_row[j])) R->mismatches++;
    *out = R;
    return CBX_OK;
}

extern "C" void cbxh_fanout_lists_destroy(cbxh_row_lists* R) { delete R; }
extern "C" int64_t cbxh_fanout_lists(const cbxh_row_lists* R, int64_t* row_start, int64_t* rows, int64_t* bad_slots,
                                     int64_t* mismatches) {
    for (int64_t j = 0; row_start && j <= R->n_values; j++) row_start[j] = R->row_start[j];
    for (int64_t i = 0; rows && i < R->cap; i++) rows[i] = R->rows[i];
    if (bad_slots) *bad_slots = R->bad_slots;
    if (mismatches) *mismatches = R->mismatches;
    return R->cap;
}

// As cbx_join_records_expand, on the host.  fact / match NULL: the count-only form.  Otherwise they hold exactly
// `capacity` entries and T > capacity returns CBX_E_CAPACITY with nothing written.
extern "C" int cbxh_fanout_expand(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                  const uint32_t* lut, const uint8_t* data, int64_t n_bytes, const int64_t* rec_off,
                                  const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec, int32_t stride, int32_t start_off,
                                  int32_t segment, const cbxh_key_set* const* sets, const int32_t* negate, int32_t n_sets,
                                  const cbxh_key_map* map, const cbxh_row_lists* lists, int32_t join_type, int64_t capacity,
                                  int64_t* n_out, int64_t* n_kept, int64_t* fact, int64_t* match, char* err, int32_t err_cap) {
    std::string e;
    const bool count_only = !fact && !match && capacity == 0;
    int rc = km_join_check(map != nullptr, true, join_type, count_only || match != nullptr, n_sets, sets != nullptr, e);
    if (rc == CBX_OK) rc = fx_expand_check(lists != nullptr, !count_only, capacity, e);
    std::vector<FilterProg> flt(1);
    if (rc == CBX_OK && fl) rc = filter_build(fields, n_fields, walk_plan != 0, fl, flt.data(), e);
    if (rc != CBX_OK) { put_err(e, err, err_cap); return rc; }
    const Source src{data, n_bytes, rec_off, rec_len, rec_seg, stride, segment};
    auto lutf = [&](uint32_t b) -> uint32_t { return lut[b]; };
    const GrpHostTab mtab{map->set->prog.data()};
    std::vector<int64_t> kept_ord, kept_start, kept_base;
    int64_t T = 0;
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
        // the view of the map the device's test pass probes: (row_start, n_rows)
        if (k) k = km_verdict(join_type, mtab, map->set->t, lists->row_start, map->n_rows, me, start_off, lutf, m, r);
        if (!k) continue;
        kept_ord.push_back(i);
        kept_start.push_back(m);
        kept_base.push_back(T);
        T += fx_count(join_type, r);
    }
    kept_base.push_back(T);
    kept_base.shrink_to_fit();   // (exact size: a window read past n_kept is a heap overflow)
    const int64_t nk = (int64_t)kept_ord.size();
    *n_out = T;
    *n_kept = nk;
    if (count_only) return CBX_OK;
    if (T > capacity) { put_err(fx_capacity_message(T, capacity), err, err_cap); return CBX_E_CAPACITY; }
    for (int64_t o0 = 0; o0 < T; o0 += 64) {
        const int64_t k0 = fx_first_kept(kept_base.data(), nk, o0);
        int64_t window[64];
        for (int l = 0; l < 64; l++) window[l] = kept_base[k0 + l < nk ? k0 + l : nk];
        for (int l = 0; l < 64 && o0 + l < T; l++) {
            const int64_t o = o0 + l;
            const int w = fx_locate([&](int x) -> int64_t { return window[x]; }, o);
            const int64_t k = k0 + w;
            fact[o] = kept_ord[k];
            match[o] = fx_match(lists->rows, lists->cap, kept_start[k], o - window[w]);
        }
    }
    return CBX_OK;
}

extern "C" int cbxh_expand_check(int32_t has_rows, int32_t has_out, int64_t capacity, char* err, int32_t err_cap) {
    std::string e;
    const int rc = fx_expand_check(has_rows != 0, has_out != 0, capacity, e);
    put_err(e, err, err_cap);
    return rc;
}

extern "C" int cbxh_rows_check(int32_t has_map, int32_t same_plan, int64_t n_rec, int64_t map_n_rec, char* err, int32_t err_cap) {
    std::string e;
    const int rc = km_rows_check(has_map != 0, same_plan != 0, n_rec, map_n_rec, e);
    put_err(e, err, err_cap);
    return rc;
}

extern "C" void cbxh_fanout_messages(int64_t needed, int64_t capacity, char* cap_msg, char* differs_msg, int32_t err_cap) {
    put_err(fx_capacity_message(needed, capacity), cap_msg, err_cap);
    put_err(kRowsSourceDiffers, differs_msg, err_cap);
}

// The sorting network as `nthreads` threads would run it, one after the other within a step (m: exactly n entries).
extern "C" void cbxh_rows_sort(int64_t* m, int64_t n, int32_t nthreads) {
    // (steps are separated by the sync callback, which thread 0's call cannot provide for the others: run each
    // thread's share of every step in turn by replaying the network per step)
    int lp = 0;
    while (lp < 62 && (1ll << lp) < n) lp++;
    const int64_t half = (1ll << lp) >> 1;
    for (int lk = 1; lk <= lp; lk++)
        for (int lj = lk - 1; lj >= 0; lj--)
            for (int tid = nthreads - 1; tid >= 0; tid--)
                for (int64_t t = tid; t < half; t += nthreads) {
                    int64_t a, b;
                    cbx::rows_pair(lk, lj, t, a, b);
                    if (b < n && m[a] > m[b]) { const int64_t x = m[a]; m[a] = m[b]; m[b] = x; }
                }
}

extern "C" void cbxh_fanout_bounds(int32_t* short_max, int32_t* lds_max, int32_t* outputs_per_workgroup) {
    *short_max = kRowsShortMax; *lds_max = kRowsLdsMax; *outputs_per_workgroup = kFxThreads;
}
