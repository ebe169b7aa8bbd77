// TEST PROGRAM: the fan-out host shim (fanout_host.cpp) with a main of its own, built with
// -fsanitize=address,undefined by tests/test_fanout.py and run on the CPU.  The case file is the one of
// keymap_host_main.cpp (both plans' field tables and code pages, both key tables, the source and the probe records);
// every array is copied into a heap buffer of its exact size, and the shim's lists, cursors and kept-row arrays are
// exact-size too, so a write one entry past a member's segment or a window read past the kept rows is reported.
// A map is built from the source records at their stride.  Then:
//   lists:    the row lists from the same source.  Prints "lists rows <total> bad <n> mismatch <n> sum <sum of all
//             ordinals> firsts <sum of each segment's first entry> sorted <1|0>".
//   expand:   INNER and LEFT over the probe records: count-only, then capacity T - 1 into sentinel-filled buffers,
//             then capacity T.  Prints "<inner|left> out <T> kept <n> short <rc> untouched <1|0> fact <sum> match <sum
//             of match >= 0> unmatched <n>".
//   other:    the row lists from a DIFFERENT source with the same record count (the records in reverse order).  Prints
//             "other bad <n> mismatch <n>"; no write may land outside the list (the sanitizer) .
#include "fanout_host.cpp"

#include <stdio.h>
#include <stdlib.h>

namespace {
struct CaseHeader {
    int32_t n_pf, n_sf, p_stride, s_stride, n_keys, reserved;
    int64_t n_probe, n_source, max_values;
    int32_t p_keys[CBX_GROUP_MAX_KEYS];
    int32_t s_keys[CBX_GROUP_MAX_KEYS];
};

template <typename T>
T* exact(FILE* f, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s case-file\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    CaseHeader* h = exact<CaseHeader>(f, 1);
    cbx_field* pf = exact<cbx_field>(f, (size_t)h->n_pf);
    cbx_field* sf = exact<cbx_field>(f, (size_t)h->n_sf);
    uint32_t* p_lut = exact<uint32_t>(f, 256);
    uint32_t* s_lut = exact<uint32_t>(f, 256);
    const int64_t p_bytes = h->n_probe * h->p_stride, s_bytes = h->n_source * h->s_stride;
    uint8_t* p_data = exact<uint8_t>(f, (size_t)p_bytes);
    uint8_t* s_data = exact<uint8_t>(f, (size_t)s_bytes);
    fclose(f);
    cbx_group_by* pk = (cbx_group_by*)calloc(1, sizeof(cbx_group_by));
    cbx_group_by* sk = (cbx_group_by*)calloc(1, sizeof(cbx_group_by));
    pk->n_keys = sk->n_keys = h->n_keys;
    for (int k = 0; k < h->n_keys; k++) { pk->fields[k] = h->p_keys[k]; sk->fields[k] = h->s_keys[k]; }
    char err[256];
    cbx_keymap_info* info = (cbx_keymap_info*)malloc(sizeof(cbx_keymap_info));
    cbxh_key_map* map = nullptr;
    int rc = cbxh_keymap_from_records(pf, h->n_pf, 0, pk, sf, h->n_sf, 0, sk, nullptr, s_lut, s_data, s_bytes, nullptr, nullptr,
                                      nullptr, h->n_source, h->s_stride, 0, -1, h->max_values, &map, info, err, sizeof(err));
    if (rc != CBX_OK) { fprintf(stderr, "from_records: %d %s\n", rc, err); return 1; }
    cbxh_row_lists* lists = nullptr;
    rc = cbxh_fanout_index_rows(map, pf, h->n_pf, 0, pk, sf, h->n_sf, 0, sk, nullptr, s_lut, s_data, s_bytes, nullptr, nullptr,
                                nullptr, h->n_source, h->s_stride, 0, -1, &lists, err, sizeof(err));
    if (rc != CBX_OK) { fprintf(stderr, "index_rows: %d %s\n", rc, err); return 1; }
    {
        int64_t bad = 0, mism = 0;
        const int64_t total = cbxh_fanout_lists(lists, nullptr, nullptr, &bad, &mism);
        const int64_t nv = cbxh_keymap_payload(map, nullptr, nullptr);
        int64_t* rs = (int64_t*)malloc((size_t)(nv + 1) * 8);
        int64_t* rows = (int64_t*)malloc(total ? (size_t)total * 8 : 1);
        cbxh_fanout_lists(lists, rs, rows, nullptr, nullptr);
        long long sum = 0, firsts = 0;
        int sorted = 1;
        for (int64_t v = 0; v < nv; v++) {
            firsts += rows[rs[v]];
            for (int64_t i = rs[v]; i < rs[v + 1]; i++) {
                sum += rows[i];
                if (i > rs[v] && rows[i - 1] >= rows[i]) sorted = 0;
            }
        }
        printf("lists rows %lld bad %lld mismatch %lld sum %lld firsts %lld sorted %d\n", (long long)total, (long long)bad,
               (long long)mism, sum, firsts, sorted);
        free(rs); free(rows);
    }
    for (int32_t jt = 0; jt < 2; jt++) {
        int64_t T = 0, kept = 0;
        rc = cbxh_fanout_expand(pf, h->n_pf, 0, nullptr, p_lut, p_data, p_bytes, nullptr, nullptr, nullptr, h->n_probe, h->p_stride,
                                0, -1, nullptr, nullptr, 0, map, lists, jt, 0, &T, &kept, nullptr, nullptr, err, sizeof(err));
        if (rc != CBX_OK) { fprintf(stderr, "count: %d %s\n", rc, err); return 1; }
        int short_rc = 0, untouched = 1;
        if (T > 0) {
            int64_t* fs = (int64_t*)malloc((size_t)(T - 1) * 8 ? (size_t)(T - 1) * 8 : 1);
            int64_t* ms = (int64_t*)malloc((size_t)(T - 1) * 8 ? (size_t)(T - 1) * 8 : 1);
            for (int64_t i = 0; i < T - 1; i++) { fs[i] = -7; ms[i] = -7; }
            int64_t t2 = 0, k2 = 0;
            short_rc = cbxh_fanout_expand(pf, h->n_pf, 0, nullptr, p_lut, p_data, p_bytes, nullptr, nullptr, nullptr, h->n_probe,
                                          h->p_stride, 0, -1, nullptr, nullptr, 0, map, lists, jt, T - 1, &t2, &k2, fs, ms, err,
                                          sizeof(err));
            for (int64_t i = 0; i < T - 1; i++) untouched &= fs[i] == -7 && ms[i] == -7;
            untouched &= t2 == T && k2 == kept;
            free(fs); free(ms);
        }
        int64_t* fact = (int64_t*)malloc(T ? (size_t)T * 8 : 1);
        int64_t* match = (int64_t*)malloc(T ? (size_t)T * 8 : 1);
        int64_t t3 = 0, k3 = 0;
        rc = cbxh_fanout_expand(pf, h->n_pf, 0, nullptr, p_lut, p_data, p_bytes, nullptr, nullptr, nullptr, h->n_probe, h->p_stride,
                                0, -1, nullptr, nullptr, 0, map, lists, jt, T, &t3, &k3, fact, match, err, sizeof(err));
        if (rc != CBX_OK || t3 != T || k3 != kept) { fprintf(stderr, "expand: %d %s\n", rc, err); return 1; }
        long long sf_ = 0, sm = 0, un = 0;
        for (int64_t o = 0; o < T; o++) {
            sf_ += fact[o];
            if (match[o] >= 0) sm += match[o]; else un++;
        }
        printf("%s out %lld kept %lld short %d untouched %d fact %lld match %lld unmatched %lld\n", jt ? "left" : "inner",
               (long long)T, (long long)kept, short_rc, untouched, sf_, sm, un);
        free(fact); free(match);
    }
    {
        uint8_t* back = (uint8_t*)malloc(s_bytes ? (size_t)s_bytes : 1);
        for (int64_t i = 0; i < h->n_source; i++)
            memcpy(back + i * h->s_stride, s_data + (h->n_source - 1 - i) * h->s_stride, (size_t)h->s_stride);
        cbxh_row_lists* other = nullptr;
        rc = cbxh_fanout_index_rows(map, pf, h->n_pf, 0, pk, sf, h->n_sf, 0, sk, nullptr, s_lut, back, s_bytes, nullptr, nullptr,
                                    nullptr, h->n_source, h->s_stride, 0, -1, &other, err, sizeof(err));
        if (rc != CBX_OK) { fprintf(stderr, "other: %d %s\n", rc, err); return 1; }
        int64_t bad = 0, mism = 0;
        cbxh_fanout_lists(other, nullptr, nullptr, &bad, &mism);
        printf("other bad %lld mismatch %lld\n", (long long)bad, (long long)mism);
        cbxh_fanout_lists_destroy(other);
        // ... and from n_source copies of source record `reserved` (a member): all but n_rows of them find the segment full
        for (int64_t i = 0; i < h->n_source; i++)
            memcpy(back + i * h->s_stride, s_data + (int64_t)h->reserved * h->s_stride, (size_t)h->s_stride);
        rc = cbxh_fanout_index_rows(map, pf, h->n_pf, 0, pk, sf, h->n_sf, 0, sk, nullptr, s_lut, back, s_bytes, nullptr, nullptr,
                                    nullptr, h->n_source, h->s_stride, 0, -1, &other, err, sizeof(err));
        if (rc != CBX_OK) { fprintf(stderr, "flood: %d %s\n", rc, err); return 1; }
        cbxh_fanout_lists(other, nullptr, nullptr, &bad, &mism);
        printf("flood bad %lld mismatch %lld\n", (long long)bad, (long long)mism);
        cbxh_fanout_lists_destroy(other);
        free(back);
    }
    cbxh_fanout_lists_destroy(lists);
    cbxh_keymap_destroy(map);
    free(h); free(pf); free(sf); free(p_lut); free(s_lut); free(p_data); free(s_data); free(pk); free(sk); free(info);
    return 0;
}
