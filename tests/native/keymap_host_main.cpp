// TEST PROGRAM: the key-map host shim (keymap_host.cpp) with a main of its own, built with
// -fsanitize=address,undefined by tests/test_keymap.py and run on the CPU.  The case file is the one of
// keyset_from_host_main.cpp (both plans' field tables and code pages, both key tables, the source and the probe
// records), and every array is copied into a heap buffer of its exact size, so a read one byte past the data, the
// offsets, the table, a value, its string bytes or a payload entry is reported.  Two maps are built from the source:
//   fixed:   the records at their stride;
//   framed:  the same records, record i cut to (7 * i) mod stride + 1 bytes, the last ones ending where the data ends.
// Each is probed with the probe records at their stride as INNER and as LEFT.  Prints per map
// "<name> map values <n> dup <n> max <n> pins <n> first <sum of first_row> rows <sum of n_rows>" and per join
// "<name> <inner|left> kept <n> matched <n> match <sum of match >= 0> rows <sum of rows>", and last
// "ordinals <sum of offsets> <sum of lengths> <sum of record ids>" of a gather with repeated, descending and
// out-of-range ordinals over the framed source.
#include "keymap_host.cpp"

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
    const size_t ns = (size_t)h->n_source, np = (size_t)h->n_probe;
    int64_t* off = (int64_t*)malloc(ns ? ns * 8 : 1);
    int32_t* len = (int32_t*)malloc(ns ? ns * 4 : 1);
    for (int64_t i = 0; i < h->n_source; i++) { off[i] = i * h->s_stride; len[i] = (int32_t)((7 * i) % h->s_stride + 1); }
    for (int64_t i = h->n_source - 1, back = 1; i >= 0 && back <= h->s_stride; i--, back++) {
        off[i] = s_bytes - back;
        len[i] = (int32_t)back;
    }
    char err[256];
    uint8_t* keep = (uint8_t*)malloc(np ? np : 1);
    int64_t* match = (int64_t*)malloc(np ? np * 8 : 1);
    int64_t* rows = (int64_t*)malloc(np ? np * 8 : 1);
    cbx_keymap_info* info = (cbx_keymap_info*)malloc(sizeof(cbx_keymap_info));
    for (int framed = 0; framed < 2; framed++) {
        const char* name = framed ? "framed" : "fixed";
        cbxh_key_map* map = nullptr;
        int rc = cbxh_keymap_from_records(pf, h->n_pf, 0, pk, sf, h->n_sf, 0, sk, nullptr, s_lut, s_data, s_bytes,
                                          framed ? off : nullptr, framed ? len : nullptr, nullptr, h->n_source,
                                          framed ? 0 : h->s_stride, 0, -1, h->max_values, &map, info, err, sizeof(err));
        if (rc != CBX_OK) { fprintf(stderr, "from_records: %d %s\n", rc, err); return 1; }
        const int64_t nv = cbxh_keymap_payload(map, nullptr, nullptr);
        int64_t* fr = (int64_t*)malloc(nv ? (size_t)nv * 8 : 1);
        int64_t* nr = (int64_t*)malloc(nv ? (size_t)nv * 8 : 1);
        cbxh_keymap_payload(map, fr, nr);
        long long sf_ = 0, sr_ = 0;
        for (int64_t j = 0; j < nv; j++) { sf_ += fr[j]; sr_ += nr[j]; }
        free(fr); free(nr);
        printf("%s map values %lld dup %lld max %lld pins %lld first %lld rows %lld\n", name, (long long)nv,
               (long long)info->n_duplicate_keys, (long long)info->max_rows_per_key, (long long)cbxh_keymap_pin_failures(map), sf_, sr_);
        for (int32_t jt = 0; jt < 2; jt++) {
            rc = cbxh_keymap_join(pf, h->n_pf, 0, nullptr, p_lut, p_data, p_bytes, nullptr, nullptr, nullptr, h->n_probe, h->p_stride,
                                  0, -1, nullptr, nullptr, 0, map, jt, keep, match, rows, err, sizeof(err));
            if (rc != CBX_OK) { fprintf(stderr, "join: %d %s\n", rc, err); return 1; }
            long long kept = 0, matched = 0, sm = 0, sr = 0;
            for (int64_t i = 0; i < h->n_probe; i++) {
                if (!keep[i]) continue;
                kept++;
                if (match[i] >= 0) { matched++; sm += match[i]; }
                sr += rows[i];
            }
            printf("%s %s kept %lld matched %lld match %lld rows %lld\n", name, jt ? "left" : "inner", kept, matched, sm, sr);
        }
        cbxh_keymap_destroy(map);
    }
    {
        const int64_t n = h->n_source, n_ord = 6;
        int64_t* ord = (int64_t*)malloc((size_t)n_ord * 8);
        ord[0] = n - 1; ord[1] = n - 1; ord[2] = n / 2; ord[3] = 0; ord[4] = n; ord[5] = -1;
        int64_t* o_off = (int64_t*)malloc((size_t)n_ord * 8);
        int32_t* o_len = (int32_t*)malloc((size_t)n_ord * 4);
        int64_t* o_id = (int64_t*)malloc((size_t)n_ord * 8);
        int32_t* o_seg = (int32_t*)malloc((size_t)n_ord * 4);
        cbxh_ordinal_rows(ord, n_ord, n, off, len, 0, 1000, o_off, o_len, o_id, o_seg);
        long long a = 0, b = 0, c = 0;
        for (int64_t j = 0; j < n_ord; j++) { a += o_off[j]; b += o_len[j]; c += o_id[j]; }
        printf("ordinals %lld %lld %lld\n", a, b, c);
        free(ord); free(o_off); free(o_len); free(o_id); free(o_seg);
    }
    free(h); free(pf); free(sf); free(p_lut); free(s_lut); free(p_data); free(s_data); free(pk); free(sk); free(off); free(len);
    free(keep); free(match); free(rows); free(info);
    return 0;
}
