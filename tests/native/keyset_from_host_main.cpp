// TEST PROGRAM: the key-set-from-records host shim (keyset_from_host.cpp) with a main of its own, built with
// -fsanitize=address,undefined by tests/test_keyset_from.py and run on the CPU.  The case comes from a file the test
// writes (both plans' field tables and code pages, both key tables, the source and the probe records), and every array
// is copied into a heap buffer of its exact size, so a read one byte past the data, the offsets, the distinct table, a
// value or its string bytes is reported.  Two sets are built from the source records:
//   fixed:   the records at their stride;
//   framed:  the same records, record i cut to (7 * i) mod stride + 1 bytes -- records end inside and in front of
//            the key fields -- and the last ones end where the data buffer ends.
// Each is probed with the probe records at their stride, as IN and (single-column sets) as NOT IN.  Prints per set
// "<name> source rows <n> nulls <n> keys <n> dropped <n> distinct <n>" and "<name> <in|not_in> kept <n>", and last
// "overflow <status> <flag>" of a build with max_values one below the fixed run's keys.
#include "keyset_from_host.cpp"

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
    int64_t* off = (int64_t*)malloc((size_t)h->n_source * 8 + 1);
    int32_t* len = (int32_t*)malloc((size_t)h->n_source * 4 + 1);
    for (int64_t i = 0; i < h->n_source; i++) { off[i] = i * h->s_stride; len[i] = (int32_t)((7 * i) % h->s_stride + 1); }
    // the last records: lengths that run exactly to the end of the data
    for (int64_t i = h->n_source - 1, back = 1; i >= 0 && back <= h->s_stride; i--, back++) {
        off[i] = s_bytes - back;
        len[i] = (int32_t)back;
    }
    char err[256];
    uint8_t* keep = (uint8_t*)malloc((size_t)h->n_probe ? (size_t)h->n_probe : 1);
    cbx_keyset_source_info* info = (cbx_keyset_source_info*)malloc(sizeof(cbx_keyset_source_info));
    int64_t fixed_keys = 0;
    for (int framed = 0; framed < 2; framed++) {
        const char* name = framed ? "framed" : "fixed";
        cbxh_key_set* set = nullptr;
        int rc = cbxh_keyset_from_records(pf, h->n_pf, 0, pk, sf, h->n_sf, 0, sk, nullptr, s_lut, s_data, s_bytes,
                                          framed ? off : nullptr, framed ? len : nullptr, nullptr, h->n_source,
                                          framed ? 0 : h->s_stride, 0, -1, h->max_values, &set, info, err, sizeof(err));
        if (rc != CBX_OK) { fprintf(stderr, "from_records: %d %s\n", rc, err); return 1; }
        if (!framed) fixed_keys = info->n_source_keys;
        cbx_keyset_info ki;
        cbxh_keyset_info(set, &ki);
        printf("%s source rows %lld nulls %lld keys %lld dropped %lld distinct %lld\n", name, (long long)info->n_rows,
               (long long)info->n_null_rows, (long long)info->n_source_keys, (long long)info->n_dropped, (long long)ki.n_distinct);
        for (int32_t neg = 0; neg < (h->n_keys == 1 ? 2 : 1); neg++) {
            rc = cbxh_keyset_keep(pf, h->n_pf, 0, nullptr, p_lut, p_data, p_bytes, nullptr, nullptr, nullptr, h->n_probe, h->p_stride,
                                  0, -1, &set, &neg, 1, keep, err, sizeof(err));
            if (rc != CBX_OK) { fprintf(stderr, "keep: %d %s\n", rc, err); return 1; }
            long long kept = 0;
            for (int64_t i = 0; i < h->n_probe; i++) kept += keep[i];
            printf("%s %s kept %lld\n", name, neg ? "not_in" : "in", kept);
        }
        cbxh_keyset_destroy(set);
    }
    if (fixed_keys > 1) {
        cbxh_key_set* set = nullptr;
        const int rc = cbxh_keyset_from_records(pf, h->n_pf, 0, pk, sf, h->n_sf, 0, sk, nullptr, s_lut, s_data, s_bytes, nullptr,
                                                nullptr, nullptr, h->n_source, h->s_stride, 0, -1, fixed_keys - 1, &set, info, err,
                                                sizeof(err));
        printf("overflow %d %d\n", rc, (int)info->overflow);
        if (set) cbxh_keyset_destroy(set);
    }
    free(h); free(pf); free(sf); free(p_lut); free(s_lut); free(p_data); free(s_data); free(pk); free(sk); free(off); free(len);
    free(keep); free(info);
    return 0;
}
