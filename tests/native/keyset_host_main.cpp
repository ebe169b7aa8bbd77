// TEST PROGRAM: the key-set host shim (keyset_host.cpp) with a main of its own, built with
// -fsanitize=address,undefined by tests/test_keyset.py and run on the CPU.  The case comes from a file the test
// writes (the plan's field table, code page, key table, records and key values), and every array is copied into a
// heap buffer of its exact size, so a read one byte past the data, the offsets, a value, its string bytes or the
// table is reported.  Runs, each as IN and (single-column sets) as NOT IN:
//   fixed:   the records at their stride;
//   framed:  the same records, record i cut to (7 * i) mod stride + 1 bytes -- records end inside and in front of
//            the key fields -- and the last ones end where the data buffer ends.
// Prints one line per run: "<name> <in|not_in> kept <n>", and first "set distinct <n> max_probe <n>".
#include "keyset_host.cpp"

#include <stdio.h>
#include <stdlib.h>

namespace {
struct CaseHeader {
    int32_t n_fields, stride, n_keys, str_stride;
    int64_t n_rec, n_values;
    int32_t keys[CBX_GROUP_MAX_KEYS];
    int32_t str_off[CBX_GROUP_MAX_KEYS];
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
    cbx_field* fields = exact<cbx_field>(f, (size_t)h->n_fields);
    uint32_t* lut = exact<uint32_t>(f, 256);
    const int64_t n_bytes = h->n_rec * h->stride;
    uint8_t* data = exact<uint8_t>(f, (size_t)n_bytes);
    cbx_key_value* values = exact<cbx_key_value>(f, (size_t)(h->n_values * h->n_keys));
    uint8_t* bytes = exact<uint8_t>(f, (size_t)(h->n_values * h->str_stride));
    fclose(f);
    cbx_group_by* gb = (cbx_group_by*)calloc(1, sizeof(cbx_group_by));
    gb->n_keys = h->n_keys;
    for (int k = 0; k < h->n_keys; k++) gb->fields[k] = h->keys[k];
    int64_t* off = (int64_t*)malloc((size_t)h->n_rec * 8 + 1);
    int32_t* len = (int32_t*)malloc((size_t)h->n_rec * 4 + 1);
    for (int64_t i = 0; i < h->n_rec; i++) { off[i] = i * h->stride; len[i] = (int32_t)((7 * i) % h->stride + 1); }
    // the last records: lengths that run exactly to the end of the data
    for (int64_t i = h->n_rec - 1, back = 1; i >= 0 && back <= h->stride; i--, back++) {
        off[i] = n_bytes - back;
        len[i] = (int32_t)back;
    }
    char err[256];
    cbxh_key_set* set = nullptr;
    int rc = cbxh_keyset_create(fields, h->n_fields, 0, gb, values, bytes, h->str_stride, h->str_off, h->n_values, &set, err,
                                sizeof(err));
    if (rc != CBX_OK) { fprintf(stderr, "create: %d %s\n", rc, err); return 1; }
    cbx_keyset_info info;
    cbxh_keyset_info(set, &info);
    printf("set distinct %lld max_probe %lld\n", (long long)info.n_distinct, (long long)info.max_probe);
    uint8_t* keep = (uint8_t*)malloc((size_t)h->n_rec ? (size_t)h->n_rec : 1);
    for (int framed = 0; framed < 2; framed++) {
        for (int32_t neg = 0; neg < (h->n_keys == 1 ? 2 : 1); neg++) {
            rc = cbxh_keyset_keep(fields, h->n_fields, 0, nullptr, lut, data, n_bytes, framed ? off : nullptr, framed ? len : nullptr,
                                  nullptr, h->n_rec, framed ? 0 : h->stride, 0, -1, &set, &neg, 1, keep, err, sizeof(err));
            if (rc != CBX_OK) { fprintf(stderr, "keep: %d %s\n", rc, err); return 1; }
            long long kept = 0;
            for (int64_t i = 0; i < h->n_rec; i++) kept += keep[i];
            printf("%s %s kept %lld\n", framed ? "framed" : "fixed", neg ? "not_in" : "in", kept);
        }
    }
    cbxh_keyset_destroy(set);
    free(h); free(fields); free(lut); free(data); free(values); free(bytes); free(gb); free(off); free(len); free(keep);
    return 0;
}
