// TEST PROGRAM: the grouped-aggregate host shim (group_host.cpp) with a main of its own, built with
// -fsanitize=address,undefined by tests/test_group.py and run on the CPU.  The case comes from a file the test
// writes (the plan's field table, code page, tables and records), and every array is copied into a heap buffer
// of its exact size, so a read one byte past the data, the offsets or a table is reported.  Three runs:
//   fixed:   the records at their stride;
//   framed:  the same records, record i cut to (7 * i) mod (stride + 1) bytes -- records end inside the key and
//            value fields, and the last ones end where the data buffer ends;
//   tight:   the fixed run with max_groups = the number of groups the first run found (must not overflow) and,
//            when there are at least two groups, one less (must overflow).
// Prints one line per run: "<name> groups <n> rows <n> overflow <0|1>".
#include "group_host.cpp"

#include <stdio.h>
#include <stdlib.h>

namespace {
struct CaseHeader {
    int32_t n_fields, stride, n_keys, n_terms;
    int64_t n_rec, max_groups;
    int32_t keys[CBX_GROUP_MAX_KEYS];
    int32_t term_field[CBX_AGG_MAX_TERMS];
    int32_t term_funcs[CBX_AGG_MAX_TERMS];
};

template <typename T>
T* exact(FILE* f, size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}

struct Out {
    int64_t* rows;
    cbx_aggregate_value* values;
    cbx_group_key* keys;
    uint8_t* bytes;
    cbx_group_output o;
    Out(int64_t mg, int nt, int nk, int str_stride) {
        rows = (int64_t*)malloc((size_t)mg * 8);
        values = nt ? (cbx_aggregate_value*)malloc((size_t)mg * nt * sizeof(cbx_aggregate_value)) : nullptr;
        keys = (cbx_group_key*)malloc((size_t)mg * nk * sizeof(cbx_group_key));
        bytes = str_stride ? (uint8_t*)malloc((size_t)mg * str_stride) : nullptr;
        o = cbx_group_output{rows, values, keys, bytes};
    }
    ~Out() { free(rows); free(values); free(keys); free(bytes); }
};
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
    fclose(f);
    cbx_aggregate* ag = (cbx_aggregate*)calloc(1, sizeof(cbx_aggregate));
    ag->n_terms = h->n_terms;
    for (int t = 0; t < h->n_terms; t++) { ag->terms[t].field = h->term_field[t]; ag->terms[t].funcs = h->term_funcs[t]; }
    cbx_group_by* gb = (cbx_group_by*)calloc(1, sizeof(cbx_group_by));
    gb->n_keys = h->n_keys;
    for (int k = 0; k < h->n_keys; k++) gb->fields[k] = h->keys[k];
    int64_t* off = (int64_t*)malloc((size_t)h->n_rec * 8 + 1);
    int32_t* len = (int32_t*)malloc((size_t)h->n_rec * 4 + 1);
    for (int64_t i = 0; i < h->n_rec; i++) { off[i] = i * h->stride; len[i] = (int32_t)((7 * i) % (h->stride + 1)); }
    // the last records: lengths that run exactly to the end of the data
    for (int64_t i = h->n_rec - 1, back = 1; i >= 0 && back <= h->stride; i--, back++) {
        off[i] = n_bytes - back;
        len[i] = (int32_t)back;
    }
    char err[256];
    cbx_group_strides S;
    int rc = cbxh_group_strides(fields, h->n_fields, 0, ag, gb, h->max_groups, &S, err, sizeof(err));
    if (rc != CBX_OK) { fprintf(stderr, "strides: %d %s\n", rc, err); return 1; }
    int status = 0;
    int64_t found = 0;
    {
        Out out(h->max_groups, h->n_terms, h->n_keys, S.str_stride);
        cbx_group_header hd;
        rc = cbxh_group_fixed(fields, h->n_fields, 0, nullptr, ag, gb, lut, data, h->n_rec, h->stride, 0, -1, 3, h->max_groups,
                              &out.o, &hd, err, sizeof(err));
        if (rc != CBX_OK) { fprintf(stderr, "fixed: %d %s\n", rc, err); return 1; }
        printf("fixed groups %lld rows %lld overflow %d\n", (long long)hd.n_groups, (long long)hd.n_rows, hd.overflow);
        found = hd.n_groups;
        rc = cbxh_group_framed(fields, h->n_fields, 0, nullptr, ag, gb, lut, data, n_bytes, off, len, nullptr, h->n_rec, 0, 3,
                               h->max_groups, &out.o, &hd, err, sizeof(err));
        if (rc != CBX_OK) { fprintf(stderr, "framed: %d %s\n", rc, err); return 1; }
        printf("framed groups %lld rows %lld overflow %d\n", (long long)hd.n_groups, (long long)hd.n_rows, hd.overflow);
    }
    for (int64_t mg = found; mg >= 1 && mg >= found - 1; mg--) {
        Out out(mg, h->n_terms, h->n_keys, S.str_stride);
        cbx_group_header hd;
        rc = cbxh_group_fixed(fields, h->n_fields, 0, nullptr, ag, gb, lut, data, h->n_rec, h->stride, 0, -1, 1, mg, &out.o, &hd,
                              err, sizeof(err));
        if (rc != CBX_OK) { fprintf(stderr, "tight: %d %s\n", rc, err); return 1; }
        printf("tight groups %lld rows %lld overflow %d\n", (long long)hd.n_groups, (long long)hd.n_rows, hd.overflow);
        if ((mg == found) == (hd.overflow != 0)) status = 1;
    }
    free(h); free(fields); free(lut); free(data); free(ag); free(gb); free(off); free(len);
    return status;
}
