// TEST SHIM: runs the Top-N stage's host/device part (cobrix_amd/csrc/cbx_topn.h: topn_build, topn_word -- the
// per-record composite-key word the GPU kernels compute per lane -- and topn_pick_digit, the pick step of the
// radix select) on the host, with a sequential restatement of the select / classify / tie-list levels that
// cbx_top_n_records launches as kernels, so the composite key and the chosen rows can be compared with a Python
// encoder and a Python comparator over the oracle's rows without a GPU.  Compiled by tests/test_topn.py with
// hipcc (host path of the __host__ __device__ functions); never part of the product library.
#define CBX_FILTER_HOST_ONLY
#include "cbx_topn.h"

#include <algorithm>
#include <vector>

using namespace cbx;

namespace {
struct Progs {
    std::vector<TopnProg> topn{1};
    std::vector<FilterProg> flt{1};
    bool has_filter = false;
};

void copy_err(const std::string& e, char* err, int32_t err_cap) {
    if (!err || err_cap <= 0) return;
    const size_t n = e.size() < (size_t)err_cap - 1 ? e.size() : (size_t)err_cap - 1;
    memcpy(err, e.data(), n);
    err[n] = 0;
}

int build(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl, const cbx_sort_order* so,
          Progs& p, char* err, int32_t err_cap) {
    std::string e;
    int rc = topn_build(fields, n_fields, walk_plan != 0, so, p.topn.data(), e);
    if (rc == CBX_OK && fl) {
        rc = filter_build(fields, n_fields, walk_plan != 0, fl, p.flt.data(), e);
        p.has_filter = true;
    }
    copy_err(e, err, err_cap);
    return rc;
}

// The records of one source: fixed-length (rec_off == nullptr: data + i * stride, active segment `segment`) or
// framed (clamped to the data as the kernels' flt_record does, active segment rec_seg[i] or -1).
struct Source {
    const uint8_t* data;
    int64_t n_bytes;
    const int64_t* rec_off;
    const int32_t* rec_len;
    const int32_t* rec_seg;
    int64_t n_rec;
    int32_t stride, start_off, segment;
    GrpRec rec(int64_t i) const {
        if (!rec_off) return GrpRec{data + i * (int64_t)stride, stride, i * (int64_t)stride, segment};
        int64_t off = rec_off[i], len = rec_len[i];
        if (off < 0 || off > n_bytes) { off = 0; len = 0; }
        if (len > n_bytes - off) len = n_bytes - off;
        if (len < 0) len = 0;
        return GrpRec{data + off, (int)len, off, rec_seg ? rec_seg[i] : -1};
    }
};

uint64_t word_of(const Progs& p, const Source& s, const uint32_t* lut, int level, int64_t i) {
    const GrpRec r = s.rec(i);
    const TopnHostTab tab{p.topn.data()};
    return topn_word(tab, level, r.rec, r.avail, r.head, s.start_off, r.seg, i, [&](uint32_t b) -> uint32_t { return lut[b]; });
}
}  // namespace

// out_words[i * levels_total + l] = word l of record i's composite key (the source index word included).
// Returns topn_build's status (reason copied to err); *levels_total and words_per_key are set on CBX_OK.
extern "C" int cbxh_topn_words(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_sort_order* so,
                               const uint32_t* lut, const uint8_t* data, int64_t n_bytes, const int64_t* rec_off,
                               const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec, int32_t stride,
                               int32_t start_off, int32_t segment, uint64_t* out_words, int64_t out_cap,
                               int32_t* levels_total, int32_t* words_per_key, char* err, int32_t err_cap) {
    Progs p;
    const int rc = build(fields, n_fields, walk_plan, nullptr, so, p, err, err_cap);
    if (rc != CBX_OK) return rc;
    const int lt = p.topn[0].n_words + 1;
    *levels_total = lt;
    for (int k = 0; k < CBX_TOPN_MAX_KEYS; k++) words_per_key[k] = k < p.topn[0].n_keys ? topn_words_of_key(p.topn[0], k) : 0;
    const Source s{data, n_bytes, rec_off, rec_len, rec_seg, n_rec, stride, start_off, segment};
    if (out_cap < n_rec * lt) { copy_err("out_words too small", err, err_cap); return CBX_E_CAPACITY; }
    for (int64_t i = 0; i < n_rec; i++)
        for (int l = 0; l < lt; l++) out_words[i * lt + l] = word_of(p, s, lut, l, i);
    return CBX_OK;
}

// The rows cbx_top_n_records returns, as ascending source indices in out_idx (capacity min(limit, n_rec)), and how
// the levels ran.  The levels follow the library's host loop step by step: the level-0 candidates are the live
// records, a round counts the candidates matching the prefix into 256 bins and fixes a digit with
// topn_pick_digit, classify keeps word < T (and the whole tie class when exactly `need` remain), the tie class
// goes to the next level.
extern "C" int cbxh_topn_select(const cbx_field* fields, int32_t n_fields, int32_t walk_plan, const cbx_filter* fl,
                                const cbx_sort_order* so, const uint32_t* lut, const uint8_t* data, int64_t n_bytes,
                                const int64_t* rec_off, const int32_t* rec_len, const int32_t* rec_seg, int64_t n_rec,
                                int32_t stride, int32_t start_off, int32_t segment, int64_t limit, int64_t* out_idx,
                                int64_t* n_out, cbx_topn_info* info, char* err, int32_t err_cap) {
    Progs p;
    const int rc = build(fields, n_fields, walk_plan, fl, so, p, err, err_cap);
    if (rc != CBX_OK) return rc;
    if (limit < 0) { copy_err("limit < 0", err, err_cap); return CBX_E_ARGUMENT; }
    *n_out = 0;
    memset(info, 0, sizeof(*info));
    info->levels_total = p.topn[0].n_words + 1;
    for (int k = 0; k < p.topn[0].n_keys; k++) info->words_per_key[k] = topn_words_of_key(p.topn[0], k);
    if (n_rec == 0) return CBX_OK;
    if (limit == 0) { info->n_live = -1; return CBX_OK; }
    const Source s{data, n_bytes, rec_off, rec_len, rec_seg, n_rec, stride, start_off, segment};
    std::vector<int64_t> cand;
    for (int64_t i = 0; i < n_rec; i++) {
        bool keep = true;
        if (p.has_filter) {
            const GrpRec r = s.rec(i);
            const FilterHostTab tab{p.flt.data()};
            keep = filter_keep(tab, p.flt[0].pool, r.rec, r.avail, r.head, start_off, r.seg, [&](uint32_t b) -> uint32_t { return lut[b]; });
        }
        if (keep) cand.push_back(i);
    }
    info->n_live = (int64_t)cand.size();
    std::vector<int64_t> kept;
    if (limit >= n_rec) {
        kept = cand;
    } else {
        uint64_t need = (uint64_t)limit;
        for (int level = 0;; level++) {
            std::vector<uint64_t> w(cand.size());
            for (size_t c = 0; c < cand.size(); c++) w[c] = word_of(p, s, lut, level, cand[c]);
            info->levels_run = level + 1;
            if (level == 0 && need >= cand.size()) { kept = cand; break; }   // (the kernels' TS_ALL)
            uint64_t prefix = 0, ties = 0;
            for (int round = 0; round < 8; round++) {
                const int shift = 56 - 8 * round;
                const uint64_t mask = round == 0 ? 0ull : ~0ull << (64 - 8 * round);
                uint32_t bins[256] = {};
                for (uint64_t x : w)
                    if (((x ^ prefix) & mask) == 0) bins[(x >> shift) & 0xFF]++;
                uint64_t below;
                const int d = topn_pick_digit(bins, 256, need, below);
                prefix |= (uint64_t)d << shift;
                need -= below;
                ties = bins[d];
            }
            std::vector<int64_t> next;
            for (size_t c = 0; c < cand.size(); c++) {
                if (w[c] < prefix || (w[c] == prefix && ties == need)) kept.push_back(cand[c]);
                else if (w[c] == prefix) next.push_back(cand[c]);
            }
            if (ties == need) break;
            if (level + 1 >= info->levels_total) { copy_err("the source index did not decide", err, err_cap); return CBX_E_STATE; }
            if (level == 0) info->ties_after_level0 = (int64_t)ties;
            info->ties_max = std::max<int64_t>(info->ties_max, (int64_t)ties);
            cand.swap(next);
        }
    }
    std::sort(kept.begin(), kept.end());
    for (size_t k = 0; k < kept.size(); k++) out_idx[k] = kept[k];
    *n_out = (int64_t)kept.size();
    return CBX_OK;
}
