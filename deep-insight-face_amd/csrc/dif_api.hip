// C ABI entry points (include/dif.h): error plumbing, distances, gallery + match.
// The embedding network entry points live in net_api.hip.
#include "../../include/dif.h"
#include "dif_internal.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <new>

namespace dif {

static thread_local char g_err[1024] = "";

int set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}

static int check_metric(int metric) {
  if (metric != DIF_METRIC_SQL2 && metric != DIF_METRIC_COSINE)
    return set_error("Undefined distance metric %d", metric);   // evaluation/utility.py:64
  return 0;
}

}  // namespace dif

using namespace dif;

template <class P>
static int regrow(P** p, size_t keep_bytes, size_t new_bytes, hipStream_t st) {
  P* q = nullptr;
  DIF_HIP(hipMalloc(&q, new_bytes));
  if (*p && keep_bytes) {
    hipError_t e = hipMemcpyAsync(q, *p, keep_bytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      (void)hipFree(q);
      return set_error("dif_gallery_reserve: copy failed: %s", hipGetErrorString(e));
    }
  }
  if (*p) DIF_HIP(hipFree(*p));
  *p = q;
  return 0;
}


struct dif_gallery {
  Gallery g;
};

extern "C" {

int dif_version(void) { return DIF_VERSION; }

const char* dif_last_error(void) { return g_err; }

int dif_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dif_pairwise(const float* e1_dev, int64_t n1, const float* e2_dev, int64_t n2, int d, int metric,
                 float* out_dev, void* stream) {
  if (metric != DIF_METRIC_SIMILARITY && check_metric(metric)) return -1;
  if (d <= 0) return set_error("dif_pairwise: d must be positive (got %d)", d);
  if (n1 < 0 || n2 < 0) return set_error("dif_pairwise: negative row count");
  if (n1 != n2 && n1 != 1 && n2 != 1)
    return set_error("dif_pairwise: shapes (%lld,%d) and (%lld,%d) do not broadcast", (long long)n1, d,
                     (long long)n2, d);
  if (n1 == 0 || n2 == 0) return 0;
  if (!e1_dev || !e2_dev || !out_dev) return set_error("dif_pairwise: null pointer");
  return pairwise_run(e1_dev, n1, e2_dev, n2, d, metric, out_dev, (hipStream_t)stream);
}

int dif_gallery_create(dif_gallery** out, int d) {
  if (!out) return set_error("dif_gallery_create: null out");
  if (d <= 0 || d % 32 != 0)
    return set_error("dif_gallery_create: embedding size must be a positive multiple of 32 (got %d)", d);
  dif_gallery* h = new (std::nothrow) dif_gallery();
  if (!h) return set_error("dif_gallery_create: out of host memory");
  h->g.d = d;
  *out = h;
  return 0;
}

int dif_gallery_destroy(dif_gallery* h) {
  if (!h) return 0;
  Gallery& g = h->g;
  if (g.rows) (void)hipFree(g.rows);
  if (g.rows2) (void)hipFree(g.rows2);
  if (g.rows1) (void)hipFree(g.rows1);
  if (g.probes2) (void)hipFree(g.probes2);
  if (g.sq) (void)hipFree(g.sq);
  if (g.ninv) (void)hipFree(g.ninv);
  for (void* p : {(void*)g.part_key, (void*)g.part_cnt, (void*)g.part_idx, (void*)g.eps, (void*)g.eps32, (void*)g.best,
                  (void*)g.best_dist, (void*)g.flagged, (void*)g.nflag, (void*)g.sqmax_bits, (void*)g.hi,
                  (void*)g.pcls, (void*)g.anti_cnt, (void*)g.anti_idx, (void*)g.flags, (void*)g.within_census,
                  (void*)g.within_thr, (void*)g.rank_mate, (void*)g.remove_ws, (void*)g.topk_min, (void*)g.cluster_parent,
                  (void*)g.cluster_bad, (void*)g.dbscan_degree, (void*)g.dbscan_anchor, (void*)g.roc_mask, (void*)g.roc_thr, (void*)g.roc_tab, (void*)g.roc_bins,
                  (void*)g.topk_ids_stat, (void*)g.topk_tagged_stat, (void*)g.within_tagged_stat})
    if (p) (void)hipFree(p);
  delete h;
  return 0;
}

int dif_gallery_set(dif_gallery* h, const float* rows_dev, int64_t n, int64_t index_base, void* stream) {
  if (!h) return set_error("dif_gallery_set: null handle");
  if (n < 0) return set_error("dif_gallery_set: negative row count");
  if (n > 0x7ffffff0LL) return set_error("dif_gallery_set: at most 2^31-16 rows per shard");
  if (n > 0 && !rows_dev) return set_error("dif_gallery_set: null rows");
  Gallery& g = h->g;
  hipStream_t st = (hipStream_t)stream;
  if (n > g.cap) {
    DIF_HIP(hipStreamSynchronize(st));
    if (g.rows) DIF_HIP(hipFree(g.rows));
    if (g.rows2) DIF_HIP(hipFree(g.rows2));
    if (g.rows1) DIF_HIP(hipFree(g.rows1));
    g.rows1 = nullptr;
    if (g.sq) DIF_HIP(hipFree(g.sq));
    if (g.ninv) DIF_HIP(hipFree(g.ninv));
    g.rows = g.rows2 = g.sq = g.ninv = nullptr;
    g.cap = 0;
    g.n = 0;                                               // an allocation failure below leaves an EMPTY gallery, not dangling rows
    g.rows2_refused = g.rows1_refused = false;
    DIF_HIP(hipMalloc(&g.rows, (size_t)n * g.d * sizeof(float)));
    DIF_HIP(hipMalloc(&g.sq, (size_t)n * sizeof(float)));
    DIF_HIP(hipMalloc(&g.ninv, (size_t)n * sizeof(float)));
    g.cap = n;
    // the split-bf16 copy the filter reads (as large as the rows themselves) is allocated by gallery_split_copy,
    // from gallery_norms below or from the first dif_match after "filter" was switched on: NOT fatal when it does
    // not fit -- the f32 filter needs no copy and gives the same answers
  }
  g.n = n;
  g.index_base = index_base;
  g.rows2_valid = g.rows1_valid = false;
  if (n == 0) return 0;
  return gallery_norms(&g, rows_dev, st);                   // one pass: the copy, the norms and the filter's bf16 copy
}

int dif_gallery_reserve(dif_gallery* h, int64_t capacity, void* stream) {
  if (!h) return set_error("dif_gallery_reserve: null handle");
  if (capacity > 0x7ffffff0LL) return set_error("dif_gallery_reserve: at most 2^31-16 rows per shard");
  Gallery& g = h->g;
  if (capacity <= g.cap) return 0;
  hipStream_t st = (hipStream_t)stream;
  DIF_HIP(hipStreamSynchronize(st));
  const size_t c = (size_t)capacity, n = (size_t)g.n, d = (size_t)g.d;
  if (regrow(&g.rows, n * d * 4, c * d * 4, st)) return -1;
  if (regrow(&g.sq, n * 4, c * 4, st)) return -1;
  if (regrow(&g.ninv, n * 4, c * 4, st)) return -1;
  // the filter's copy: moved when it fits, otherwise dropped (the next dif_match rebuilds it, or the f32 filter serves)
  if (g.rows1) {
    uint16_t* q = nullptr;
    if (hipMalloc(&q, (c + 63) / 64 * 64 * d * 2) == hipSuccess) {   // (whole 64-row tiles: either layout of the first n rows lies inside them)
      if (g.rows1_valid && n) {
        DIF_HIP(hipMemcpyAsync(q, g.rows1, (n + 63) / 64 * 64 * d * 2, hipMemcpyDeviceToDevice, st));
        DIF_HIP(hipStreamSynchronize(st));
      }
    } else {
      (void)hipGetLastError();
      g.rows1_valid = false;
    }
    DIF_HIP(hipFree(g.rows1));
    g.rows1 = q;
  }
  if (g.rows2) {
    float* q = nullptr;
    if (hipMalloc(&q, c * d * 4) == hipSuccess) {
      if (g.rows2_valid && n) {
        DIF_HIP(hipMemcpyAsync(q, g.rows2, n * d * 4, hipMemcpyDeviceToDevice, st));
        DIF_HIP(hipStreamSynchronize(st));
      }
    } else {
      (void)hipGetLastError();
      g.rows2_valid = false;
    }
    DIF_HIP(hipFree(g.rows2));
    g.rows2 = q;
  }
  g.rows1_refused = g.rows2_refused = false;
  g.cap = capacity;
  return 0;
}

int dif_gallery_update(dif_gallery* h, const float* rows_dev, int64_t n, int64_t first_row, void* stream) {
  if (!h) return set_error("dif_gallery_update: null handle");
  if (n < 0 || first_row < 0) return set_error("dif_gallery_update: negative row count or position");
  if (n > 0 && !rows_dev) return set_error("dif_gallery_update: null rows");
  Gallery& g = h->g;
  if (first_row > g.n)
    return set_error("dif_gallery_update: first_row %lld would leave a gap behind the gallery's %lld rows", (long long)first_row,
                     (long long)g.n);
  if (first_row + n > g.cap)
    return set_error("dif_gallery_update: rows [%lld, %lld) exceed the capacity of %lld rows (dif_gallery_reserve grows it)",
                     (long long)first_row, (long long)(first_row + n), (long long)g.cap);
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t old_n = g.n;
  if (first_row + n > g.n) g.n = first_row + n;
  return gallery_update_rows(&g, rows_dev, first_row, n, old_n, st);
}

int dif_gallery_remove(dif_gallery* h, const int64_t* rows_dev, int64_t k, int64_t* moved_from_dev, int64_t* moved_to_dev,
                       int64_t* n_moved_out, void* stream) {
  if (!h) return set_error("dif_gallery_remove: null handle");
  if (k < 0) return set_error("dif_gallery_remove: negative row count");
  if (n_moved_out) *n_moved_out = 0;
  if (k == 0) return 0;
  if (!rows_dev) return set_error("dif_gallery_remove: null rows");
  Gallery& g = h->g;
  if (k > g.n)
    return set_error("dif_gallery_remove: %lld rows named, the gallery holds %lld (the list must be distinct)", (long long)k,
                     (long long)g.n);
  return gallery_remove_rows(&g, rows_dev, k, moved_from_dev, moved_to_dev, n_moved_out, (hipStream_t)stream);
}

int64_t dif_gallery_size(const dif_gallery* h) { return h ? h->g.n : 0; }
int64_t dif_gallery_capacity(const dif_gallery* h) { return h ? h->g.cap : 0; }

static const char* const kGalleryOptions[] = {"filter", "frag", "clamp_nan", "bd", "bd_fill", "topk_seed", "cluster_round", "roc_round", "roc_blocks", "within_round", "topk_round", nullptr};

const char* dif_gallery_option_name(int i) {
  int n = 0;
  while (kGalleryOptions[n]) ++n;
  return i >= 0 && i < n ? kGalleryOptions[i] : nullptr;
}

int dif_gallery_set_option(dif_gallery* h, const char* key, int value) {
  if (!h || !key) return set_error("dif_gallery_set_option: null argument");
  {
    bool known = false;
    for (const char* const* t = kGalleryOptions; *t; ++t) known |= std::string(*t) == key;
    if (!known) return set_error("dif_gallery_set_option: unknown key '%s'", key);
  }
  if (std::string(key) == "clamp_nan") {
    h->g.clamp_nan = value != 0;
    return 0;
  }
  if (std::string(key) == "topk_seed") {
    // tiles the seed stage of dif_match_topk evaluates per probe (0: k of them).  Same answers: the sweep completes the list
    if (value < 0) return set_error("dif_gallery_set_option: 'topk_seed' takes 0 or a positive tile count");
    h->g.topk_seed = value;
    return 0;
  }
  if (std::string(key) == "cluster_round") {
    // probes per round of dif_gallery_cluster and dif_gallery_dbscan (0: a sixteenth of the rows, at least 2048).  Same answers: tests force several rounds
    if (value < 0 || value % 128 != 0) return set_error("dif_gallery_set_option: 'cluster_round' takes 0 or a multiple of 128");
    h->g.cluster_round = value;
    return 0;
  }
  if (std::string(key) == "roc_round") {
    // probes per round of dif_match_roc (0: what the mask workspace's cap allows).  Same answers: tests force several rounds
    if (value < 0 || value % 128 != 0) return set_error("dif_gallery_set_option: 'roc_round' takes 0 or a multiple of 128");
    h->g.roc_round = value;
    return 0;
  }
  if (std::string(key) == "within_round") {
    // probes per round of dif_match_within, dif_match_rank and dif_match_rank_at (0: what the census' cap allows).  Same answers: tests force several rounds
    if (value < 0 || value % 128 != 0) return set_error("dif_gallery_set_option: 'within_round' takes 0 or a multiple of 128");
    h->g.within_round = value;
    return 0;
  }
  if (std::string(key) == "topk_round") {
    // probes per round of dif_match_topk, dif_match_topk_ids and their tagged forms (0: what the tile words' cap allows).  Same answers: tests force several rounds
    if (value < 0 || value % 128 != 0) return set_error("dif_gallery_set_option: 'topk_round' takes 0 or a multiple of 128");
    h->g.topk_round = value;
    return 0;
  }
  if (std::string(key) == "roc_blocks") {
    // most blocks the resolve stage of dif_match_roc launches (0: 2048).  Same answers: tests make a block take several trips
    if (value < 0 || value > 65536) return set_error("dif_gallery_set_option: 'roc_blocks' takes 0 .. 65536");
    h->g.roc_blocks = value;
    return 0;
  }
  if (std::string(key) == "bd_fill") {
    if (value < 1 || value > 16) return set_error("dif_gallery_set_option: 'bd_fill' takes 1..16");
    h->g.bd_fill = value;
    return 0;
  }
  if (std::string(key) == "bd") {
    h->g.no_bd = value == 0;
    return 0;
  }
  if (std::string(key) == "frag") {
    // the one-term filter's copy in MFMA-fragment order (match_g1_kernel) or row-major (match_b1_kernel): same answers.
    // The copy is rewritten in the other layout by the next dif_match (or dif_gallery_set).
    if (value < 0 || value > 2) return set_error("dif_gallery_set_option: 'frag' takes 0, 1 or 2");
    h->g.frag = value;
    return 0;
  }
  if (std::string(key) == "filter") {
    // 0: f32 MFMA on the rows themselves; 1: two-term split-bf16 copy; 2: one-term bf16 copy (a wider net, re-ranked)
    if (value < 0 || value > 2) return set_error("dif_gallery_set_option: 'filter' takes 0, 1 or 2");
    Gallery& g = h->g;
    g.filter_bf2 = value != 0;
    g.filter_one = value == 2;
    const bool drop2 = g.rows2 && value != 1, drop1 = g.rows1 && value != 2;
    if (drop1 || drop2) {                      // give back the copy the chosen filter does not read
      DIF_HIP(hipDeviceSynchronize());         // a dif_match in flight may still read it
      if (drop2) {
        DIF_HIP(hipFree(g.rows2));
        g.rows2 = nullptr;
        g.rows2_valid = false;
      }
      if (drop1) {
        DIF_HIP(hipFree(g.rows1));
        g.rows1 = nullptr;
        g.rows1_valid = false;
      }
    }
    if (value) g.rows2_refused = g.rows1_refused = false;   // switched (back) on: the next dif_gallery_set / dif_match builds the copy
    return 0;
  }
  return set_error("dif_gallery_set_option: unknown key '%s'", key);
}

int dif_gallery_get_stat(dif_gallery* h, const char* key, int64_t* out, void* stream) {
  if (!h || !key || !out) return set_error("dif_gallery_get_stat: null argument");
  Gallery& g = h->g;
  const std::string k(key);
  if (k == "split_copy") {
    *out = ((g.rows2 && g.rows2_valid) || (g.rows1 && g.rows1_valid)) ? 1 : 0;
    return 0;
  }
  if (k == "filter_terms") {                   // what the next dif_match's filter stage runs on: 0 f32 rows, 2 / 1 bf16 terms per operand
    *out = (g.filter_bf2 && g.filter_one && g.rows1 && g.rows1_valid) ? 1 : ((g.filter_bf2 && g.rows2 && g.rows2_valid) ? 2 : 0);
    return 0;
  }
  if (k == "frag_copy") {                      // 1: the one-term copy is held in fragment order (the next dif_match runs match_g1_kernel)
    *out = (g.filter_bf2 && g.filter_one && g.rows1 && g.rows1_valid && g.rows1_frag) ? 1 : 0;
    return 0;
  }
  if (k == "row_bytes") {                      // device bytes held per gallery row
    *out = (int64_t)g.d * 4 * (g.rows2 ? 2 : 1) + (g.rows1 ? (int64_t)g.d * 2 : 0) + 8;
    return 0;
  }
  if (k == "exact_probes") {                   // probes the last dif_match sent to the exact whole-gallery search
    int v = 0;
    if (g.nflag) {
      DIF_HIP(hipMemcpyAsync(&v, g.nflag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
      DIF_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    *out = v;
    return 0;
  }
  if (k == "roc_resolved") {                   // pairs the last dif_match_roc evaluated one by one (too close to a threshold to call)
    unsigned long long v = 0;
    if (g.roc_bins) {
      DIF_HIP(hipMemcpyAsync(&v, g.roc_bins + 2 * (DIF_ROC_MAX_THRESHOLDS + 2), sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
      DIF_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    *out = (int64_t)v;
    return 0;
  }
  if (k == "topk_ids_tiles") {                 // (probe, tile) pairs the last dif_match_topk_ids evaluated row by row
    unsigned long long v = 0;
    if (g.topk_ids_stat) {
      DIF_HIP(hipMemcpyAsync(&v, g.topk_ids_stat, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
      DIF_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    *out = (int64_t)v;
    return 0;
  }
  if (k == "topk_tagged_tiles") {              // (probe, tile) pairs the last tagged top-k call evaluated row by row
    unsigned long long v = 0;
    if (g.topk_tagged_stat) {
      DIF_HIP(hipMemcpyAsync(&v, g.topk_tagged_stat, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
      DIF_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    *out = (int64_t)v;
    return 0;
  }
  if (k == "within_tagged_tiles") {            // (probe, tile) pairs the last tagged within / rank / rank_at call evaluated row by row
    unsigned long long v = 0;
    if (g.within_tagged_stat) {
      DIF_HIP(hipMemcpyAsync(&v, g.within_tagged_stat, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
      DIF_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    *out = (int64_t)v;
    return 0;
  }
  return set_error("dif_gallery_get_stat: unknown key '%s'", key);
}

int dif_match(dif_gallery* h, const float* probes_dev, int n, int metric, int64_t* idx_out_dev,
              float* dist_out_dev, float* key_out_dev, void* stream) {
  if (!h) return set_error("dif_match: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match: negative probe count");
  if (n == 0) return 0;
  if (!probes_dev || !idx_out_dev || !dist_out_dev) return set_error("dif_match: null pointer");
  return match_run(&h->g, probes_dev, n, metric, idx_out_dev, dist_out_dev, key_out_dev, (hipStream_t)stream);
}

int dif_match_within(dif_gallery* h, const float* probes_dev, int n, int metric, float tolerance, int max_hits,
                     int64_t* count_out_dev, int64_t* idx_out_dev, float* dist_out_dev, void* stream) {
  if (!h) return set_error("dif_match_within: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_within: negative probe count");
  if (max_hits < 0 || max_hits > DIF_WITHIN_MAX_HITS)
    return set_error("dif_match_within: max_hits %d outside [0, %d]", max_hits, DIF_WITHIN_MAX_HITS);
  if (tolerance != tolerance) return set_error("dif_match_within: the tolerance is NaN");
  if (n == 0) return 0;
  if (!probes_dev || !count_out_dev) return set_error("dif_match_within: null pointer");
  if (max_hits > 0 && (!idx_out_dev || !dist_out_dev)) return set_error("dif_match_within: null list pointer with max_hits > 0");
  return within_run(&h->g, probes_dev, n, metric, tolerance, max_hits, count_out_dev, idx_out_dev, dist_out_dev,
                    (hipStream_t)stream);
}

int dif_match_rank(dif_gallery* h, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev,
                   int64_t* rank_out_dev, float* mate_dist_out_dev, void* stream) {
  if (!h) return set_error("dif_match_rank: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_rank: negative probe count");
  if (n == 0) return 0;
  if (!probes_dev || !mate_idx_dev || !rank_out_dev) return set_error("dif_match_rank: null pointer");
  return rank_run(&h->g, probes_dev, n, metric, mate_idx_dev, nullptr, rank_out_dev, mate_dist_out_dev, (hipStream_t)stream);
}

int dif_match_mate_dist(dif_gallery* h, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev,
                        float* mate_dist_out_dev, int64_t* owned_out_dev, void* stream) {
  if (!h) return set_error("dif_match_mate_dist: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_mate_dist: negative probe count");
  if (n == 0) return 0;
  if (!probes_dev || !mate_idx_dev || !mate_dist_out_dev || !owned_out_dev) return set_error("dif_match_mate_dist: null pointer");
  return mate_dist_run(&h->g, probes_dev, n, metric, mate_idx_dev, mate_dist_out_dev, owned_out_dev, (hipStream_t)stream);
}

int dif_match_rank_at(dif_gallery* h, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev,
                      const float* mate_dist_in_dev, int64_t* count_out_dev, void* stream) {
  if (!h) return set_error("dif_match_rank_at: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_rank_at: negative probe count");
  if (n == 0) return 0;
  if (!probes_dev || !mate_idx_dev || !mate_dist_in_dev || !count_out_dev) return set_error("dif_match_rank_at: null pointer");
  return rank_run(&h->g, probes_dev, n, metric, mate_idx_dev, mate_dist_in_dev, count_out_dev, nullptr, (hipStream_t)stream);
}

// The tagged range search and rank: with rows enrolled both arrays are needed; an empty gallery reads neither (the run
// functions are handed a null pair: their untagged path, which evaluates no tile) and the counter reads 0 all the same.
static int tagged_pair(const char* fn, dif_gallery* h, const int64_t*& row_tags_dev, const int64_t*& probe_masks_dev, void* stream) {
  if (h->g.n > 0) {
    if (!row_tags_dev || !probe_masks_dev) return set_error("%s: null row tags or probe masks", fn);
    return 0;
  }
  row_tags_dev = probe_masks_dev = nullptr;
  if (h->g.within_tagged_stat) DIF_HIP(hipMemsetAsync(h->g.within_tagged_stat, 0, sizeof(unsigned long long), (hipStream_t)stream));
  return 0;
}

int dif_match_within_tagged(dif_gallery* h, const float* probes_dev, int n, int metric, float tolerance, int max_hits,
                            const int64_t* row_tags_dev, const int64_t* probe_masks_dev, int64_t* count_out_dev,
                            int64_t* idx_out_dev, float* dist_out_dev, void* stream) {
  if (!h) return set_error("dif_match_within_tagged: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_within_tagged: negative probe count");
  if (max_hits < 0 || max_hits > DIF_WITHIN_MAX_HITS)
    return set_error("dif_match_within_tagged: max_hits %d outside [0, %d]", max_hits, DIF_WITHIN_MAX_HITS);
  if (tolerance != tolerance) return set_error("dif_match_within_tagged: the tolerance is NaN");
  if (n == 0) return 0;
  if (!probes_dev || !count_out_dev) return set_error("dif_match_within_tagged: null pointer");
  if (max_hits > 0 && (!idx_out_dev || !dist_out_dev))
    return set_error("dif_match_within_tagged: null list pointer with max_hits > 0");
  if (tagged_pair("dif_match_within_tagged", h, row_tags_dev, probe_masks_dev, stream)) return -1;
  return within_run(&h->g, probes_dev, n, metric, tolerance, max_hits, count_out_dev, idx_out_dev, dist_out_dev,
                    (hipStream_t)stream, row_tags_dev, probe_masks_dev);
}

int dif_match_rank_tagged(dif_gallery* h, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev,
                          const int64_t* row_tags_dev, const int64_t* probe_masks_dev, int64_t* rank_out_dev,
                          float* mate_dist_out_dev, void* stream) {
  if (!h) return set_error("dif_match_rank_tagged: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_rank_tagged: negative probe count");
  if (n == 0) return 0;
  if (!probes_dev || !mate_idx_dev || !rank_out_dev) return set_error("dif_match_rank_tagged: null pointer");
  if (tagged_pair("dif_match_rank_tagged", h, row_tags_dev, probe_masks_dev, stream)) return -1;
  return rank_run(&h->g, probes_dev, n, metric, mate_idx_dev, nullptr, rank_out_dev, mate_dist_out_dev, (hipStream_t)stream,
                  row_tags_dev, probe_masks_dev);
}

int dif_match_mate_dist_tagged(dif_gallery* h, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev,
                               const int64_t* row_tags_dev, const int64_t* probe_masks_dev, float* mate_dist_out_dev,
                               int64_t* owned_out_dev, void* stream) {
  if (!h) return set_error("dif_match_mate_dist_tagged: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_mate_dist_tagged: negative probe count");
  if (n == 0) return 0;
  if (!probes_dev || !mate_idx_dev || !mate_dist_out_dev || !owned_out_dev)
    return set_error("dif_match_mate_dist_tagged: null pointer");
  if (h->g.n > 0 && (!row_tags_dev || !probe_masks_dev)) return set_error("dif_match_mate_dist_tagged: null row tags or probe masks");
  if (h->g.n == 0) row_tags_dev = probe_masks_dev = nullptr;   // nothing owned: neither array is read
  return mate_dist_run(&h->g, probes_dev, n, metric, mate_idx_dev, mate_dist_out_dev, owned_out_dev, (hipStream_t)stream,
                       row_tags_dev, probe_masks_dev);
}

int dif_match_rank_at_tagged(dif_gallery* h, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev,
                             const float* mate_dist_in_dev, const int64_t* row_tags_dev, const int64_t* probe_masks_dev,
                             int64_t* count_out_dev, void* stream) {
  if (!h) return set_error("dif_match_rank_at_tagged: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_rank_at_tagged: negative probe count");
  if (n == 0) return 0;
  if (!probes_dev || !mate_idx_dev || !mate_dist_in_dev || !count_out_dev) return set_error("dif_match_rank_at_tagged: null pointer");
  if (tagged_pair("dif_match_rank_at_tagged", h, row_tags_dev, probe_masks_dev, stream)) return -1;
  return rank_run(&h->g, probes_dev, n, metric, mate_idx_dev, mate_dist_in_dev, count_out_dev, nullptr, (hipStream_t)stream,
                  row_tags_dev, probe_masks_dev);
}

int dif_match_topk(dif_gallery* h, const float* probes_dev, int n, int metric, int k, int64_t* idx_out_dev,
                   float* dist_out_dev, void* stream) {
  if (!h) return set_error("dif_match_topk: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_topk: negative probe count");
  if (k < 1 || k > DIF_TOPK_MAX) return set_error("dif_match_topk: k %d outside [1, %d]", k, DIF_TOPK_MAX);
  if (n == 0) return 0;
  if (!probes_dev || !idx_out_dev || !dist_out_dev) return set_error("dif_match_topk: null pointer");
  return topk_run(&h->g, probes_dev, n, metric, k, idx_out_dev, dist_out_dev, (hipStream_t)stream);
}

int dif_match_topk_ids(dif_gallery* h, const float* probes_dev, int n, int metric, int k, const int64_t* row_labels_dev,
                       const int64_t* exclude_dev, int64_t* idx_out_dev, float* dist_out_dev, int64_t* label_out_dev,
                       void* stream) {
  if (!h) return set_error("dif_match_topk_ids: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_topk_ids: negative probe count");
  if (k < 1 || k > DIF_TOPK_MAX) return set_error("dif_match_topk_ids: k %d outside [1, %d]", k, DIF_TOPK_MAX);
  if (n == 0) return 0;
  if (!probes_dev || !idx_out_dev || !dist_out_dev) return set_error("dif_match_topk_ids: null pointer");
  if (h->g.n > 0 && !row_labels_dev) return set_error("dif_match_topk_ids: null row labels");
  return topk_ids_run(&h->g, probes_dev, n, metric, k, row_labels_dev, exclude_dev, idx_out_dev, dist_out_dev, label_out_dev,
                      (hipStream_t)stream);
}

int dif_match_topk_tagged(dif_gallery* h, const float* probes_dev, int n, int metric, int k, const int64_t* row_tags_dev,
                          const int64_t* probe_masks_dev, int64_t* idx_out_dev, float* dist_out_dev, void* stream) {
  if (!h) return set_error("dif_match_topk_tagged: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_topk_tagged: negative probe count");
  if (k < 1 || k > DIF_TOPK_MAX) return set_error("dif_match_topk_tagged: k %d outside [1, %d]", k, DIF_TOPK_MAX);
  if (n == 0) return 0;
  if (!probes_dev || !idx_out_dev || !dist_out_dev) return set_error("dif_match_topk_tagged: null pointer");
  if (h->g.n > 0 && (!row_tags_dev || !probe_masks_dev)) return set_error("dif_match_topk_tagged: null row tags or probe masks");
  if (h->g.n == 0) {                            // nothing enrolled: all padding, no tag is read, no tile evaluated
    if (h->g.topk_tagged_stat) DIF_HIP(hipMemsetAsync(h->g.topk_tagged_stat, 0, sizeof(unsigned long long), (hipStream_t)stream));
    return topk_run(&h->g, probes_dev, n, metric, k, idx_out_dev, dist_out_dev, (hipStream_t)stream);
  }
  return topk_run(&h->g, probes_dev, n, metric, k, idx_out_dev, dist_out_dev, (hipStream_t)stream, row_tags_dev,
                  probe_masks_dev);
}

int dif_match_topk_ids_tagged(dif_gallery* h, const float* probes_dev, int n, int metric, int k, const int64_t* row_labels_dev,
                              const int64_t* exclude_dev, const int64_t* row_tags_dev, const int64_t* probe_masks_dev,
                              int64_t* idx_out_dev, float* dist_out_dev, int64_t* label_out_dev, void* stream) {
  if (!h) return set_error("dif_match_topk_ids_tagged: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_topk_ids_tagged: negative probe count");
  if (k < 1 || k > DIF_TOPK_MAX) return set_error("dif_match_topk_ids_tagged: k %d outside [1, %d]", k, DIF_TOPK_MAX);
  if (n == 0) return 0;
  if (!probes_dev || !idx_out_dev || !dist_out_dev) return set_error("dif_match_topk_ids_tagged: null pointer");
  if (h->g.n > 0 && !row_labels_dev) return set_error("dif_match_topk_ids_tagged: null row labels");
  if (h->g.n > 0 && (!row_tags_dev || !probe_masks_dev))
    return set_error("dif_match_topk_ids_tagged: null row tags or probe masks");
  if (h->g.n == 0) {                            // nothing enrolled: all padding, no label or tag is read, no tile evaluated
    if (h->g.topk_tagged_stat) DIF_HIP(hipMemsetAsync(h->g.topk_tagged_stat, 0, sizeof(unsigned long long), (hipStream_t)stream));
    return topk_ids_run(&h->g, probes_dev, n, metric, k, row_labels_dev, exclude_dev, idx_out_dev, dist_out_dev, label_out_dev,
                        (hipStream_t)stream);
  }
  return topk_ids_run(&h->g, probes_dev, n, metric, k, row_labels_dev, exclude_dev, idx_out_dev, dist_out_dev, label_out_dev,
                      (hipStream_t)stream, row_tags_dev, probe_masks_dev);
}

int dif_gallery_cluster(dif_gallery* h, int metric, float tolerance, int64_t first_row, const int64_t* labels_in_dev,
                        int64_t* labels_out_dev, int64_t* n_clusters_dev, void* stream) {
  if (!h) return set_error("dif_gallery_cluster: null handle");
  if (check_metric(metric)) return -1;
  if (tolerance != tolerance) return set_error("dif_gallery_cluster: the tolerance is NaN");
  const Gallery& g = h->g;
  if (g.d % 32 != 0) return set_error("dif_gallery_cluster: embedding size must be a multiple of 32 (got %d)", g.d);
  if (first_row < 0 || first_row > g.n)
    return set_error("dif_gallery_cluster: first_row %lld outside [0, %lld]", (long long)first_row, (long long)g.n);
  if (first_row > 0 && !labels_in_dev) return set_error("dif_gallery_cluster: first_row > 0 needs the earlier labels");
  if (!n_clusters_dev || (g.n > 0 && !labels_out_dev)) return set_error("dif_gallery_cluster: null pointer");
  if (g.n >= 0x7fffffffLL) return set_error("dif_gallery_cluster: at most 2^31-1 rows");
  return cluster_run(&h->g, metric, tolerance, first_row, labels_in_dev, labels_out_dev, n_clusters_dev, (hipStream_t)stream);
}

int dif_gallery_dbscan(dif_gallery* h, int metric, float tolerance, int min_samples, int64_t* labels_out_dev,
                       int32_t* degree_out_dev, int64_t* counts_dev, void* stream) {
  if (!h) return set_error("dif_gallery_dbscan: null handle");
  if (check_metric(metric)) return -1;
  if (tolerance != tolerance) return set_error("dif_gallery_dbscan: the tolerance is NaN");
  if (min_samples < 1) return set_error("dif_gallery_dbscan: min_samples must be at least 1 (got %d)", min_samples);
  const Gallery& g = h->g;
  if (g.d % 32 != 0) return set_error("dif_gallery_dbscan: embedding size must be a multiple of 32 (got %d)", g.d);
  if (!counts_dev || (g.n > 0 && !labels_out_dev)) return set_error("dif_gallery_dbscan: null pointer");
  if (g.n >= 0x7fffffffLL) return set_error("dif_gallery_dbscan: at most 2^31-1 rows");
  return dbscan_run(&h->g, metric, tolerance, min_samples, labels_out_dev, degree_out_dev, counts_dev, (hipStream_t)stream);
}

int dif_match_roc(dif_gallery* h, const float* probes_dev, int n, int metric, const int64_t* probe_labels_dev,
                  const int64_t* row_labels_dev, const int64_t* first_row_dev, const float* thresholds_dev, int n_thresholds,
                  int64_t* accept_out_dev, int64_t* totals_out_dev, void* stream) {
  if (!h) return set_error("dif_match_roc: null handle");
  if (check_metric(metric)) return -1;
  if (n < 0) return set_error("dif_match_roc: negative probe count");
  if (n_thresholds < 1 || n_thresholds > DIF_ROC_MAX_THRESHOLDS)
    return set_error("dif_match_roc: n_thresholds %d outside [1, %d]", n_thresholds, DIF_ROC_MAX_THRESHOLDS);
  if (!thresholds_dev || !accept_out_dev || !totals_out_dev) return set_error("dif_match_roc: null pointer");
  const Gallery& g = h->g;
  if (n > 0 && (!probes_dev || !probe_labels_dev)) return set_error("dif_match_roc: null probes or probe labels");
  if (n > 0 && g.n > 0 && !row_labels_dev) return set_error("dif_match_roc: null row labels");
  // the one host read of the call, of an INPUT: the thresholds (at most 4 KB) are checked before anything is launched
  float thr[DIF_ROC_MAX_THRESHOLDS];
  hipStream_t st = (hipStream_t)stream;
  DIF_HIP(hipMemcpyAsync(thr, thresholds_dev, (size_t)n_thresholds * sizeof(float), hipMemcpyDeviceToHost, st));
  DIF_HIP(hipStreamSynchronize(st));
  for (int j = 0; j < n_thresholds; ++j) {
    if (thr[j] != thr[j]) return set_error("dif_match_roc: threshold %d is NaN", j);
    if (j > 0 && thr[j] < thr[j - 1])
      return set_error("dif_match_roc: the thresholds must be non-decreasing (%d: %g after %g)", j, (double)thr[j], (double)thr[j - 1]);
  }
  return roc_run(&h->g, probes_dev, n, metric, probe_labels_dev, row_labels_dev, first_row_dev, thresholds_dev, n_thresholds,
                 accept_out_dev, totals_out_dev, st);
}

int dif_match_merge(const float* keys_dev, const int64_t* idx_dev, const float* dist_dev, int R, int n,
                    int64_t* idx_out_dev, float* dist_out_dev, void* stream) {
  if (R <= 0 || n < 0) return set_error("dif_match_merge: bad sizes R=%d n=%d", R, n);
  if (n == 0) return 0;
  if (!keys_dev || !idx_dev || !dist_dev || !idx_out_dev || !dist_out_dev)
    return set_error("dif_match_merge: null pointer");
  return match_merge_run(keys_dev, (int64_t)n * 4, idx_dev, (int64_t)n * 8, dist_dev, (int64_t)n * 4, R, n, idx_out_dev,
                         dist_out_dev, (hipStream_t)stream);
}

int dif_match_merge_packed(const void* packed_dev, int R, int n, int64_t* idx_out_dev, float* dist_out_dev,
                           void* stream) {
  if (R <= 0 || n < 0) return set_error("dif_match_merge_packed: bad sizes R=%d n=%d", R, n);
  if (n == 0) return 0;
  if (!packed_dev || !idx_out_dev || !dist_out_dev) return set_error("dif_match_merge_packed: null pointer");
  const char* base = static_cast<const char*>(packed_dev);
  const int64_t pitch = (int64_t)n * 16;     // per rank: key[n] f32 | dist[n] f32 | idx[n] i64
  return match_merge_run(base, pitch, base + (size_t)n * 8, pitch, base + (size_t)n * 4, pitch, R, n, idx_out_dev,
                         dist_out_dev, (hipStream_t)stream);
}

static int check_shards(const char* fn, int R, int n) {
  if (R < 1 || R > DIF_SHARD_MAX) return set_error("%s: R %d outside [1, %d]", fn, R, DIF_SHARD_MAX);
  if (n < 0) return set_error("%s: negative probe count", fn);
  return 0;
}

int dif_shard_merge_topk(const int64_t* idx_dev, const float* dist_dev, int R, int n, int k, int64_t* idx_out_dev,
                         float* dist_out_dev, void* stream) {
  if (check_shards("dif_shard_merge_topk", R, n)) return -1;
  if (k < 1 || k > DIF_TOPK_MAX) return set_error("dif_shard_merge_topk: k %d outside [1, %d]", k, DIF_TOPK_MAX);
  if (n == 0) return 0;
  if (!idx_dev || !dist_dev || !idx_out_dev || !dist_out_dev) return set_error("dif_shard_merge_topk: null pointer");
  return shard_merge_lists_run(true, nullptr, idx_dev, dist_dev, R, n, k, nullptr, idx_out_dev, dist_out_dev, (hipStream_t)stream);
}

int dif_shard_merge_topk_ids(const int64_t* idx_dev, const float* dist_dev, const int64_t* label_dev, int R, int n, int k,
                             int64_t* idx_out_dev, float* dist_out_dev, int64_t* label_out_dev, void* stream) {
  if (check_shards("dif_shard_merge_topk_ids", R, n)) return -1;
  if (k < 1 || k > DIF_TOPK_MAX) return set_error("dif_shard_merge_topk_ids: k %d outside [1, %d]", k, DIF_TOPK_MAX);
  if (n == 0) return 0;
  if (!idx_dev || !dist_dev || !label_dev || !idx_out_dev || !dist_out_dev) return set_error("dif_shard_merge_topk_ids: null pointer");
  return shard_merge_ids_run(idx_dev, dist_dev, label_dev, R, n, k, idx_out_dev, dist_out_dev, label_out_dev, (hipStream_t)stream);
}

int dif_shard_merge_within(const int64_t* count_dev, const int64_t* idx_dev, const float* dist_dev, int R, int n, int max_hits,
                           int64_t* count_out_dev, int64_t* idx_out_dev, float* dist_out_dev, void* stream) {
  if (check_shards("dif_shard_merge_within", R, n)) return -1;
  if (max_hits < 0 || max_hits > DIF_WITHIN_MAX_HITS)
    return set_error("dif_shard_merge_within: max_hits %d outside [0, %d]", max_hits, DIF_WITHIN_MAX_HITS);
  if (n == 0) return 0;
  if (!count_dev || !count_out_dev) return set_error("dif_shard_merge_within: null pointer");
  if (max_hits > 0 && (!idx_dev || !dist_dev || !idx_out_dev || !dist_out_dev))
    return set_error("dif_shard_merge_within: null list pointer with max_hits > 0");
  return shard_merge_lists_run(false, count_dev, idx_dev, dist_dev, R, n, max_hits, count_out_dev, idx_out_dev, dist_out_dev,
                               (hipStream_t)stream);
}

int dif_shard_merge_rank(const int64_t* count_dev, const int64_t* owned_dev, const float* mate_dist_dev, int R, int n,
                         int64_t* rank_out_dev, float* mate_dist_out_dev, void* stream) {
  if (check_shards("dif_shard_merge_rank", R, n)) return -1;
  if (n == 0) return 0;
  if (!count_dev || !owned_dev || !mate_dist_dev || !rank_out_dev) return set_error("dif_shard_merge_rank: null pointer");
  return shard_merge_rank_run(count_dev, owned_dev, mate_dist_dev, R, n, rank_out_dev, mate_dist_out_dev, (hipStream_t)stream);
}

}  // extern "C"
