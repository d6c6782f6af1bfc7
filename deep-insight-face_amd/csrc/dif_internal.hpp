// Internal declarations shared by the translation units of libdif.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

namespace dif {

int set_error(const char* fmt, ...);   // records the message for dif_last_error(), returns -1

#define DIF_HIP(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return ::dif::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// ---- gallery (owned copy of the rows + per-row norms + match workspace)
struct Gallery {
  int d = 0;
  int64_t n = 0;
  int64_t cap = 0;
  int64_t index_base = 0;   // global index of row 0 (gallery sharded across ranks)
  float* rows = nullptr;    // [n][d]
  float* rows2 = nullptr;   // the same rows as two bf16 planes per K-step of 32, [n][d/32][hi 32 | mid 32] (the filter's operand)
  uint16_t* rows1 = nullptr;// the same rows rounded to bf16 (the one-term filter's operand: "filter" = 2), capacity rounded up to 64 rows:
                            // [n][d] for match_b1_kernel, or -- rows1_frag -- in MFMA-fragment order for match_g1_kernel
  float* probes2 = nullptr; // this call's probes in the filter's form (probes2_cap rows of d floats)
  size_t probes2_cap = 0;
  float* sq = nullptr;      // |g|^2
  float* ninv = nullptr;    // -1/|g|
  // match workspace (csrc/match.hip): per (block, probe) minimum key, candidate count, candidate rows
  float* part_key = nullptr;
  int* part_cnt = nullptr;
  int* part_idx = nullptr;
  size_t part_cap = 0;
  // per probe: error bound of the search key, packed (key, index) winner, its distance, overflow list
  float* eps = nullptr;
  float* eps32 = nullptr;          // ... and of the f32 re-check the finish stage makes of the filter's candidates
  unsigned long long* best = nullptr;
  float* best_dist = nullptr;
  int* flagged = nullptr;
  size_t probe_cap = 0;
  float* hi = nullptr;             // per probe: key above which a row may be anti-parallel beyond -1 (metric 1)
  int* pcls = nullptr;             // per probe: 1 = |q|^2 outside the filter's range, classified by the finish stage
  int* anti_cnt = nullptr;         // per probe: rows whose key reached hi, and up to KANTI of their indices
  int* anti_idx = nullptr;
  int* nflag = nullptr;            // number of probes sent to the exact search in the current call
  unsigned* sqmax_bits = nullptr;  // bits of max |g|^2 over the rows the metric-0 filter sees
  struct GalleryFlags* flags = nullptr;   // rows the filter cannot rank (csrc/match.hip), found by gallery_norms
  bool rows2_valid = false;        // rows2 holds the split of the CURRENT rows
  bool rows2_refused = false;      // its allocation failed for this capacity: the f32 filter serves, no retry per call
  bool rows1_valid = false, rows1_refused = false;   // the same two states for rows1
  int frag = 1;                    // "frag": rows1 in fragment order -- 1 (default) where the embedding size allows it (match.hip: g1_dims) and the
                                   // gallery is large enough to give every wave of match_g1_kernel a few tiles, 2 whatever its size, 0 never
  bool rows1_frag = false;         // the layout rows1 was last filled in
  bool filter_one = true;          // "filter" = 2 (default): one bf16 term per operand (match_b1_kernel), a wider net re-ranked; 1: two terms
  bool filter_bf2 = true;          // the MFMA filter runs on bf16 operands (dif_gallery_set_option "filter" = 0: f32)
  int bd_fill = 1;                 // "bd_fill": blocks of match_bd_kernel per resident slot (development: no effect measured, r04)
  bool no_bd = false;              // dif_gallery_set_option "bd" = 0: the split-bf16 filter stays on match_tile_kernel for every batch
  bool clamp_nan = false;          // report distance 0 / 1 instead of the reference's NaN (dif_gallery_set_option)
  // range-search workspace (csrc/match_within.hip), apart from dif_match's; every buffer grows against a capacity of its own
  unsigned short* within_census = nullptr;   // [gallery tile][probe]: rows surely within the tolerance | borderline rows << 8
  size_t within_census_cap = 0;              // ... in 16-bit words
  float* within_thr = nullptr;               // per probe: {key <= [0]: sure, key > [1]: out, |key| >= [2]: borderline, [3] != 0: resolve all}
  size_t within_thr_cap = 0;                 // ... in probes
  int within_round = 0;                      // "within_round": probes per round of dif_match_within / _rank / _rank_at (0: what the census' cap allows)
  // the tagged forms (dif_match_within_tagged, _rank_tagged, _rank_at_tagged) add the counter of "within_tagged_tiles"
  unsigned long long* within_tagged_stat = nullptr;
  // dif_match_rank shares the two above (stream-ordered calls) and adds, per probe, the mate's distance and local row
  struct RankMate* rank_mate = nullptr;
  size_t rank_mate_cap = 0;                  // ... in probes
  // dif_match_topk's workspace, its own: per (gallery tile of 128 rows, probe) the minimum search key of the tile
  float* topk_min = nullptr;
  size_t topk_min_cap = 0;                   // ... in floats
  int topk_seed = 0;                         // "topk_seed": tiles the seed of dif_match_topk evaluates per probe (0: k of them)
  int topk_round = 0;                        // "topk_round": probes per round of the four top-k entries (0: what the tile words' cap allows)
  // dif_match_topk_ids shares topk_min (stream-ordered calls) and adds one counter: the (probe, tile) evaluations of the last call
  unsigned long long* topk_ids_stat = nullptr;
  // dif_match_topk_tagged / dif_match_topk_ids_tagged share topk_min too and add the counter of "topk_tagged_tiles"
  unsigned long long* topk_tagged_stat = nullptr;
  // dif_gallery_cluster (csrc/match_within.hip) shares the census and its thresholds (stream-ordered calls) and adds the
  // union-find's parent array, one int per row, and one int that tells cluster_flatten_kernel of a bad labels_in entry
  int* cluster_parent = nullptr;
  size_t cluster_parent_cap = 0;             // ... in rows
  int* cluster_bad = nullptr;
  int cluster_round = 0;                     // "cluster_round": probes per round of dif_gallery_cluster (0: a sixteenth of the rows, at least 2048)
  // dif_gallery_dbscan (csrc/match_within.hip) shares the census, its thresholds and cluster_parent (stream-ordered calls) and
  // adds, per row, the number of rows within the tolerance and the nearest core row; each grows against a capacity of its own
  int* dbscan_degree = nullptr;
  size_t dbscan_degree_cap = 0;              // ... in rows
  unsigned long long* dbscan_anchor = nullptr;   // float bits of the distance << 32 | core row, ~0: none
  size_t dbscan_anchor_cap = 0;              // ... in rows
  // dif_match_roc's workspace (csrc/match_roc.hip), its own; every buffer grows against a capacity of its own
  unsigned* roc_mask = nullptr;              // [gallery tile][probe][4]: the 128-bit mask of the borderline rows
  size_t roc_mask_cap = 0;                   // ... in masks of 16 bytes
  float* roc_thr = nullptr;                  // per probe: {scale of the key, half width of the band, |key| >= [2]: borderline, -}
  size_t roc_thr_cap = 0;                    // ... in probes
  float* roc_tab = nullptr;                  // the call's two search tables, 2048 floats each (allocated once)
  unsigned long long* roc_bins = nullptr;    // the call's bins, [DIF_ROC_MAX_THRESHOLDS + 2][2] (allocated once)
  int roc_blocks = 0;                        // "roc_blocks": most blocks of roc_resolve_kernel (0: 2048)
  int roc_round = 0;                         // "roc_round": probes per round of dif_match_roc (0: what the mask workspace's cap allows)
  // dif_gallery_remove's plan (csrc/match.hip): the record the host reads, then one destination per tail slot
  int64_t* remove_ws = nullptr;
  size_t remove_ws_cap = 0;                  // ... in 8-byte words
};

int gallery_norms(Gallery* g, const float* src, hipStream_t st);   // src: the caller's rows (copied into g->rows in the same pass), or null
int gallery_split_copy(Gallery* g, hipStream_t st);   // (re)builds rows2 when the option asks for it; never fatal
int gallery_update_rows(Gallery* g, const float* src, int64_t first, int64_t count, int64_t old_n, hipStream_t st);   // rows [first, first+count) <- src
int gallery_remove_rows(Gallery* g, const int64_t* rows_dev, int64_t k, int64_t* moved_from, int64_t* moved_to, int64_t* n_moved,
                        hipStream_t st);   // swap-remove of the k rows listed (global indices, strictly ascending; k <= g->n)
int match_run(Gallery* g, const float* probes, int B, int metric, int64_t* idx_out, float* dist_out,
              float* key_out, hipStream_t st);
int within_run(Gallery* g, const float* probes, int B, int metric, float tolerance, int max_hits, int64_t* count_out,
               int64_t* idx_out, float* dist_out, hipStream_t st, const int64_t* row_tags = nullptr,
               const int64_t* probe_masks = nullptr);                                     // tags given: dif_match_within_tagged
int rank_run(Gallery* g, const float* probes, int B, int metric, const int64_t* mates, const float* dm_in, int64_t* rank_out,
             float* mate_dist_out, hipStream_t st, const int64_t* row_tags = nullptr,
             const int64_t* probe_masks = nullptr);   // dm_in null: dif_match_rank; else dif_match_rank_at (rank_out: the shard's count); tags given: the tagged forms
int mate_dist_run(Gallery* g, const float* probes, int B, int metric, const int64_t* mates, float* mate_dist_out,
                  int64_t* owned_out, hipStream_t st, const int64_t* row_tags = nullptr, const int64_t* probe_masks = nullptr);
int topk_run(Gallery* g, const float* probes, int B, int metric, int k, int64_t* idx_out, float* dist_out, hipStream_t st,
             const int64_t* row_tags = nullptr, const int64_t* probe_masks = nullptr);   // tags given: dif_match_topk_tagged
int topk_ids_run(Gallery* g, const float* probes, int B, int metric, int k, const int64_t* row_labels, const int64_t* exclude,
                 int64_t* idx_out, float* dist_out, int64_t* label_out, hipStream_t st, const int64_t* row_tags = nullptr,
                 const int64_t* probe_masks = nullptr);                                   // tags given: dif_match_topk_ids_tagged
int cluster_run(Gallery* g, int metric, float tolerance, int64_t first_row, const int64_t* labels_in, int64_t* labels_out,
                int64_t* n_clusters, hipStream_t st);
int dbscan_run(Gallery* g, int metric, float tolerance, int min_samples, int64_t* labels_out, int* degree_out, int64_t* counts,
               hipStream_t st);
int roc_run(Gallery* g, const float* probes, int B, int metric, const int64_t* probe_labels, const int64_t* row_labels,
            const int64_t* first_row, const float* thresholds, int nT, int64_t* accept_out, int64_t* totals_out, hipStream_t st);
int pairwise_run(const float* e1, int64_t n1, const float* e2, int64_t n2, int D, int metric, float* out,
                 hipStream_t st);
int match_merge_run(const void* keys, int64_t key_pitch, const void* idx, int64_t idx_pitch, const void* dist,
                    int64_t dist_pitch, int R, int B, int64_t* idx_out, float* dist_out, hipStream_t st);   // pitches in bytes

// csrc/radix_sort.hip: the stable LSD radix sort of (key, position) pairs on 8-bit digits, K = unsigned or unsigned long long.
// The plan of a sort whose skipped passes are known on the device alone:
struct RadixPlan {
  int active[8], src[8];   // per pass: does it run, and which of the two buffers holds its input
  int final_buf, pad;      // the buffer that holds the sorted pairs
};
constexpr int kRadixSortTile = 2048;         // keys per block and pass (radix_sort.hip: kSortThreads * kSortItems)
int radix_sort_tile();                       // ... for a caller that sizes its blocks at run time
size_t radix_sort_hist_bytes(int64_t m);     // the [256][blocks] histogram of a pass over m keys
// enqueues passes 0 .. passes - 1 over (k0, p0) / (k1, p1).  plan_dev null: every pass runs, pass b reads buffer b & 1
template <typename K>
int radix_sort_run(const RadixPlan* plan_dev, int passes, K* k0, K* k1, int* p0, int* p1, int64_t m, unsigned* hist, hipStream_t st);
int block_scan_run(unsigned* data, int64_t E, hipStream_t st);   // the sort's scan on its own: exclusive, in place, by one block

// One allocation shared out in steps of 256 bytes.  With a null base take() returns null and `at` still counts: the size.
struct Carver {
  char* base;
  size_t at = 0;
  explicit Carver(void* b) : base((char*)b) {}
  void* take(size_t bytes) {
    char* q = base ? base + at : nullptr;
    at += (bytes + 255) & ~(size_t)255;
    return q;
  }
};

// csrc/match_shard.hip: merges of R per-shard results laid out [R][n][...]
int shard_merge_lists_run(bool by_dist, const int64_t* count, const int64_t* idx, const float* dist, int R, int n, int L,
                          int64_t* count_out, int64_t* idx_out, float* dist_out, hipStream_t st);
int shard_merge_ids_run(const int64_t* idx, const float* dist, const int64_t* label, int R, int n, int k, int64_t* idx_out,
                        float* dist_out, int64_t* label_out, hipStream_t st);
int shard_merge_rank_run(const int64_t* count, const int64_t* owned, const float* mate_dist, int R, int n, int64_t* rank_out,
                         float* mate_dist_out, hipStream_t st);

}  // namespace dif
