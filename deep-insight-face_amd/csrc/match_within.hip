// Gallery range search: every enrolled row within a tolerance of each probe, exact (dif_match_within), the rank of
// one given row among all of them (dif_match_rank, and its shard-local halves dif_match_mate_dist / dif_match_rank_at for a
// mate the shard need not hold; the section starts at rank_prep_kernel), and the k nearest rows in order
// (dif_match_topk; its section, with the argument for its exactness, starts at topk_tilemin_kernel), the k nearest distinct
// identities over a label per row (dif_match_topk_ids; its section follows topk_run) -- both also over the rows each probe is
// eligible for (dif_match_topk_tagged, dif_match_topk_ids_tagged: the `Tagged` form of their three kernels; likewise the range search and
// the rank, dif_match_within_tagged / _rank_tagged / _mate_dist_tagged / _rank_at_tagged: WithinTags and TaggedCensusEpi) --, and the connected components
// of the gallery's own rows under a tolerance (dif_gallery_cluster; its section, with the union-find argument, starts at cl_find),
// and density clustering with noise on the same edges (dif_gallery_dbscan; its section starts at dbscan_init_kernel).
// hipcc-flags: -ffp-contract=off
// (the resolve stage restates the reference's float32 operations one by one, as match.hip's re-rank does)
//
// Semantics, per probe q (evaluation/utility.py:52-66 broadcast over the gallery rows, then three lines of NumPy):
//   dist = distance(q[None, :], gallery, metric);  hits = np.flatnonzero(dist <= t)      (NaN <= t is False)
//   count = len(hits);  idx = hits[:K] + index_base;  dist = dist[hits[:K]];  unused slots: idx -1, dist NaN
// The B x G distances are never materialised.  The tolerance is known before the first tile, so -- unlike the arg-min -- there
// is no running state: two stages, no atomics on global memory, no lists, no overflow path, deterministic by construction.
//
//  1. within_census_kernel -- key_tiles (key_tiles.hpp: match_tile_kernel<T, false>'s tiles, f32 MFMA main loop on the rows
//     themselves and XCD-aware block order) with the census policy: the search key of the epilogue
//        metric 1: key = -dot / |g|        metric 0: key = |g|^2 - 2 dot
//     is classified against two per-probe thresholds (within_prep_kernel):
//        SURE        key <= T - E  and |key| < H      the reference's distance is <= t whatever the rounding
//        OUT         key >  T + E                     ... is > t (or NaN) whatever the rounding
//        BORDERLINE  everything else, a NaN key included (rows kept out of the filter carry a NaN ingredient: zero-norm,
//                    tiny, huge and non-finite rows reach the reference arithmetic this way; GalleryFlags is not needed)
//     and stores, per (gallery tile of 128 rows, probe), one 16-bit word  sure | borderline << 8.  Every tile belongs to
//     exactly one block: nothing is accumulated in global memory.
//  2. within_resolve_kernel -- one block per probe walks that probe's words in ascending tile order.  A tile with a
//     borderline row, or with any sure row while the list still has room, is evaluated row by row with ref_distance
//     (match_ref.hpp: bit-identical to the reference for metric 0; metric 1 up to the arccos caveat of dif_match) and
//     `dist <= t` decides; its hits are counted and appended in row order.  Any other tile adds its sure count, no memory
//     touched.  A probe outside the bound's validity resolves every tile.
//
// The thresholds (u = 2^-24; E_key = match_ref.hpp's bound on |key - exact key| with c = D u for the f32 MFMA):
//   metric 1.  The reference's similarity s_ref = fl(dot / fl(|q| |g|)) -- float32 products, NumPy's pairwise sums (at most
//     25 roundings on a term's way into a sum of up to 8192 terms: 18 in its leaf of <= 128, 6 levels of the tree, 1 for the
//     product), two square roots, a product, a quotient -- lies within (25 + 2 (12.5 + 1) + 2) u = 54 u of the exact
//     s = q.g / (|q| |g|).  The reported distance fl(fl(acos(s_ref)) / fl(pi)) is a non-increasing function of s_ref with
//     at most 3 u of relative error, so `dist <= t` holds iff s_ref >= s* for an s* within pi 3 u < 10 u of cos(pi t).
//     T = -|q| cos(pi t) is formed in double from |q|^2 summed as an fma chain over 64 lanes (relative error of |q| below
//     (D / 128 + 4) u) and rounded once (u).  Hence  W1 = (96 + D / 64) u |q|  covers reference, arccos and T together, and
//        E = (c + 8 u) |q| + W1.
//     t >= 1: every distance that is not NaN is <= 1 <= t: T = +inf;  t < 0: no distance is: T = -inf.
//     A similarity within 54 u of +-1 may round beyond it and is NaN in the reference (not a hit; with "clamp_nan" 0 or 1 is
//     compared instead): a key with |key| >= H = |q| (1 - anti), anti = 2e-4 + 1.01 (c + 136 u) -- match.hip's net around
//     -1, widened by the key's own error and used on both sides -- is never SURE.  (OUT needs no such care: NaN is not a
//     hit, and a clamped distance of 1 is a hit only for t >= 1, where nothing is OUT.)
//   metric 0.  dist_ref = pairwise sum of fl(fl(q - g)^2): each term within 3 u, the sum within 25 u more:
//     |dist_ref - |q - g|^2| <= 28 u (|q| + |g|)^2.  T = t - |q|^2 with |q|^2 and the rows' |g|^2 each summed over 64 lanes
//     ((D / 64 + 8) u relative) and T rounded once:
//        E = u 18 gmax^2 + (2 c + 2 u) |q| gmax  +  32 u (|q| + gmax)^2 + (D / 64 + 8) u (|q|^2 + gmax^2) + u (|t| + |q|^2).
//   |q| enters as sqrt(sum) * 1.0001 as in probe_eps_one.  Deliberately generous: a wider E only costs resolved tiles.
//   Probes whose |q|^2 leaves [NORM_LO, NORM_HI] (metric 0: exceeds NORM_HI) or is not finite: every tile is resolved.
#include "key_tiles.hpp"

namespace dif {

constexpr size_t WITHIN_CENSUS_MAX = (size_t)128 << 20;   // census words per launch (256 MB); more probes go in several rounds

__global__ __launch_bounds__(256) void within_prep_kernel(const float* __restrict__ probes, int B, int D, int metric, float t,
                                                          float cdot, const unsigned* __restrict__ sqmax_bits,
                                                          f32x4* __restrict__ thr) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= B) return;
  const float s = probe_sq(probes + (int64_t)p * D, D, lane);
  if (lane != 0) return;
  const float inf = __builtin_inff();
  const Band b = within_band(metric, t, s, D, cdot, sqmax_bits);
  // (an infinite tolerance under metric 0 makes T - E a NaN: no key is SURE, none is OUT, every tile is resolved)
  thr[p] = b.odd ? f32x4{-inf, inf, b.H, 1.f} : f32x4{b.T - b.E, b.T + b.E, b.H, 0.f};
}

// ---------------------------------------------------------------------------------------------
// Rank of the mate (dif_match_rank): where does row m rank among all rows by distance to the probe?
//   dm = d[m];  rank = count(d < dm) + count(d[:m] == dm)            (NaN compares False: a NaN distance is never closer)
// Once dm is known this is the range search with the tolerance taken per probe and nothing listed:
//   rank_prep_kernel     dm on the reference arithmetic, and the census thresholds from it
//   within_census_kernel unchanged
//   rank_resolve_kernel  SURE counts of the tiles without a borderline row + the rows of the other tiles one by one
// SURE has to mean STRICTLY closer.  The bound of the header comment is not re-derived; it is used twice:
//   thr[0] = T(t') - E(t'),  t' = nextafterf(dm, -inf):  key <= thr[0] (and |key| < H)  =>  d <= t' < dm
//   thr[1] = T(dm) + E(dm):                              key >  thr[1]  =>  d > dm or NaN: neither closer nor tied
// thr[0] <= thr[1], which the census needs for bord = not out - sure: T is the rounding of a non-decreasing function of t
// (metric 1: -|q| cos(pi t) on [0, 1], -inf below 0, +inf from 1; cos in double is monotone up to 1e-16, far inside 2 E >=
// 192 u |q|; metric 0: the float subtraction t - |q|^2), E >= 0, and t' < dm.  Where E is not finite thr[0] is NaN or -inf
// and nothing is SURE.  dm = 0 gives t' < 0: T = -inf under metric 1, below every possible key minus E under metric 0 --
// nothing is closer than 0 and nothing is SURE.
struct RankMate {
  float dm;                                                   // the mate's distance (NaN: a miss at every rank)
  int row;                                                    // its local row, or -1: unmated
};

// Tagged (dif_match_within_tagged, dif_match_rank_tagged, dif_match_mate_dist_tagged, dif_match_rank_at_tagged): row r is
// eligible for probe p iff (row_tags[r] & probe_masks[p]) != 0 on the raw 64 bits, and every query is the untagged one with the
// distance of an ineligible row taken as NaN: never a hit, never closer, never a tie.  The tagged kernels below are the
// `Tagged` instantiations of the untagged ones and take one WithinTags by value through a parameter pack that is empty for
// Tagged = false, so the untagged kernels keep the argument lists -- and the code -- they had.
struct WithinTags {
  const int64_t* row_tags;                                    // [G]
  const int64_t* probe_masks;                                 // [B], this launch's probes
  unsigned long long* tiles_stat;                             // "within_tagged_tiles"
};
__device__ __forceinline__ const WithinTags& within_tags(const WithinTags& t) { return t; }

// Tagged: the mate's eligibility is tested first.  An ineligible mate has the distance NaN -- thresholds all OUT, nothing
// resolved, rank = G, "behind every row" -- and stays mated (RankMate.row >= 0), which tells it from an unmated probe (-1).
template <bool Tagged, class... TagArgs>
__global__ __launch_bounds__(256) void rank_prep_kernel(const float* __restrict__ probes, int B, int D, int metric, float cdot,
                                                        const unsigned* __restrict__ sqmax_bits,
                                                        const float* __restrict__ gallery, int64_t G, int64_t index_base,
                                                        const int64_t* __restrict__ mates, int clamp, const SumPlan plan,
                                                        f32x4* __restrict__ thr, RankMate* __restrict__ mate,
                                                        float* __restrict__ mate_dist_out,
                                                        const float* __restrict__ dm_in, const TagArgs... tagargs) {
  static_assert(sizeof...(TagArgs) == (Tagged ? 1 : 0), "one WithinTags exactly when Tagged");
  __shared__ float scratch[4][NP_SCRATCH];
  const int wave = threadIdx.x >> 6, p = blockIdx.x * 4 + wave, lane = threadIdx.x & 63;
  if (p >= B) return;                                         // (wave-uniform, like everything below)
  const float* q = probes + (int64_t)p * D;
  const int64_t m = mates[p];
  // (unsigned: one comparison covers both sides and cannot overflow, whatever the sign of index_base; a shard holds fewer
  // than 2^31 rows -- dif_gallery_set -- so the local row fits an int)
  const uint64_t ml = (uint64_t)m - (uint64_t)index_base;
  const bool mated = ml < (uint64_t)G;
  const float inf = __builtin_inff();
  float dm = __builtin_nanf("");
  // dif_match_rank_at (dm_in): the mate's distance is handed in -- the shard need not hold the mate -- and RankMate.row is
  // not used: rank_resolve_kernel<true> compares global rows with mates[p] itself
  bool elig = true;                                           // (dm_in: the owning shard has tested the mate)
  if constexpr (Tagged) {
    const WithinTags& tg = within_tags(tagargs...);
    if (!dm_in && mated) elig = ((unsigned long long)tg.row_tags[ml] & (unsigned long long)tg.probe_masks[p]) != 0;
  }
  if (dm_in) dm = dm_in[p];
  else if (mated && elig) (void)ref_distance(plan, scratch[wave], q, gallery + (int64_t)ml * D, metric, lane, &dm, clamp != 0);
  const float s = probe_sq(q, D, lane);
  if (lane != 0) return;
  mate[p] = RankMate{dm, dm_in ? 0 : (mated ? (int)ml : -1)};
  if (mate_dist_out) mate_dist_out[p] = dm;
  // unmated, or a NaN distance: every row OUT, nothing to resolve (the third word, H, only ever vetoes SURE, and with
  // thr[0] = -inf nothing is: its value does not matter here)
  if (!(dm == dm)) {
    thr[p] = f32x4{-inf, -inf, inf, 0.f};
    return;
  }
  const Band lo = within_band(metric, nextafterf(dm, -inf), s, D, cdot, sqmax_bits);
  const Band hi = within_band(metric, dm, s, D, cdot, sqmax_bits);
  thr[p] = hi.odd ? f32x4{-inf, inf, hi.H, 1.f} : f32x4{lo.T - lo.E, hi.T + hi.E, hi.H, 0.f};
}

// dif_match_mate_dist: the ref_distance part of rank_prep_kernel alone, a wave per probe -- the mate's distance where this
// shard holds the mate (owned 1), NaN and owned 0 where it does not.  No census, no gallery pass.
// Tagged: a mate this shard holds but the probe is not eligible for is owned (1) with the distance NaN.
template <bool Tagged, class... TagArgs>
__global__ __launch_bounds__(256) void mate_dist_kernel(const float* __restrict__ probes, int B, int D, int metric,
                                                        const float* __restrict__ gallery, int64_t G, int64_t index_base,
                                                        const int64_t* __restrict__ mates, int clamp, const SumPlan plan,
                                                        float* __restrict__ mate_dist_out, int64_t* __restrict__ owned_out,
                                                        const TagArgs... tagargs) {
  static_assert(sizeof...(TagArgs) == (Tagged ? 1 : 0), "one WithinTags exactly when Tagged");
  __shared__ float scratch[4][NP_SCRATCH];
  const int wave = threadIdx.x >> 6, p = blockIdx.x * 4 + wave, lane = threadIdx.x & 63;
  if (p >= B) return;                                         // (wave-uniform, like everything below)
  const uint64_t ml = (uint64_t)mates[p] - (uint64_t)index_base;   // (unsigned: as in rank_prep_kernel)
  const bool mated = ml < (uint64_t)G;
  float dm = __builtin_nanf("");
  bool elig = true;
  if constexpr (Tagged) {
    const WithinTags& tg = within_tags(tagargs...);
    if (mated) elig = ((unsigned long long)tg.row_tags[ml] & (unsigned long long)tg.probe_masks[p]) != 0;
  }
  if (mated && elig)
    (void)ref_distance(plan, scratch[wave], probes + (int64_t)p * D, gallery + (int64_t)ml * D, metric, lane, &dm, clamp != 0);
  if (lane != 0) return;
  mate_dist_out[p] = dm;
  owned_out[p] = mated ? 1 : 0;
}

// The census policy of key_tiles: two counts per probe column against the column's thresholds, a 16-bit word.  A NaN key is
// neither SURE nor OUT.  Rows past G are OUT (key +inf; where T + E is +inf as well they count as borderline, and the resolve
// stage, which stops at G, finds nothing in them).
struct CensusEpi : KeyEpi {
  const f32x4* __restrict__ thr;
  unsigned short* __restrict__ census;
  using Meet = int;                                           // sure | not out << 16
  struct Col {
    float ts, tm, hk;
  };
  struct State {
    int sure, nout;
  };
  __device__ __forceinline__ CensusEpi(const f32x4* thr_, unsigned short* census_) : thr(thr_), census(census_) {}
  __device__ __forceinline__ Col column(int p, int B) const {
    // (a column that pads the probe block: its words are not stored)
    const f32x4 v = (p < B) ? thr[p] : f32x4{0.f, 0.f, 0.f, 0.f};
    return Col{v[0], v[1], v[2]};
  }
  __device__ __forceinline__ State start(const Tile&, int) const { return State{0, 0}; }
  __device__ __forceinline__ void visit(State& s, const Col& c, const Rows&, int, float key, bool ok) const {
    key = ok ? key : __builtin_inff();
    s.sure += (key <= c.ts && fabsf(key) < c.hk) ? 1 : 0;
    s.nout += !(key > c.tm) ? 1 : 0;
  }
  __device__ __forceinline__ Meet partial(const State& s) const { return s.sure | (s.nout << 16); }
  __device__ static __forceinline__ Meet combine(Meet a, Meet b) { return a + b; }
  __device__ __forceinline__ void store(int64_t i, Meet v) const {
    const int sure = v & 0xffff, bord = (v >> 16) - sure;     // SURE implies not OUT (T - E <= T + E)
    census[i] = (unsigned short)(sure | (bord << 8));
  }
};

// The tagged census policy: CensusEpi's two counts over the ELIGIBLE rows only.  The tags of the thread's four rows are read
// beside each `aux` load and the column's mask once per tile, through buffer descriptors bounded like `arsrc` (row_tags + g0
// over min(rows left, 128) * 8 bytes, probe_masks + p0 over the columns that exist): a row past G reads tag 0, a probe past B
// mask 0 -- never eligible.  Nothing is loaded per pair.  An ineligible row, like a row past G, adds to neither count, so
//   word == 0  <=>  the tile holds no eligible row that is SURE or not OUT.
// A tile with word 0 contributes nothing to a count and nothing to a list: its eligible rows are all OUT (distance > t, or
// NaN), its other rows are not the probe's.  Under the "resolve everything" flag the thresholds are (-inf, +inf): no key is
// SURE (key <= -inf only for key = -inf, which fails |key| < H), every key -- a NaN key included -- is "not OUT"
// (!(key > +inf)), so nout, and with it bord, is the number of ELIGIBLE rows of the tile: word 0 means "no eligible row here"
// there too, and the resolve kernels may skip it for such a probe as well.  (An untagged census counts the rows past G as
// borderline under that flag; here they read tag 0 and are not counted.)  bord <= 128 fits the word's upper byte as before.
struct TaggedCensusEpi : KeyEpi {
  const f32x4* __restrict__ thr;
  unsigned short* __restrict__ census;
  const int64_t* __restrict__ row_tags;
  const int64_t* __restrict__ probe_masks;
  using Meet = int;                                           // sure | not out << 16
  using Col = CensusEpi::Col;
  struct Tile {
    __amdgpu_buffer_rsrc_t trsrc, mrsrc;
  };
  struct Rows {
    u32x4 tg[2];                                              // four tags, {lo, hi} each
  };
  struct State {
    int sure, nout;
    u32x2 msk;                                                // the column's mask, once per tile
  };
  __device__ __forceinline__ TaggedCensusEpi(const f32x4* thr_, unsigned short* census_, const int64_t* row_tags_,
                                             const int64_t* probe_masks_)
      : thr(thr_), census(census_), row_tags(row_tags_), probe_masks(probe_masks_) {}
  __device__ __forceinline__ Col column(int p, int B) const {
    const f32x4 v = (p < B) ? thr[p] : f32x4{0.f, 0.f, 0.f, 0.f};
    return Col{v[0], v[1], v[2]};
  }
  __device__ __forceinline__ Tile tile(int64_t g0, int rows, int p0, int cols) const {
    return Tile{make_rsrc(row_tags + g0, (uint32_t)(rows * 8)), make_rsrc(probe_masks + p0, (uint32_t)(cols * 8))};
  }
  __device__ __forceinline__ State start(const Tile& t, int c) const {
    return State{0, 0, __builtin_amdgcn_raw_buffer_load_b64(t.mrsrc, (uint32_t)c * 8u, 0, 0)};
  }
  __device__ __forceinline__ Rows rows(const Tile& t, int r) const {
    return Rows{{__builtin_amdgcn_raw_buffer_load_b128(t.trsrc, (uint32_t)r * 8u, 0, 0),
                 __builtin_amdgcn_raw_buffer_load_b128(t.trsrc, (uint32_t)r * 8u + 16u, 0, 0)}};
  }
  __device__ __forceinline__ void visit(State& s, const Col& c, const Rows& rw, int j, float key, bool ok) const {
    // (a row past G reads tag 0 through the descriptor as well)
    const unsigned tlo = ok ? rw.tg[j >> 1][2 * (j & 1)] : 0u, thi = ok ? rw.tg[j >> 1][2 * (j & 1) + 1] : 0u;
    const bool elig = ((tlo & s.msk[0]) | (thi & s.msk[1])) != 0u;
    s.sure += (elig && key <= c.ts && fabsf(key) < c.hk) ? 1 : 0;
    s.nout += (elig && !(key > c.tm)) ? 1 : 0;
  }
  __device__ __forceinline__ Meet partial(const State& s) const { return s.sure | (s.nout << 16); }
  __device__ static __forceinline__ Meet combine(Meet a, Meet b) { return a + b; }
  __device__ __forceinline__ void store(int64_t i, Meet v) const {
    const int sure = v & 0xffff, bord = (v >> 16) - sure;     // SURE implies not OUT (T - E <= T + E)
    census[i] = (unsigned short)(sure | (bord << 8));
  }
};

// Tagged = false: the census as it was, with the arguments it had (`tagargs` is one WithinTags when Tagged, nothing otherwise)
template <class T, bool Tagged, class... TagArgs>
__global__ __launch_bounds__(T::NT, 2) void within_census_kernel(const float* __restrict__ gallery, int64_t G,
                                                               const float* __restrict__ probes, int B, int D,
                                                               const float* __restrict__ aux, int metric, int nparts,
                                                               const f32x4* __restrict__ thr,
                                                               unsigned short* __restrict__ census,
                                                               const TagArgs... tagargs) {
  static_assert(sizeof...(TagArgs) == (Tagged ? 1 : 0), "one WithinTags exactly when Tagged");
  if constexpr (Tagged)
    key_tiles<T>(gallery, G, probes, B, D, aux, metric, nparts,
                 TaggedCensusEpi(thr, census, within_tags(tagargs...).row_tags, within_tags(tagargs...).probe_masks));
  else key_tiles<T>(gallery, G, probes, B, D, aux, metric, nparts, CensusEpi(thr, census));
}

// One block per probe; `census` rows are B words apart.  All control flow is block-uniform: every wave derives the same
// counts from the same LDS words.  (This kernel and the two select kernels synchronise inside a tile and keep walk_words'
// loop written out: on the shared function they measured 1 to 5 % slower)
// Tagged (the words are within_census_kernel<T, true>'s): a tile whose word is 0 holds no eligible row that could be a hit
// and is never evaluated, also for a probe under the "resolve everything" flag (TaggedCensusEpi has the argument); inside an
// evaluated tile an ineligible row is skipped before ref_distance -- a wave handles one row, so the test is wave-uniform, and
// which tiles are evaluated still follows from the LDS words alone.  Every evaluated tile counts one into "within_tagged_tiles".
template <bool Tagged, class... TagArgs>
__global__ __launch_bounds__(64 * WITHIN_NW) void within_resolve_kernel(const unsigned short* __restrict__ census, int64_t G,
                                                                      int B, const f32x4* __restrict__ thr,
                                                                      const float* __restrict__ probes,
                                                                      const float* __restrict__ gallery, int D, int metric,
                                                                      float t, int clamp, const SumPlan plan, int K,
                                                                      int64_t index_base, int64_t* __restrict__ count_out,
                                                                      int64_t* __restrict__ idx_out,
                                                                      float* __restrict__ dist_out,
                                                                      const TagArgs... tagargs) {
  static_assert(sizeof...(TagArgs) == (Tagged ? 1 : 0), "one WithinTags exactly when Tagged");
  constexpr int NT = 64 * WITHIN_NW;
  __shared__ float scratch[WITHIN_NW][NP_SCRATCH];
  __shared__ unsigned short s_word[NT];
  __shared__ float s_dist[WITHIN_BM];
  __shared__ unsigned char s_hit[WITHIN_BM];
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* q = probes + (int64_t)p * D;
  const int64_t gtiles = (G + WITHIN_BM - 1) / WITHIN_BM;
  const bool all = gtiles > 0 && thr[p][3] != 0.f;
  unsigned long long pm = 0;                                  // Tagged: the probe's mask
  if constexpr (Tagged) pm = (unsigned long long)within_tags(tagargs...).probe_masks[p];
  unsigned ntiles = 0;                                        // Tagged: tiles this block evaluated row by row
  int64_t count = 0;                                          // hits so far; the list holds the first min(count, K) of them
  for (int64_t t0 = 0; t0 < gtiles; t0 += NT) {
    const unsigned short w = t0 + tid < gtiles ? census[(t0 + tid) * B + p] : (unsigned short)0;
    s_word[tid] = w;
    // (also the barrier between two rounds of words)
    if (!__syncthreads_or(Tagged ? w != 0 : (all || w != 0))) continue;
    const int nw = gtiles - t0 < NT ? (int)(gtiles - t0) : NT;
    for (int j = 0; j < nw; ++j) {
      const int sure = s_word[j] & 0xff, bord = s_word[j] >> 8;
      if constexpr (Tagged) {
        if (s_word[j] == 0) continue;                         // no eligible row that is SURE or not OUT; `all`: no eligible row
      }
      if (!(all || bord > 0 || (sure > 0 && count < K))) {
        count += sure;
        continue;
      }
      if constexpr (Tagged) ++ntiles;
      const int64_t g0 = (t0 + j) * WITHIN_BM;
      const int rows = G - g0 < WITHIN_BM ? (int)(G - g0) : WITHIN_BM;
      for (int r = wave; r < rows; r += WITHIN_NW) {
        if constexpr (Tagged) {
          if (((unsigned long long)within_tags(tagargs...).row_tags[g0 + r] & pm) == 0) {   // not eligible: never a hit
            if (lane == 0) s_hit[r] = 0;
            continue;
          }
        }
        float d;
        (void)ref_distance(plan, scratch[wave], q, gallery + (g0 + r) * D, metric, lane, &d, clamp != 0);
        if (lane == 0) {
          s_dist[r] = d;
          s_hit[r] = d <= t ? 1 : 0;                          // NaN: not a hit
        }
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < WITHIN_BM / 64; ++h) {
        const int r = h * 64 + lane;
        const bool hit = r < rows && s_hit[r] != 0;
        const unsigned long long mask = __ballot(hit);
        const int64_t pos = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && wave == 0 && pos < K) {
          idx_out[(int64_t)p * K + pos] = g0 + r + index_base;
          dist_out[(int64_t)p * K + pos] = s_dist[r];
        }
        count += __popcll(mask);
      }
      __syncthreads();                                        // s_dist / s_hit are rewritten by the next resolved tile
    }
    __syncthreads();                                          // s_word is rewritten by the next round
  }
  if (tid == 0) count_out[p] = count;
  for (int64_t i = (count < K ? count : K) + tid; i < K; i += NT) {
    idx_out[(int64_t)p * K + i] = -1;
    dist_out[(int64_t)p * K + i] = __builtin_nanf("");
  }
  if constexpr (Tagged) {
    if (tid == 0 && ntiles) atomicAdd(within_tags(tagargs...).tiles_stat, (unsigned long long)ntiles);
  }
}

// One block per probe, as within_resolve_kernel without the lists: a tile without a borderline row adds its SURE count (no
// memory touched), any other tile -- every tile under the "resolve everything" flag -- is evaluated row by row, a wave per
// row, and a row counts when it is closer than the mate or ties with it from a lower index.  Every wave keeps the count of
// its own rows; they meet once, in LDS, at the end.  Which tiles are evaluated is block-uniform (the same LDS words).
// EXT (dif_match_rank_at): the mate is named by its GLOBAL index mates[p] -- below, inside or above this shard -- and its
// distance was handed in: there is no "unmated", and a tie counts when the row's global index is below the mate's.
// Tagged: as in within_resolve_kernel -- a tile whose word is 0 is never evaluated, whatever the flag; an ineligible row is
// skipped before ref_distance: it is neither closer nor a tie; every evaluated tile counts one into "within_tagged_tiles".
template <bool EXT, bool Tagged, class... TagArgs>
__global__ __launch_bounds__(64 * WITHIN_NW) void rank_resolve_kernel(const unsigned short* __restrict__ census, int64_t G,
                                                                    int B, const f32x4* __restrict__ thr,
                                                                    const RankMate* __restrict__ mate,
                                                                    const float* __restrict__ probes,
                                                                    const float* __restrict__ gallery, int D, int metric,
                                                                    int clamp, const SumPlan plan,
                                                                    const int64_t* __restrict__ mates, int64_t index_base,
                                                                    int64_t* __restrict__ rank_out,
                                                                    const TagArgs... tagargs) {
  static_assert(sizeof...(TagArgs) == (Tagged ? 1 : 0), "one WithinTags exactly when Tagged");
  constexpr int NT = 64 * WITHIN_NW;
  __shared__ float scratch[WITHIN_NW][NP_SCRATCH];
  __shared__ unsigned short s_word[NT];
  __shared__ int s_part[WITHIN_NW];
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const RankMate mt = mate[p];
  if ((!EXT && mt.row < 0) || !(mt.dm == mt.dm)) {            // unmated: -1; the mate's distance is NaN: behind every row
    if (tid == 0) rank_out[p] = (!EXT && mt.row < 0) ? -1 : G;
    return;
  }
  const int64_t m_ext = EXT ? mates[p] : 0;
  const float dm = mt.dm;
  const float* q = probes + (int64_t)p * D;
  const int64_t gtiles = (G + WITHIN_BM - 1) / WITHIN_BM;
  const bool all = thr[p][3] != 0.f;
  int64_t sure_rows = 0;                                      // the same in every thread
  int mine = 0;                                               // rows this wave evaluated and counted (G < 2^31)
  unsigned long long pm = 0;                                  // Tagged: the probe's mask
  if constexpr (Tagged) pm = (unsigned long long)within_tags(tagargs...).probe_masks[p];
  unsigned ntiles = 0;                                        // Tagged: tiles this block evaluated row by row
  walk_words(census, B, p, gtiles, s_word, [&](unsigned short w) { return Tagged ? w != 0 : (all || w != 0); },
             [&](int64_t tl, unsigned short w) {
    const int sure = w & 0xff, bord = w >> 8;
    if constexpr (Tagged) {
      if (w == 0) return;                                     // no eligible row that is SURE or not OUT; `all`: no eligible row
    }
    if (!(all || bord > 0)) {
      sure_rows += sure;
      return;
    }
    if constexpr (Tagged) ++ntiles;
    const int64_t g0 = tl * WITHIN_BM;
    const int rows = G - g0 < WITHIN_BM ? (int)(G - g0) : WITHIN_BM;
    for (int r = wave; r < rows; r += WITHIN_NW) {
      if constexpr (Tagged) {
        if (((unsigned long long)within_tags(tagargs...).row_tags[g0 + r] & pm) == 0) continue;   // not eligible: neither
      }
      float d;
      (void)ref_distance(plan, scratch[wave], q, gallery + (g0 + r) * D, metric, lane, &d, clamp != 0);
      const bool lower = EXT ? index_base + g0 + r < m_ext : g0 + r < mt.row;
      mine += (d < dm || (d == dm && lower)) ? 1 : 0;         // NaN: neither
    }
  });
  if (lane == 0) s_part[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    int64_t rank = sure_rows;
#pragma unroll
    for (int w = 0; w < WITHIN_NW; ++w) rank += s_part[w];
    rank_out[p] = rank;
    if constexpr (Tagged) {
      if (ntiles) atomicAdd(within_tags(tagargs...).tiles_stat, (unsigned long long)ntiles);
    }
  }
}

// The census of nb probes at the thresholds in g->within_thr, over gallery rows [0, rows) only (-1: all of them); its words are
// laid out as for a gallery of `rows` rows.  `tags` given: the tagged census, tags->probe_masks being these probes'.
static int census_pass(const Gallery* g, const float* pr, int nb, int metric, hipStream_t st, int64_t rows = -1,
                       const WithinTags* tags = nullptr) {
  return with_census_tile(nb, [&](auto tile) {
    using T = decltype(tile);
    const int nparts = key_tiles_parts(g, nb, rows);
    const f32x4* thr = reinterpret_cast<const f32x4*>(g->within_thr);
    return tags ? launch_key_tiles<within_census_kernel<T, true, WithinTags>, T>(g, pr, nb, metric, st, key_tiles_lds<T>, rows, nparts,
                                                                                 thr, g->within_census, *tags)
                : launch_key_tiles<within_census_kernel<T, false>, T>(g, pr, nb, metric, st, key_tiles_lds<T>, rows, nparts, thr,
                                                                      g->within_census);
  });
}

// the counter of "within_tagged_tiles", zeroed on the stream by every tagged within / rank / rank_at call
static int within_tagged_stat_reset(Gallery* g, hipStream_t st) {
  if (!g->within_tagged_stat) DIF_HIP(hipMalloc(&g->within_tagged_stat, sizeof(unsigned long long)));
  DIF_HIP(hipMemsetAsync(g->within_tagged_stat, 0, sizeof(unsigned long long), st));
  return 0;
}

// row_tags null: dif_match_within; else dif_match_within_tagged (probe_masks [B]).  The masks advance with the probes from
// round to round, the tags belong to the rows and do not.
int within_run(Gallery* g, const float* probes, int B, int metric, float tolerance, int max_hits, int64_t* count_out,
               int64_t* idx_out, float* dist_out, hipStream_t st, const int64_t* row_tags, const int64_t* probe_masks) {
  if (B <= 0) return 0;
  const bool tagged = row_tags != nullptr;
  if (tagged && within_tagged_stat_reset(g, st)) return -1;
  SumPlan plan;
  if (make_sum_plan(g->d, &plan)) return -1;
  const int clamp = g->clamp_nan ? 1 : 0;
  if (g->n <= 0) {                                           // np.flatnonzero of an empty array: counts 0, lists all padding
    hipLaunchKernelGGL(within_resolve_kernel<false>, dim3(B), dim3(64 * WITHIN_NW), 0, st, nullptr, (int64_t)0, B, nullptr, probes,
                       nullptr, g->d, metric, tolerance, clamp, plan, max_hits, g->index_base, count_out, idx_out, dist_out);
    DIF_HIP(hipGetLastError());
    return 0;
  }
  const int64_t gtiles = (g->n + WITHIN_BM - 1) / WITHIN_BM;
  const Rounds rounds = plan_rounds(gtiles, B, WITHIN_CENSUS_MAX, g->within_round, 128);
  if (ensure(st, workspace(&g->within_census, &g->within_census_cap, (size_t)gtiles * (size_t)rounds.per, sizeof(unsigned short)),
             workspace(&g->within_thr, &g->within_thr_cap, (size_t)rounds.per, 4 * sizeof(float))))
    return -1;
  const float cdot = g->d * U24;                              // the f32 MFMA: a D-term fma chain
  return for_rounds(rounds, 0, B, [&](int64_t b0, int nb) {
    const float* pr = probes + b0 * g->d;
    const WithinTags tags{row_tags, tagged ? probe_masks + b0 : nullptr, g->within_tagged_stat};
    hipLaunchKernelGGL(within_prep_kernel, dim3((nb + 3) / 4), dim3(256), 0, st, pr, nb, g->d, metric, tolerance, cdot,
                       g->sqmax_bits, reinterpret_cast<f32x4*>(g->within_thr));
    DIF_HIP(hipGetLastError());
    if (census_pass(g, pr, nb, metric, st, -1, tagged ? &tags : nullptr)) return -1;
    if (tagged)
      hipLaunchKernelGGL((within_resolve_kernel<true, WithinTags>), dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->within_census, g->n, nb,
                         reinterpret_cast<const f32x4*>(g->within_thr), pr, g->rows, g->d, metric, tolerance, clamp, plan,
                         max_hits, g->index_base, count_out + b0, max_hits ? idx_out + b0 * max_hits : nullptr,
                         max_hits ? dist_out + b0 * max_hits : nullptr, tags);
    else
      hipLaunchKernelGGL(within_resolve_kernel<false>, dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->within_census, g->n, nb,
                         reinterpret_cast<const f32x4*>(g->within_thr), pr, g->rows, g->d, metric, tolerance, clamp, plan,
                         max_hits, g->index_base, count_out + b0, max_hits ? idx_out + b0 * max_hits : nullptr,
                         max_hits ? dist_out + b0 * max_hits : nullptr);
    DIF_HIP(hipGetLastError());
    return 0;
  });
}

// row_tags null: dif_match_mate_dist; else dif_match_mate_dist_tagged (no tile is evaluated: the counter is left alone)
int mate_dist_run(Gallery* g, const float* probes, int B, int metric, const int64_t* mates, float* mate_dist_out,
                  int64_t* owned_out, hipStream_t st, const int64_t* row_tags, const int64_t* probe_masks) {
  if (B <= 0) return 0;
  SumPlan plan;
  if (make_sum_plan(g->d, &plan)) return -1;
  if (row_tags)
    hipLaunchKernelGGL((mate_dist_kernel<true, WithinTags>), dim3((B + 3) / 4), dim3(256), 0, st, probes, B, g->d, metric, g->rows,
                       g->n, g->index_base, mates, g->clamp_nan ? 1 : 0, plan, mate_dist_out, owned_out,
                       WithinTags{row_tags, probe_masks, nullptr});
  else
    hipLaunchKernelGGL(mate_dist_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, st, probes, B, g->d, metric, g->rows, g->n,
                       g->index_base, mates, g->clamp_nan ? 1 : 0, plan, mate_dist_out, owned_out);
  DIF_HIP(hipGetLastError());
  return 0;
}

// `dm_in` null: dif_match_rank.  Not null: dif_match_rank_at -- the mates' distances are the caller's, rank_out receives the
// shard's count and mate_dist_out is not written.  row_tags given: the tagged forms (probe_masks [B], advancing with the
// probes from round to round; the tags do not).
int rank_run(Gallery* g, const float* probes, int B, int metric, const int64_t* mates, const float* dm_in, int64_t* rank_out,
             float* mate_dist_out, hipStream_t st, const int64_t* row_tags, const int64_t* probe_masks) {
  if (B <= 0) return 0;
  const bool tagged = row_tags != nullptr;
  if (tagged && within_tagged_stat_reset(g, st)) return -1;
  if (dm_in && g->n <= 0) {                                   // an empty shard counts nothing, whatever dm is (NaN: its size, 0);
    DIF_HIP(hipMemsetAsync(rank_out, 0, (size_t)B * sizeof(int64_t), st));   // a handle never filled has no sqmax_bits for the band
    return 0;
  }
  SumPlan plan;
  if (make_sum_plan(g->d, &plan)) return -1;
  const int clamp = g->clamp_nan ? 1 : 0;
  const int64_t gtiles = (g->n + WITHIN_BM - 1) / WITHIN_BM;
  // (an empty gallery has no census: one round, every probe unmated)
  const Rounds rounds = plan_rounds(gtiles, B, WITHIN_CENSUS_MAX, g->within_round, 128);
  if (ensure(st, workspace(&g->within_census, &g->within_census_cap, (size_t)gtiles * (size_t)rounds.per, sizeof(unsigned short)),
             workspace(&g->within_thr, &g->within_thr_cap, (size_t)rounds.per, 4 * sizeof(float)),
             workspace(&g->rank_mate, &g->rank_mate_cap, (size_t)rounds.per, sizeof(RankMate))))
    return -1;
  const float cdot = g->d * U24;
  return for_rounds(rounds, 0, B, [&](int64_t b0, int nb) {
    const float* pr = probes + b0 * g->d;
    const WithinTags tags{row_tags, tagged ? probe_masks + b0 : nullptr, g->within_tagged_stat};
    const dim3 pgrid((nb + 3) / 4), rblock(64 * WITHIN_NW);
    f32x4* thr = reinterpret_cast<f32x4*>(g->within_thr);
    float* md = mate_dist_out ? mate_dist_out + b0 : nullptr;
    const float* dmi = dm_in ? dm_in + b0 : nullptr;
    if (tagged)
      hipLaunchKernelGGL((rank_prep_kernel<true, WithinTags>), pgrid, dim3(256), 0, st, pr, nb, g->d, metric, cdot, g->sqmax_bits,
                         g->rows, g->n, g->index_base, mates + b0, clamp, plan, thr, g->rank_mate, md, dmi, tags);
    else
      hipLaunchKernelGGL(rank_prep_kernel<false>, pgrid, dim3(256), 0, st, pr, nb, g->d, metric, cdot, g->sqmax_bits, g->rows, g->n,
                         g->index_base, mates + b0, clamp, plan, thr, g->rank_mate, md, dmi);
    DIF_HIP(hipGetLastError());
    if (gtiles > 0 && census_pass(g, pr, nb, metric, st, -1, tagged ? &tags : nullptr)) return -1;
    if (tagged)
      hipLaunchKernelGGL((dm_in ? rank_resolve_kernel<true, true, WithinTags> : rank_resolve_kernel<false, true, WithinTags>), dim3(nb),
                         rblock, 0, st, g->within_census, g->n, nb, thr, g->rank_mate, pr, g->rows, g->d, metric, clamp, plan,
                         mates + b0, g->index_base, rank_out + b0, tags);
    else
      hipLaunchKernelGGL((dm_in ? rank_resolve_kernel<true, false> : rank_resolve_kernel<false, false>), dim3(nb), rblock, 0, st,
                         g->within_census, g->n, nb, thr, g->rank_mate, pr, g->rows, g->d, metric, clamp, plan, mates + b0,
                         g->index_base, rank_out + b0);
    DIF_HIP(hipGetLastError());
    return 0;
  });
}

// ---------------------------------------------------------------------------------------------
// The k nearest rows, in order (dif_match_topk).  Per probe q:
//   d = distance(q[None, :], gallery, metric);  order = np.argsort(d, kind='stable');  keep = order[~isnan(d[order])][:k]
//   idx = keep + index_base;  dist = d[keep];  unused slots: idx -1, dist NaN
// Built on ONE fact, the OUT bound of the header comment: for a tolerance t, a row whose search key is > T(t) + E(t) has a
// reference distance > t, or NaN.  No inverse of T, no SURE bound, no lists in the MFMA stage, no atomics on global memory.
//   topk_tilemin_kernel  key_tiles with the tile-minimum policy: the census' tiles, main loop, block order and keys; per (gallery tile
//                        of 128 rows, probe) it stores ONE float, the minimum key of the tile ("word"): -inf when a key of
//                        the tile is NaN (a row kept out of the filter), rows past G count as +inf.  It takes no thresholds.
//   topk_select_kernel   one block per probe (|q|^2 and the band are formed here: there is no prep kernel).
//     seed    kappa = the s-th smallest word of the probe (s = k, or "topk_seed"; every tile when there are no more than s),
//             by a radix select on the order-preserving integer image of the float.  Every tile with word <= kappa is
//             evaluated row by row with ref_distance, a wave per row; a NaN distance is dropped.
//     list    candidates are 64-bit words  ordered(dist) << 32 | local row: unique, so their order is total, and it is the
//             stable argsort's (distances are >= +0).  After each evaluated tile its at most 128 words are merged with the
//             at most k kept ones by a bitonic sort in LDS and the smallest k are kept.  No overflow path: the kept set is
//             the k smallest seen, whatever the tile order.
//     t       the k-th smallest kept distance -- an actual reference distance -- or +inf when fewer than k were found;
//             thr_out = T(t) + E(t) from within_band, unchanged.
//     sweep   every tile not yet evaluated (word > kappa) whose word is not > thr_out is evaluated and merged the same way:
//             a -inf word, and every tile when the probe is outside the bound's validity or thr_out is +inf or NaN.
//     output  the kept words in ascending order, then the padding.
// Why it is exact.  Let d_k be the k-th smallest distance that is not NaN (the list is short otherwise and t = +inf: every
// tile is evaluated).  After the seed the list holds k actual distances, so t >= d_k.  Every true top-k row has d <= d_k <= t,
// so its key is not OUT at t, so the word of its tile -- the minimum of the tile's keys, or -inf -- is <= thr_out or -inf, so
// its tile is evaluated, in the seed or in the sweep.  A tile with word > thr_out holds only rows with d > t >= d_k or NaN.
// Correctness never depends on kappa: kappa only decides how tight t is.  (Under "clamp_nan" a similarity rounded above 1 is
// reported as 0: its key lies within E of -|q| <= T(t) for every t >= 0, so it is not OUT; one rounded below -1 is reported
// as 1 and can be listed only when t >= 1, where T = +inf and nothing is OUT.)
constexpr int TOPK_MAX = 128;                                 // DIF_TOPK_MAX
constexpr size_t TOPK_MIN_MAX = WITHIN_CENSUS_MAX / 2;        // tile words (floats) per launch: the census' cap in bytes
constexpr unsigned long long TOPK_NONE = ~0ull;               // an empty slot of the list: above every candidate

// order-preserving integer image of a float that is not NaN (-inf lowest), and back
__device__ __forceinline__ unsigned ord_f32(float x) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(unsigned o) {
  return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// the integer image of the need-th smallest word of probe p (1 <= need <= gtiles): a radix select on the order-preserving
// integer image of the float, one byte per pass (exact counts: deterministic)
__device__ __forceinline__ unsigned topk_kappa(const float* __restrict__ words, int B, int p, int64_t gtiles,
                                                   unsigned need, unsigned* s_hist, unsigned* s_sel) {
  constexpr int NT = 64 * WITHIN_NW;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned prefix = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int64_t t = tid; t < gtiles; t += NT) {
      const unsigned o = ord_f32(words[t * B + p]);
      if ((unsigned)((unsigned long long)o >> (shift + 8)) == prefix) atomicAdd(&s_hist[(o >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wave == 0) {                                          // four bins per lane, a scan over the lanes
      unsigned c[4], sum = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        c[i] = s_hist[4 * lane + i];
        sum += c[i];
      }
      unsigned incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      const unsigned excl = incl - sum;
      if (excl < need && need <= incl) {                      // exactly one lane: 1 <= need <= the total
        unsigned r = need - excl;
        int d = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (d == i && r > c[i]) {
            r -= c[i];
            d = i + 1;
          }
        s_sel[0] = (unsigned)(4 * lane + d);
        s_sel[1] = r;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | s_sel[0];
    need = s_sel[1];
    // (s_sel is written again only behind the two barriers of the next pass, or of the next call)
  }
  return prefix;
}

// The tile-minimum policy of key_tiles.  aux is NaN for the rows kept out of the filter: fminf drops a NaN, so a NaN key is
// tested for and makes the minimum -inf.
struct TileMinEpi : KeyEpi {
  float* __restrict__ words;
  using Meet = float;
  struct State {
    float mn;
  };
  __device__ __forceinline__ explicit TileMinEpi(float* words_) : words(words_) {}
  __device__ __forceinline__ State start(const Tile&, int) const { return State{__builtin_inff()}; }
  __device__ __forceinline__ void visit(State& s, const Col&, const Rows&, int, float key, bool ok) const {
    key = ok ? key : __builtin_inff();                        // a row past G
    s.mn = (key != key) ? -__builtin_inff() : fminf(s.mn, key);   // (once -inf it stays -inf)
  }
  __device__ __forceinline__ Meet partial(const State& s) const { return s.mn; }
  __device__ static __forceinline__ Meet combine(Meet a, Meet b) { return fminf(a, b); }
  __device__ __forceinline__ void store(int64_t i, Meet v) const { words[i] = v; }
};

// Tagged (dif_match_topk_tagged, dif_match_topk_ids_tagged): row r is eligible for probe p iff (row_tags[r] & probe_masks[p])
// != 0, on the raw 64 bits.  The word becomes the minimum key over the ELIGIBLE rows of the tile (-inf when an eligible row's
// key is NaN), and a tile with no eligible row for the probe stores a positive quiet NaN: "nothing here".  No eligible row can
// produce that word -- a NaN key is turned into -inf before it reaches the minimum, and every other key is a number or an
// infinity -- so the select stages skip a NaN word in every phase, also where t = +inf or the probe is outside the bound's
// validity and every other tile is evaluated.  (+inf would not do: an enrolled row with an overflowed |g|^2 has the key +inf
// under metric 0.)  The minimum starts as NaN, fminf drops a NaN operand, so the reductions over lanes and waves keep NaN
// exactly when every part is NaN.  The tags of the thread's rows and the masks of its probe columns are read once per tile
// through buffer descriptors bounded like `arsrc`: a row past G reads tag 0, a probe past B mask 0 -- never eligible.
// The tagged tile-minimum policy: the four row tags per q step and the column masks per tile
struct TaggedTileMinEpi : KeyEpi {
  float* __restrict__ words;
  const int64_t* __restrict__ row_tags;
  const int64_t* __restrict__ probe_masks;
  using Meet = float;
  struct Tile {
    __amdgpu_buffer_rsrc_t trsrc, mrsrc;
  };
  struct Rows {
    u32x4 tg[2];                                              // four tags, {lo, hi} each
  };
  struct State {
    float mn;
    u32x2 msk;                                                // the column's mask, once per tile
  };
  __device__ __forceinline__ TaggedTileMinEpi(float* words_, const int64_t* row_tags_, const int64_t* probe_masks_)
      : words(words_), row_tags(row_tags_), probe_masks(probe_masks_) {}
  __device__ __forceinline__ Tile tile(int64_t g0, int rows, int p0, int cols) const {
    return Tile{make_rsrc(row_tags + g0, (uint32_t)(rows * 8)), make_rsrc(probe_masks + p0, (uint32_t)(cols * 8))};
  }
  __device__ __forceinline__ State start(const Tile& t, int c) const {   // no eligible row yet
    return State{__builtin_nanf(""), __builtin_amdgcn_raw_buffer_load_b64(t.mrsrc, (uint32_t)c * 8u, 0, 0)};
  }
  __device__ __forceinline__ Rows rows(const Tile& t, int r) const {
    return Rows{{__builtin_amdgcn_raw_buffer_load_b128(t.trsrc, (uint32_t)r * 8u, 0, 0),
                 __builtin_amdgcn_raw_buffer_load_b128(t.trsrc, (uint32_t)r * 8u + 16u, 0, 0)}};
  }
  __device__ __forceinline__ void visit(State& s, const Col&, const Rows& rw, int j, float key, bool ok) const {
    // (a row past G reads tag 0 through the descriptor as well)
    const unsigned tlo = ok ? rw.tg[j >> 1][2 * (j & 1)] : 0u, thi = ok ? rw.tg[j >> 1][2 * (j & 1) + 1] : 0u;
    const bool elig = ((tlo & s.msk[0]) | (thi & s.msk[1])) != 0u;   // false for a row past G (tag 0)
    const float with = (key != key) ? -__builtin_inff() : fminf(s.mn, key);   // fminf(NaN, key) = key
    s.mn = elig ? with : s.mn;
  }
  __device__ __forceinline__ Meet partial(const State& s) const { return s.mn; }
  __device__ static __forceinline__ Meet combine(Meet a, Meet b) { return fminf(a, b); }
  __device__ __forceinline__ void store(int64_t i, Meet v) const {
    words[i] = (v != v) ? __builtin_nanf("") : v;             // one bit pattern for "nothing here"
  }
};

// Tagged = false takes no tags: the two pointers are unused there.
template <class T, bool Tagged>
__global__ __launch_bounds__(T::NT, 2) void topk_tilemin_kernel(const float* __restrict__ gallery, int64_t G,
                                                              const float* __restrict__ probes, int B, int D,
                                                              const float* __restrict__ aux, int metric, int nparts,
                                                              float* __restrict__ words,
                                                              const int64_t* __restrict__ row_tags,
                                                              const int64_t* __restrict__ probe_masks) {
  if constexpr (Tagged) key_tiles<T>(gallery, G, probes, B, D, aux, metric, nparts, TaggedTileMinEpi(words, row_tags, probe_masks));
  else key_tiles<T>(gallery, G, probes, B, D, aux, metric, nparts, TileMinEpi(words));
}

// One block per probe; `words` rows are B floats apart.  All control flow is block-uniform: every thread derives kappa, t and
// thr_out from the same LDS words, and which tiles are evaluated follows from those alone.
// (four waves per SIMD asked for: two blocks per CU overlap the latency of the row-by-row stage -- DESIGN 4i has the A/B)
// Tagged (the words are topk_tilemin_kernel<T, true>'s): a NaN word -- no eligible row in the tile -- is selected in neither
// phase, whatever kappa, `all` and thr_out are; an ineligible row is skipped before ref_distance (one wave per row: the test
// is wave-uniform).  The argument above holds with "row" read as "eligible row": a word is the minimum key over the tile's
// eligible rows (or -inf), every true top-k row is eligible, so its tile's word is a number <= thr_out or -inf and the tile is
// evaluated; t is the distance of an eligible row.  `tiles_stat` counts the (probe, tile) evaluations ("topk_tagged_tiles").
// Tagged = false is the kernel as it was, with the arguments it had: `tagargs` is one TopkTags when Tagged, nothing otherwise.
struct TopkTags {
  const int64_t* row_tags;                                    // [G]
  const int64_t* probe_masks;                                 // [B], this launch's probes
  unsigned long long* tiles_stat;                             // "topk_tagged_tiles"
};
__device__ __forceinline__ const TopkTags& topk_tags(const TopkTags& t) { return t; }

template <bool Tagged, class... TagArgs>
__global__ __launch_bounds__(64 * WITHIN_NW, 4) void topk_select_kernel(const float* __restrict__ words, int64_t G, int B,
                                                                   const float* __restrict__ probes,
                                                                   const float* __restrict__ gallery, int D, int metric,
                                                                   float cdot, const unsigned* __restrict__ sqmax_bits,
                                                                   int clamp, const SumPlan plan, int k, int seed,
                                                                   int64_t index_base, int64_t* __restrict__ idx_out,
                                                                   float* __restrict__ dist_out,
                                                                   const TagArgs... tagargs) {
  static_assert(sizeof...(TagArgs) == (Tagged ? 1 : 0), "one TopkTags exactly when Tagged");
  constexpr int NT = 64 * WITHIN_NW;
  static_assert(2 * TOPK_MAX <= NT && TOPK_MAX == WITHIN_BM, "the list holds k kept words and one tile's");
  __shared__ float scratch[WITHIN_NW][NP_SCRATCH];
  __shared__ unsigned long long s_list[2 * TOPK_MAX];         // [0, k): kept, ascending; [TOPK_MAX, ..): the tile being merged
  __shared__ float s_word[NT];
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_sel[2];
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* q = probes + (int64_t)p * D;
  const int64_t gtiles = (G + WITHIN_BM - 1) / WITHIN_BM;
  const float inf = __builtin_inff();
  if (tid < 2 * TOPK_MAX) s_list[tid] = TOPK_NONE;
  __syncthreads();

  // ---- seed: kappa = the seed-th smallest word; no more than `seed` tiles: all of them
  const unsigned kappa = (int64_t)seed < gtiles ? topk_kappa(words, B, p, gtiles, (unsigned)seed, s_hist, s_sel) : ~0u;

  unsigned ntiles = 0;                                        // Tagged: tiles this block evaluated row by row
  if (gtiles > 0) {
    const float s = probe_sq(q, D, lane);                     // the same in every thread
    unsigned long long pm = 0;                                // Tagged: the probe's mask
    if constexpr (Tagged) pm = (unsigned long long)topk_tags(tagargs...).probe_masks[p];
    bool all = false;
    float thr_out = 0.f;
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {                 // 0: the seed's tiles; 1: the sweep
      if (phase == 1) {
        const unsigned long long kth = s_list[k - 1];
        const float t = kth == TOPK_NONE ? inf : unord_f32((unsigned)(kth >> 32));
        const Band b = within_band(metric, t, s, D, cdot, sqmax_bits);
        all = b.odd;
        thr_out = b.T + b.E;
      }
      for (int64_t t0 = 0; t0 < gtiles; t0 += NT) {
        const float w = t0 + tid < gtiles ? words[(t0 + tid) * B + p] : inf;
        s_word[tid] = w;
        bool mine = phase == 0 ? ord_f32(w) <= kappa : (ord_f32(w) > kappa && (all || !(w > thr_out)));
        if constexpr (Tagged) mine = mine && w == w;          // a NaN word: no eligible row
        if (!__syncthreads_or(t0 + tid < gtiles && mine)) continue;   // (also the barrier between two rounds of words)
        const int nw = gtiles - t0 < NT ? (int)(gtiles - t0) : NT;
        for (int j = 0; j < nw; ++j) {
          const float wj = s_word[j];
          if (!(phase == 0 ? ord_f32(wj) <= kappa : (ord_f32(wj) > kappa && (all || !(wj > thr_out))))) continue;
          if constexpr (Tagged) {
            if (wj != wj) continue;
            ++ntiles;
          }
          const int64_t g0 = (t0 + j) * WITHIN_BM;
          const int rows = G - g0 < WITHIN_BM ? (int)(G - g0) : WITHIN_BM;
          const unsigned long long kth = s_list[k - 1];       // a word that is not below it cannot enter the list
          bool any = false;
          for (int r = wave; r < rows; r += WITHIN_NW) {
            if constexpr (Tagged) {
              if (((unsigned long long)topk_tags(tagargs...).row_tags[g0 + r] & pm) == 0) continue;   // not eligible: never a candidate
            }
            float d;
            (void)ref_distance(plan, scratch[wave], q, gallery + (g0 + r) * D, metric, lane, &d, clamp != 0);
            if (d == d) {                                     // a NaN distance is never listed
              const unsigned long long cand = ((unsigned long long)ord_f32(d) << 32) | (unsigned)(g0 + r);
              if (cand < kth) {
                if (lane == 0) s_list[TOPK_MAX + r] = cand;
                any = true;
              }
            }
          }
          if (!__syncthreads_or(any)) continue;
          // bitonic sort of the 2 * TOPK_MAX words, ascending; empty slots are above every candidate
          for (int k2 = 2; k2 <= 2 * TOPK_MAX; k2 <<= 1) {
            for (int h = k2 >> 1; h > 0; h >>= 1) {
              if (tid < TOPK_MAX) {
                const int i = ((tid & ~(h - 1)) << 1) | (tid & (h - 1)), l = i | h;
                const unsigned long long a = s_list[i], b = s_list[l];
                if ((a > b) == ((i & k2) == 0)) {
                  s_list[i] = b;
                  s_list[l] = a;
                }
              }
              __syncthreads();
            }
          }
          if (tid >= k && tid < 2 * TOPK_MAX) s_list[tid] = TOPK_NONE;   // keep the smallest k
          __syncthreads();
        }
        __syncthreads();                                      // s_word is rewritten by the next round
      }
    }
  }

  if (tid < k) {
    const unsigned long long w = s_list[tid];
    idx_out[(int64_t)p * k + tid] = w == TOPK_NONE ? -1 : (int64_t)(unsigned)w + index_base;
    dist_out[(int64_t)p * k + tid] = w == TOPK_NONE ? __builtin_nanf("") : unord_f32((unsigned)(w >> 32));
  }
  if constexpr (Tagged) {
    if (tid == 0 && ntiles) atomicAdd(topk_tags(tagargs...).tiles_stat, (unsigned long long)ntiles);
  }
}

// What the four top-k entries share on the host.  The rounds, and the tile words' workspace for one of them:
static int topk_plan(Gallery* g, int B, int64_t gtiles, hipStream_t st, Rounds* rounds) {
  *rounds = plan_rounds(gtiles, B, TOPK_MIN_MAX, g->topk_round, 128);
  return ensure(st, workspace(&g->topk_min, &g->topk_min_cap, (size_t)gtiles * (size_t)rounds->per, sizeof(float)));
}
// ... and the tile words of nb probes into g->topk_min; row_tags given: the tagged form, probe_masks being these probes'
static int tilemin_pass(const Gallery* g, const float* pr, int nb, int metric, hipStream_t st, const int64_t* row_tags,
                        const int64_t* probe_masks) {
  const int nparts = key_tiles_parts(g, nb);
  return with_census_tile(nb, [&](auto tile) {
    using T = decltype(tile);
    return row_tags ? launch_key_tiles<topk_tilemin_kernel<T, true>, T>(g, pr, nb, metric, st, key_tiles_lds<T>, -1, nparts, g->topk_min,
                                                                        row_tags, probe_masks)
                    : launch_key_tiles<topk_tilemin_kernel<T, false>, T>(g, pr, nb, metric, st, key_tiles_lds<T>, -1, nparts, g->topk_min,
                                                                         row_tags, probe_masks);
  });
}

// the counter of "topk_tagged_tiles", zeroed on the stream by every tagged call
static int tagged_stat_reset(Gallery* g, hipStream_t st) {
  if (!g->topk_tagged_stat) DIF_HIP(hipMalloc(&g->topk_tagged_stat, sizeof(unsigned long long)));
  DIF_HIP(hipMemsetAsync(g->topk_tagged_stat, 0, sizeof(unsigned long long), st));
  return 0;
}

// row_tags null: dif_match_topk; else dif_match_topk_tagged (probe_masks [B])
int topk_run(Gallery* g, const float* probes, int B, int metric, int k, int64_t* idx_out, float* dist_out, hipStream_t st,
             const int64_t* row_tags, const int64_t* probe_masks) {
  if (B <= 0) return 0;
  const bool tagged = row_tags != nullptr;
  if (tagged && tagged_stat_reset(g, st)) return -1;
  SumPlan plan;
  if (make_sum_plan(g->d, &plan)) return -1;
  const int clamp = g->clamp_nan ? 1 : 0;
  const int seed = g->topk_seed > 0 ? g->topk_seed : k;
  const int64_t gtiles = (g->n + WITHIN_BM - 1) / WITHIN_BM;
  Rounds rounds;
  if (topk_plan(g, B, gtiles, st, &rounds)) return -1;
  const float cdot = g->d * U24;                              // the f32 MFMA: a D-term fma chain
  return for_rounds(rounds, 0, B, [&](int64_t b0, int nb) {
    const float* pr = probes + b0 * g->d;
    const int64_t* pm = tagged ? probe_masks + b0 : nullptr;
    if (gtiles > 0 && tilemin_pass(g, pr, nb, metric, st, row_tags, pm)) return -1;
    if (tagged)
      hipLaunchKernelGGL((topk_select_kernel<true, TopkTags>), dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->topk_min, g->n, nb, pr, g->rows,
                         g->d, metric, cdot, g->sqmax_bits, clamp, plan, k, seed, g->index_base, idx_out + b0 * k,
                         dist_out + b0 * k, TopkTags{row_tags, pm, g->topk_tagged_stat});
    else
      hipLaunchKernelGGL((topk_select_kernel<false>), dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->topk_min, g->n, nb, pr, g->rows,
                         g->d, metric, cdot, g->sqmax_bits, clamp, plan, k, seed, g->index_base, idx_out + b0 * k,
                         dist_out + b0 * k);
    DIF_HIP(hipGetLastError());
    return 0;
  });
}

// ---------------------------------------------------------------------------------------------
// The k nearest distinct identities, each with its best row (dif_match_topk_ids).  Per probe q, with row_labels [G] and an
// optional excluded label:
//   d = distance(q[None, :], gallery, metric);  ok = ~isnan(d) & (row_labels >= 0) & (row_labels != exclude[p])
//   order = np.argsort(d, kind='stable');  order = order[ok[order]]
//   keep = the first row of every label in `order`, the first k of those;  idx, dist, label of keep, then the padding
// The MFMA pass is dif_match_topk's, unchanged: a word is the minimum key over ALL rows of its tile -- excluded rows, negative
// labels and duplicates included -- hence a lower bound of the minimum over the usable rows, and "word > T(t) + E(t) => no row
// of the tile has a distance <= t" holds as it does there.  topk_ids_select_kernel differs from topk_select_kernel in three ways:
//   usable   a row with a negative label or the probe's excluded label is never evaluated and never a candidate.
//   list     the kept entries have distinct labels: after each evaluated tile the kept set is, for every label seen so far, its
//            smallest word, and of those the k smallest.  The tile's candidates (words below the k-th kept one) and the kept
//            entries stand in one LDS array with their labels beside them; every entry that finds a smaller word of its own
//            label there is struck out, then the bitonic sort (labels moved with their words) and the cut to k.  The k-th
//            kept word only ever decreases, so an entry pushed out can never matter again, a later smaller word of its label
//            enters on its own, and the kept set is a function of the set of rows seen, not of their order.
//   seed     with several rows per identity the s tiles with the smallest words hold few identities, and a single seed leaves
//            t loose (or +inf) and the sweep long.  So the seed grows: s = "topk_seed" or k; loop { kappa = the s-th smallest
//            word; evaluate the tiles not yet evaluated with word <= kappa; t = the k-th kept distance or +inf, thr_out =
//            T(t) + E(t); n = the tiles with word > kappa that are not > thr_out (all of them when the probe is outside the
//            bound's validity); leave when n <= s or every tile is evaluated; s *= 2 }.  Then the sweep over those n tiles.
// Why it is exact.  Let d_k be the k-th smallest per-identity best distance over the usable rows (fewer than k identities: the
// list is short, t = +inf and every tile is evaluated).  Whenever the list is full it holds k actual distances of k distinct
// labels, each at least its label's best, so t >= d_k.  Every answer row has d <= d_k <= t, so it is not OUT at t, so its tile's
// word is not > thr_out, so the tile is evaluated in a seed pass or in the sweep -- and t only decreases while the sweep runs,
// which only tightens the pre-filter "candidate < k-th kept word", never thr_out.  The seed schedule decides how tight t is,
// never the answer.
constexpr long long TOPK_NOLABEL = -1;                        // the label of an empty slot: no usable row carries it

// One block per probe, block-uniform control flow, as topk_select_kernel.  `tiles_stat` counts the (probe, tile) evaluations.
// Tagged as topk_select_kernel<true>: a NaN word is never selected nor counted among the tiles left, an ineligible row is
// not usable, and the evaluations are also added to `tagged_stat`.  Tagged = false is the kernel as it was.
template <bool Tagged, class... TagArgs>
__global__ __launch_bounds__(64 * WITHIN_NW, 4) void topk_ids_select_kernel(
    const float* __restrict__ words, int64_t G, int B, const float* __restrict__ probes, const float* __restrict__ gallery, int D,
    int metric, float cdot, const unsigned* __restrict__ sqmax_bits, int clamp, const SumPlan plan, int k, int seed,
    int64_t index_base, const int64_t* __restrict__ row_labels, const int64_t* __restrict__ exclude,
    int64_t* __restrict__ idx_out, float* __restrict__ dist_out, int64_t* __restrict__ label_out,
    unsigned long long* __restrict__ tiles_stat, const TagArgs... tagargs) {
  static_assert(sizeof...(TagArgs) == (Tagged ? 1 : 0), "one TopkTags exactly when Tagged");
  constexpr int NT = 64 * WITHIN_NW;
  __shared__ float scratch[WITHIN_NW][NP_SCRATCH];
  __shared__ unsigned long long s_list[2 * TOPK_MAX];         // [0, k): kept, ascending; [TOPK_MAX, ..): the tile being merged
  __shared__ long long s_lab[2 * TOPK_MAX];                   // the label of each word
  __shared__ float s_word[NT];
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_sel[2];
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* q = probes + (int64_t)p * D;
  const int64_t gtiles = (G + WITHIN_BM - 1) / WITHIN_BM;
  const float inf = __builtin_inff();
  const long long ex = exclude ? (long long)exclude[p] : TOPK_NOLABEL;   // negative: nothing excluded (usable labels are >= 0)
  if (tid < 2 * TOPK_MAX) {
    s_list[tid] = TOPK_NONE;
    s_lab[tid] = TOPK_NOLABEL;
  }
  __syncthreads();

  unsigned ntiles = 0;                                        // tiles this block evaluated row by row
  if (gtiles > 0) {
    const float s = probe_sq(q, D, lane);                     // the same in every thread
    long long lo = -1;                                        // tiles with ord(word) <= lo are evaluated already
    unsigned kappa = ~0u;
    bool all = false;
    float thr_out = inf;
    int sd = seed;

    // evaluates and merges the tiles the pass selects: a seed pass those with lo < ord(word) <= kappa, the sweep those with
    // ord(word) > kappa that are not > thr_out
    auto pass = [&](const bool sweep) {
      auto sel = [&](const float w) {
        const unsigned o = ord_f32(w);
        if constexpr (Tagged) {
          if (w != w) return false;                           // a NaN word: no eligible row
        }
        return sweep ? (o > kappa && (all || !(w > thr_out))) : ((long long)o > lo && o <= kappa);
      };
      for (int64_t t0 = 0; t0 < gtiles; t0 += NT) {
        const float w = t0 + tid < gtiles ? words[(t0 + tid) * B + p] : inf;
        s_word[tid] = w;
        if (!__syncthreads_or(t0 + tid < gtiles && sel(w))) continue;   // (also the barrier between two rounds of words)
        const int nw = gtiles - t0 < NT ? (int)(gtiles - t0) : NT;
        for (int j = 0; j < nw; ++j) {
          if (!sel(s_word[j])) continue;
          ++ntiles;
          const int64_t g0 = (t0 + j) * WITHIN_BM;
          const int rows = G - g0 < WITHIN_BM ? (int)(G - g0) : WITHIN_BM;
          const unsigned long long kth = s_list[k - 1];       // the kept labels are distinct: a word that is not below it cannot enter
          bool any = false;
          for (int r = wave; r < rows; r += WITHIN_NW) {
            const long long lab = row_labels[g0 + r];
            if (lab < 0 || lab == ex) continue;               // not usable: never a candidate
            if constexpr (Tagged) {
              const TopkTags& tg = topk_tags(tagargs...);   // (the probe's mask: a uniform load)
              if ((tg.row_tags[g0 + r] & tg.probe_masks[p]) == 0) continue;   // not eligible: not usable
            }
            float d;
            (void)ref_distance(plan, scratch[wave], q, gallery + (g0 + r) * D, metric, lane, &d, clamp != 0);
            if (d == d) {                                     // a NaN distance is never listed
              const unsigned long long cand = ((unsigned long long)ord_f32(d) << 32) | (unsigned)(g0 + r);
              if (cand < kth) {
                if (lane == 0) {
                  s_list[TOPK_MAX + r] = cand;
                  s_lab[TOPK_MAX + r] = lab;
                }
                any = true;
              }
            }
          }
          if (!__syncthreads_or(any)) continue;
          // one entry per label: an entry that finds a smaller word of its own label is struck out.  The kept ones differ
          // among themselves already, so they look at the tile's candidates only; broadcast reads, words are unique
          bool dead = false;
          if (tid < 2 * TOPK_MAX) {
            const unsigned long long my = s_list[tid];
            if (my != TOPK_NONE) {
              const long long mylab = s_lab[tid];
              if (tid >= TOPK_MAX)
                for (int i = 0; i < k; ++i)
                  if (s_lab[i] == mylab && s_list[i] < my) dead = true;
              for (int i = TOPK_MAX; i < TOPK_MAX + rows; ++i)
                if (s_lab[i] == mylab && s_list[i] < my) dead = true;
            }
          }
          __syncthreads();
          if (dead) {
            s_list[tid] = TOPK_NONE;
            s_lab[tid] = TOPK_NOLABEL;
          }
          __syncthreads();
          // bitonic sort of the 2 * TOPK_MAX words, ascending, the labels with them; empty slots are above every candidate
          for (int k2 = 2; k2 <= 2 * TOPK_MAX; k2 <<= 1) {
            for (int h = k2 >> 1; h > 0; h >>= 1) {
              if (tid < TOPK_MAX) {
                const int i = ((tid & ~(h - 1)) << 1) | (tid & (h - 1)), l = i | h;
                const unsigned long long a = s_list[i], b = s_list[l];
                if ((a > b) == ((i & k2) == 0)) {
                  const long long la = s_lab[i], lb = s_lab[l];
                  s_list[i] = b;
                  s_list[l] = a;
                  s_lab[i] = lb;
                  s_lab[l] = la;
                }
              }
              __syncthreads();
            }
          }
          if (tid >= k && tid < 2 * TOPK_MAX) {               // keep the smallest k
            s_list[tid] = TOPK_NONE;
            s_lab[tid] = TOPK_NOLABEL;
          }
          __syncthreads();
        }
        __syncthreads();                                      // s_word is rewritten by the next round
      }
    };

    bool sweep = false;
#pragma unroll 1
    for (;;) {                                                // the seed passes, then the sweep: one call site of `pass`
      if (!sweep) kappa = (int64_t)sd < gtiles ? topk_kappa(words, B, p, gtiles, (unsigned)sd, s_hist, s_sel) : ~0u;
      pass(sweep);
      if (sweep || kappa == ~0u) break;                       // ~0u: every tile is evaluated (no word has a NaN's image)
      const unsigned long long kth = s_list[k - 1];
      const float t = kth == TOPK_NONE ? inf : unord_f32((unsigned)(kth >> 32));
      const Band b = within_band(metric, t, s, D, cdot, sqmax_bits);
      all = b.odd;
      thr_out = b.T + b.E;
      int left = 0;                                           // the tiles the sweep would evaluate at this tolerance
      for (int64_t t0 = 0; t0 < gtiles; t0 += NT) {
        bool mine = false;
        if (t0 + tid < gtiles) {
          const float w = words[(t0 + tid) * B + p];
          mine = ord_f32(w) > kappa && (all || !(w > thr_out));
          if constexpr (Tagged) mine = mine && w == w;
        }
        left += __syncthreads_count(mine);
      }
      if (left <= sd) {
        sweep = true;
      } else {
        lo = kappa;
        sd *= 2;                                              // (sd < gtiles < 2^24 here)
      }
    }
  }

  if (tid < k) {
    const unsigned long long w = s_list[tid];
    idx_out[(int64_t)p * k + tid] = w == TOPK_NONE ? -1 : (int64_t)(unsigned)w + index_base;
    dist_out[(int64_t)p * k + tid] = w == TOPK_NONE ? __builtin_nanf("") : unord_f32((unsigned)(w >> 32));
    if (label_out) label_out[(int64_t)p * k + tid] = w == TOPK_NONE ? -1 : (int64_t)s_lab[tid];
  }
  if (tid == 0 && ntiles) atomicAdd(tiles_stat, (unsigned long long)ntiles);
  if constexpr (Tagged) {
    if (tid == 0 && ntiles) atomicAdd(topk_tags(tagargs...).tiles_stat, (unsigned long long)ntiles);
  }
}

// row_tags null: dif_match_topk_ids; else dif_match_topk_ids_tagged (probe_masks [B])
int topk_ids_run(Gallery* g, const float* probes, int B, int metric, int k, const int64_t* row_labels, const int64_t* exclude,
                 int64_t* idx_out, float* dist_out, int64_t* label_out, hipStream_t st, const int64_t* row_tags,
                 const int64_t* probe_masks) {
  if (B <= 0) return 0;
  const bool tagged = row_tags != nullptr;
  if (tagged && tagged_stat_reset(g, st)) return -1;
  SumPlan plan;
  if (make_sum_plan(g->d, &plan)) return -1;
  const int clamp = g->clamp_nan ? 1 : 0;
  const int seed = g->topk_seed > 0 ? g->topk_seed : k;
  const int64_t gtiles = (g->n + WITHIN_BM - 1) / WITHIN_BM;
  Rounds rounds;
  if (topk_plan(g, B, gtiles, st, &rounds)) return -1;
  if (!g->topk_ids_stat) DIF_HIP(hipMalloc(&g->topk_ids_stat, sizeof(unsigned long long)));
  DIF_HIP(hipMemsetAsync(g->topk_ids_stat, 0, sizeof(unsigned long long), st));
  const float cdot = g->d * U24;                              // the f32 MFMA: a D-term fma chain
  return for_rounds(rounds, 0, B, [&](int64_t b0, int nb) {
    const float* pr = probes + b0 * g->d;
    const int64_t* pm = tagged ? probe_masks + b0 : nullptr;
    if (gtiles > 0 && tilemin_pass(g, pr, nb, metric, st, row_tags, pm)) return -1;
    if (tagged)
      hipLaunchKernelGGL((topk_ids_select_kernel<true, TopkTags>), dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->topk_min, g->n, nb, pr,
                         g->rows, g->d, metric, cdot, g->sqmax_bits, clamp, plan, k, seed, g->index_base, row_labels,
                         exclude ? exclude + b0 : nullptr, idx_out + b0 * k, dist_out + b0 * k,
                         label_out ? label_out + b0 * k : nullptr, g->topk_ids_stat,
                         TopkTags{row_tags, pm, g->topk_tagged_stat});
    else
      hipLaunchKernelGGL((topk_ids_select_kernel<false>), dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->topk_min, g->n, nb, pr,
                         g->rows, g->d, metric, cdot, g->sqmax_bits, clamp, plan, k, seed, g->index_base, row_labels,
                         exclude ? exclude + b0 : nullptr, idx_out + b0 * k, dist_out + b0 * k,
                         label_out ? label_out + b0 * k : nullptr, g->topk_ids_stat);
    DIF_HIP(hipGetLastError());
    return 0;
  });
}

// ---------------------------------------------------------------------------------------------
// Which enrolled rows are the same person (dif_gallery_cluster): the connected components of the graph on the gallery's rows
// whose edges are the pairs within the tolerance -- exact single-linkage clustering.  With the rows themselves as probes:
//   for i in range(G):  d = distance(rows[i][None, :], rows[:i + 1], metric);  for j in np.flatnonzero(d <= t): unite(i, j)
//   label[i] = index_base + min(rows of i's component);  n_clusters = number of components
// The range search with a self-join driver and a resolve stage that unites instead of listing; nothing of size G x G is kept:
//   cluster_init_kernel     parent[i] = i, or the earlier label of the incremental form (checked: it is an index into parent)
//   per round of probes [p0, p1), whole 128-probe blocks:
//     within_prep_kernel    unchanged, on the gallery's own rows
//     within_census_kernel  unchanged, over gallery rows [0, p1) only: probe i needs rows j <= i -- the lower triangle, half
//                           the MFMA work of running every row as a probe of dif_match_within
//     cluster_resolve_kernel  one block per probe i walks its words in ascending tile order up to i's own tile.  A census
//                           word holds counts, not row numbers, so every tile with a sure OR a borderline row is evaluated
//                           row by row with ref_distance, a wave per row j < i (the self hit changes nothing), and on
//                           dist <= t lane 0 calls cl_unite(i, j).  A probe outside the bound's validity resolves every tile.
//   cluster_flatten_kernel  label[i] = index_base + cl_find(i), read-only; n_clusters = number of i with cl_find(i) == i, one
//                           integer atomicAdd per block.
// The union-find.  parent[x] <= x always; x is a root iff parent[x] == x.  cl_unite(i, j) finds both roots and hooks the
// LARGER under the smaller by atomicCAS(&parent[hi], hi, lo), retrying from the finds when the CAS fails (hi was hooked by
// someone else meanwhile).  Facts, each by induction over the successful writes:
//   (a) no cycles: every write to parent[x] stores a value below x -- the CAS stores lo < hi; path halving stores the parent of
//       x's parent, which is below x because x was seen not to be a root -- so a walk along parent strictly descends and ends.
//   (b) a row that has stopped being a root never becomes one again: only the CAS writes to a root, it expects parent[hi] == hi,
//       and by (a) no later write restores that.  So a path-halving store can never undo a hook, and it only ever stores an
//       ancestor of x, i.e. a row of x's own component.
//   (c) the root of a component is its smallest row: true for singletons; a hook puts a root hi, the minimum of its tree, under
//       lo < hi, whose tree's root is (still, or by now) an even smaller row.
// Every edge found is united, trees only merge, and when the last round has ended two rows share a root iff a chain of edges
// joins them.  By (c) that root is the component's minimum, whatever the order the edges arrived in, whichever thread won
// which CAS: the labels are a function of the edge SET, and the edge set is decided by ref_distance alone.  Hence two calls,
// or a different round size, give identical arrays.  (The incremental form starts from the labels of rows [0, r): those trees
// have the components of the earlier call and the same roots, and probes >= r add exactly the edges the full call adds after
// its probe r - 1.)
// Memory.  The eight XCDs do not share an L2, so a plain cached load of parent may stay stale for a whole kernel.  A stale
// value is a former parent, still an ancestor by (b): correctness does not need fresh loads.  Termination of the retry loop
// does: a CAS fails because parent[hi] changed, and the next cl_find must see that change to make progress.  So cl_find reads
// through agent-scope atomic loads, the halving store is an agent-scope atomic store, and the CAS is HIP's atomicCAS: plain
// HIP C++, vector global atomics.  Kernel boundaries order the rounds.
__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool HALVE>
__device__ __forceinline__ int cl_find(int* __restrict__ parent, int x) {
  for (;;) {
    const int p = cl_load(parent + x);
    if (p == x) return x;
    const int gp = cl_load(parent + p);
    if (gp == p) return p;
    if (HALVE) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
}

__device__ __forceinline__ void cl_unite(int* __restrict__ parent, int a, int b) {
  for (;;) {
    a = cl_find<true>(parent, a);
    b = cl_find<true>(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
  }
}

__global__ __launch_bounds__(256) void cluster_init_kernel(int* __restrict__ parent, int64_t G, int64_t first_row,
                                                           const int64_t* __restrict__ labels_in, int64_t index_base,
                                                           int* __restrict__ bad, int64_t* __restrict__ n_clusters) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *n_clusters = 0;
  if (i >= G) return;
  int64_t v = i;
  if (i < first_row) {
    // (unsigned: one comparison covers both sides and cannot overflow, as in rank_prep_kernel)
    const uint64_t l = (uint64_t)labels_in[i] - (uint64_t)index_base;
    if (l <= (uint64_t)i) {
      v = (int64_t)l;
    } else {
      *bad = 1;                                               // (identical stores; the row stays a singleton: parent stays in bounds)
    }
  }
  parent[i] = (int)v;
}

// The walk of the self-join (cluster, DBSCAN): probe i's census words in ascending tile order up to i's own tile; every tile
// with a sure or a borderline row -- a census word holds counts, not row numbers -- (every tile for a probe outside the bound's
// validity) is evaluated row by row, a wave per row j < i, and lane 0 of that wave calls edge(j, d) where d <= t.
// Block-uniform control flow; a wave owns its rows.
template <class F>
__device__ __forceinline__ void edge_walk(const unsigned short* __restrict__ census, int B, const f32x4* __restrict__ thr,
                                          const float* __restrict__ gallery, int64_t i, int D, int metric, float t, int clamp,
                                          const SumPlan& plan, float (*scratch)[NP_SCRATCH], unsigned short* s_word, F&& edge) {
  const int p = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* q = gallery + i * D;
  const bool all = thr[p][3] != 0.f;
  auto sel = [&](unsigned short w) { return all || w != 0; };
  walk_words(census, B, p, i / WITHIN_BM + 1, s_word, sel, [&](int64_t tl, unsigned short w) {
    if (!sel(w)) return;
    const int64_t g0 = tl * WITHIN_BM;
    const int rows = i - g0 < WITHIN_BM ? (int)(i - g0) : WITHIN_BM;   // rows j < i only: no self pair
    for (int r = wave; r < rows; r += WITHIN_NW) {
      float d;
      (void)ref_distance(plan, scratch[wave], q, gallery + (g0 + r) * D, metric, lane, &d, clamp != 0);
      if (lane == 0 && d <= t) edge((int)(g0 + r), d);        // NaN: not an edge
    }
  });
}

// One block per probe i = p0 + blockIdx.x; `census` rows are B words apart and cover tiles 0 .. (p0 + B - 1) / 128.
__global__ __launch_bounds__(64 * WITHIN_NW) void cluster_resolve_kernel(const unsigned short* __restrict__ census, int B,
                                                                       const f32x4* __restrict__ thr,
                                                                       const float* __restrict__ gallery, int64_t p0,
                                                                       int64_t first_row, int D, int metric, float t,
                                                                       int clamp, const SumPlan plan,
                                                                       int* __restrict__ parent) {
  __shared__ float scratch[WITHIN_NW][NP_SCRATCH];
  __shared__ unsigned short s_word[64 * WITHIN_NW];
  const int64_t i = p0 + blockIdx.x;
  if (i < first_row) return;                                  // (block-uniform) a row the earlier labels already cover
  edge_walk(census, B, thr, gallery, i, D, metric, t, clamp, plan, scratch, s_word,
            [&](int j, float) { cl_unite(parent, (int)i, j); });
}

__global__ __launch_bounds__(256) void cluster_flatten_kernel(int* __restrict__ parent, int64_t G, int64_t index_base,
                                                              const int* __restrict__ bad, int64_t* __restrict__ labels_out,
                                                              int64_t* __restrict__ n_clusters) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int root = -1;
  if (i < G) {
    root = cl_find<false>(parent, (int)i);
    labels_out[i] = index_base + root;
  }
  const int roots = __syncthreads_count(i < G && root == (int)i);
  if (threadIdx.x != 0) return;
  if (*bad) {                                                 // a labels_in entry that no earlier call can have produced
    if (blockIdx.x == 0) *n_clusters = -1;
  } else if (roots) {
    atomicAdd(reinterpret_cast<unsigned long long*>(n_clusters), (unsigned long long)roots);   // integer: order-free
  }
}

// Rows per round of the self-join ("cluster_round"; dif_gallery_cluster and dif_gallery_dbscan): at most what the census cap
// allows.  A round's census covers rows [0, its last probe], so R equal rounds do (R + 1) / 2R of the square's MFMA work: one
// round would do all of it.  The default is a sixteenth of the rows (17 / 32 of the square), never below 2048 probes (a
// launch that fills the chip).  ... and the census workspace for one such round, grown in one `ensure` with whatever else the
// caller needs (`more`)
template <class... W>
static int selfjoin_plan(Gallery* g, int64_t gtiles, hipStream_t st, Rounds* rounds, W... more) {
  int64_t want = g->cluster_round;
  if (want <= 0) {
    want = ((g->n + 15) / 16 + 127) / 128 * 128;
    if (want < 2048) want = 2048;
  }
  *rounds = plan_rounds(gtiles, g->n, WITHIN_CENSUS_MAX, want, 1);
  return ensure(st, workspace(&g->within_census, &g->within_census_cap, (size_t)gtiles * (size_t)rounds->per, sizeof(unsigned short)),
                workspace(&g->within_thr, &g->within_thr_cap, (size_t)rounds->per, 4 * sizeof(float)), more...);
}
// the thresholds and the census of one round [b0, b0 + nb): the triangle -- no probe of the round looks past its last row
static int selfjoin_census(Gallery* g, int64_t b0, int nb, int metric, float tolerance, hipStream_t st) {
  const float* pr = g->rows + b0 * g->d;
  hipLaunchKernelGGL(within_prep_kernel, dim3((nb + 3) / 4), dim3(256), 0, st, pr, nb, g->d, metric, tolerance, g->d * U24,
                     g->sqmax_bits, reinterpret_cast<f32x4*>(g->within_thr));   // (g->d * U24: the f32 MFMA, a D-term fma chain)
  DIF_HIP(hipGetLastError());
  return census_pass(g, pr, nb, metric, st, b0 + nb);
}

int cluster_run(Gallery* g, int metric, float tolerance, int64_t first_row, const int64_t* labels_in, int64_t* labels_out,
                int64_t* n_clusters, hipStream_t st) {
  const int64_t n = g->n;
  if (n <= 0) {
    DIF_HIP(hipMemsetAsync(n_clusters, 0, sizeof(int64_t), st));
    return 0;
  }
  SumPlan plan;
  if (make_sum_plan(g->d, &plan)) return -1;
  const int clamp = g->clamp_nan ? 1 : 0;
  Rounds rounds;
  if (selfjoin_plan(g, (n + WITHIN_BM - 1) / WITHIN_BM, st, &rounds,
                    workspace(&g->cluster_parent, &g->cluster_parent_cap, (size_t)n, sizeof(int))))
    return -1;
  if (!g->cluster_bad) DIF_HIP(hipMalloc(&g->cluster_bad, sizeof(int)));
  DIF_HIP(hipMemsetAsync(g->cluster_bad, 0, sizeof(int), st));
  const unsigned nblk = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(cluster_init_kernel, dim3(nblk), dim3(256), 0, st, g->cluster_parent, n, first_row, labels_in,
                     g->index_base, g->cluster_bad, n_clusters);
  DIF_HIP(hipGetLastError());
  const int rc = for_rounds(rounds, first_row / 128 * 128, first_row < n ? n : 0, [&](int64_t b0, int nb) {
    if (selfjoin_census(g, b0, nb, metric, tolerance, st)) return -1;
    hipLaunchKernelGGL(cluster_resolve_kernel, dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->within_census, nb,
                       reinterpret_cast<const f32x4*>(g->within_thr), g->rows, b0, first_row, g->d, metric, tolerance, clamp,
                       plan, g->cluster_parent);
    DIF_HIP(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(cluster_flatten_kernel, dim3(nblk), dim3(256), 0, st, g->cluster_parent, n, g->index_base, g->cluster_bad,
                     labels_out, n_clusters);
  DIF_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Density clustering with noise (dif_gallery_dbscan): DBSCAN on the edge set of dif_gallery_cluster.
//   E = {(i, j): j < i and distance(rows[i][None, :], rows[j][None, :], metric) <= t}      row i is the probe; no self pairs
//   degree[i] = 1 + edges of E that contain i;  core[i] = degree[i] >= min_samples
//   clusters  = connected components of (core rows, edges of E between two core rows);  label = index_base + smallest row
//   a non-core row with a core neighbour takes the label of the NEAREST one (the edge's float32 value, ties to the lower row)
//   every other row is noise: label -1
// Two sweeps of the lower triangle in cluster_run's rounds; every edge is seen exactly once per sweep, by its probe i:
//   dbscan_init_kernel     parent[i] = i, degree[i] = 1, anchor[i] = ~0, counts = {0, 0}
//   degree sweep, per round: within_prep_kernel, within_census_kernel (both unchanged), dbscan_degree_kernel: the walk of
//                          cluster_resolve_kernel; an edge adds 1 to degree[i] (summed per wave first) and to degree[j]
//   link sweep, per round: the census again (kept when one round covers the gallery: same probes, same thresholds), then
//                          dbscan_link_kernel: the same walk, the same ref_distance values, and per edge
//                            both ends core         cl_unite(i, j)
//                            one end core (c), b    atomicMin(&anchor[b], float_bits(d) << 32 | c)
//                            neither                nothing
//   dbscan_flatten_kernel  core: index_base + cl_find(i); anchored: index_base + cl_find(anchor & 0xffffffff); else -1;
//                          counts[0] = core rows that are roots, counts[1] = noise rows: one integer atomicAdd per block each
// Why the result is a function of the edge set alone.  degree is a sum of integer atomicAdds: order-free, and complete when
// the degree sweep's last kernel has ended, which is before the first link kernel reads it (one stream).  So `core` is fixed
// throughout the link sweep.  Unions happen among core rows only, parent[x] <= x still holds, and facts (a)-(c) above carry
// over word for word: a core row's root is the smallest row of its core component.  A non-core row is never hooked and never
// a hook's target: it stays its own root and no core row's path passes through it.  anchor[b] is the minimum over a SET of
// 64-bit words, one per (edge, core end): a minimum does not depend on the order its operands arrive in, nor on which thread
// brings them.  Both metrics only give distances >= +0 (a pairwise sum of squares; acos(.) / pi), so the float's bit pattern
// orders like its value and the word orders by (distance, row): the nearest core neighbour, exact ties to the lower row.
// d is ref_distance's value, the same bits in both sweeps (the same operands in the same order).  min_samples = 1 makes every
// row core: the labels are dif_gallery_cluster's and nothing is noise.
constexpr unsigned long long DBSCAN_NONE = ~0ull;             // no core neighbour: above every anchor word (a row is < 2^31)

__global__ __launch_bounds__(256) void dbscan_init_kernel(int* __restrict__ parent, int* __restrict__ degree,
                                                          unsigned long long* __restrict__ anchor, int64_t G,
                                                          int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < 2) counts[i] = 0;
  if (i >= G) return;
  parent[i] = (int)i;
  degree[i] = 1;                                              // the row itself, whatever distance(i, i) evaluates to
  anchor[i] = DBSCAN_NONE;
}

// One block per probe i = p0 + blockIdx.x; `census` rows are B words apart and cover tiles 0 .. (p0 + B - 1) / 128.
__global__ __launch_bounds__(64 * WITHIN_NW) void dbscan_degree_kernel(const unsigned short* __restrict__ census, int B,
                                                                     const f32x4* __restrict__ thr,
                                                                     const float* __restrict__ gallery, int64_t p0, int D,
                                                                     int metric, float t, int clamp, const SumPlan plan,
                                                                     int* __restrict__ degree) {
  __shared__ float scratch[WITHIN_NW][NP_SCRATCH];
  __shared__ unsigned short s_word[64 * WITHIN_NW];
  const int64_t i = p0 + blockIdx.x;
  int mine = 0;                                               // lane 0: edges this wave found for probe i
  edge_walk(census, B, thr, gallery, i, D, metric, t, clamp, plan, scratch, s_word, [&](int j, float) {
    ++mine;
    atomicAdd(degree + j, 1);                                 // integer: order-free
  });
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(degree + i, mine);
}

__global__ __launch_bounds__(64 * WITHIN_NW) void dbscan_link_kernel(const unsigned short* __restrict__ census, int B,
                                                                   const f32x4* __restrict__ thr,
                                                                   const float* __restrict__ gallery, int64_t p0, int D,
                                                                   int metric, float t, int clamp, const SumPlan plan,
                                                                   int min_samples, const int* __restrict__ degree,
                                                                   int* __restrict__ parent,
                                                                   unsigned long long* __restrict__ anchor) {
  __shared__ float scratch[WITHIN_NW][NP_SCRATCH];
  __shared__ unsigned short s_word[64 * WITHIN_NW];
  const int64_t i = p0 + blockIdx.x;
  const bool core_i = degree[i] >= min_samples;               // (final: the degree sweep ended before this kernel began)
  unsigned long long best = DBSCAN_NONE;                      // lane 0: the nearest core row this wave found for a non-core i
  edge_walk(census, B, thr, gallery, i, D, metric, t, clamp, plan, scratch, s_word, [&](int j, float d) {
    const bool core_j = degree[j] >= min_samples;
    const unsigned long long hi = (unsigned long long)__builtin_bit_cast(unsigned, d) << 32;   // d >= +0: ordered like d
    if (core_i && core_j) {
      cl_unite(parent, (int)i, j);
    } else if (core_i) {
      atomicMin(anchor + j, hi | (unsigned)i);                // a minimum over a set: order-free
    } else if (core_j) {
      const unsigned long long w = hi | (unsigned)j;
      best = w < best ? w : best;
    }
  });
  if ((threadIdx.x & 63) == 0 && best != DBSCAN_NONE) atomicMin(anchor + i, best);
}

__global__ __launch_bounds__(256) void dbscan_flatten_kernel(int* __restrict__ parent, const int* __restrict__ degree,
                                                             const unsigned long long* __restrict__ anchor, int64_t G,
                                                             int min_samples, int64_t index_base,
                                                             int64_t* __restrict__ labels_out, int* __restrict__ degree_out,
                                                             int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool is_root = false, is_noise = false;
  if (i < G) {
    const int deg = degree[i];
    const unsigned long long a = anchor[i];
    int64_t label = -1;                                       // noise, whatever index_base is
    if (deg >= min_samples) {
      const int root = cl_find<false>(parent, (int)i);
      is_root = root == (int)i;
      label = index_base + root;
    } else if (a != DBSCAN_NONE) {
      label = index_base + cl_find<false>(parent, (int)(a & 0xffffffffull));
    } else {
      is_noise = true;
    }
    labels_out[i] = label;
    if (degree_out) degree_out[i] = deg;
  }
  const int roots = __syncthreads_count(is_root), noise = __syncthreads_count(is_noise);
  if (threadIdx.x != 0) return;
  if (roots) atomicAdd(reinterpret_cast<unsigned long long*>(counts), (unsigned long long)roots);       // integer: order-free
  if (noise) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 1), (unsigned long long)noise);
}

int dbscan_run(Gallery* g, int metric, float tolerance, int min_samples, int64_t* labels_out, int* degree_out, int64_t* counts,
               hipStream_t st) {
  const int64_t n = g->n;
  if (n <= 0) {
    DIF_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    return 0;
  }
  SumPlan plan;
  if (make_sum_plan(g->d, &plan)) return -1;
  const int clamp = g->clamp_nan ? 1 : 0;
  Rounds rounds;
  if (selfjoin_plan(g, (n + WITHIN_BM - 1) / WITHIN_BM, st, &rounds,
                    workspace(&g->cluster_parent, &g->cluster_parent_cap, (size_t)n, sizeof(int)),
                    workspace(&g->dbscan_degree, &g->dbscan_degree_cap, (size_t)n, sizeof(int)),
                    workspace(&g->dbscan_anchor, &g->dbscan_anchor_cap, (size_t)n, sizeof(unsigned long long))))
    return -1;
  const unsigned nblk = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(dbscan_init_kernel, dim3(nblk), dim3(256), 0, st, g->cluster_parent, g->dbscan_degree, g->dbscan_anchor, n,
                     counts);
  DIF_HIP(hipGetLastError());
  const bool one_round = rounds.per >= n;
  for (int link = 0; link < 2; ++link) {
    const int rc = for_rounds(rounds, 0, n, [&](int64_t b0, int nb) {
      // (one round: the degree sweep's census is the link sweep's)
      if (!(link && one_round) && selfjoin_census(g, b0, nb, metric, tolerance, st)) return -1;
      if (!link) {
        hipLaunchKernelGGL(dbscan_degree_kernel, dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->within_census, nb,
                           reinterpret_cast<const f32x4*>(g->within_thr), g->rows, b0, g->d, metric, tolerance, clamp, plan,
                           g->dbscan_degree);
      } else {
        hipLaunchKernelGGL(dbscan_link_kernel, dim3(nb), dim3(64 * WITHIN_NW), 0, st, g->within_census, nb,
                           reinterpret_cast<const f32x4*>(g->within_thr), g->rows, b0, g->d, metric, tolerance, clamp, plan,
                           min_samples, g->dbscan_degree, g->cluster_parent, g->dbscan_anchor);
      }
      DIF_HIP(hipGetLastError());
      return 0;
    });
    if (rc) return rc;
  }
  hipLaunchKernelGGL(dbscan_flatten_kernel, dim3(nblk), dim3(256), 0, st, g->cluster_parent, g->dbscan_degree, g->dbscan_anchor,
                     n, min_samples, g->index_base, labels_out, degree_out, counts);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dif
