// All-pairs verification counts at every threshold, exact (dif_match_roc): how many genuine and how many impostor pairs of
// (probe, enrolled row) lie below each of T thresholds -- the numerators of TAR and FAR -- in ONE pass over the gallery.
// hipcc-flags: -ffp-contract=off
// (the resolve stage restates the reference's float32 operations one by one, as match_within.hip's does)
//
// Semantics, per call (include/dif.h has the contract; the B x G distances are never materialised):
//   dist = distance(q[:, None], gallery[None, :], metric);  use = both labels >= 0 and row + index_base >= first_row[probe]
//   accept[j][0 | 1] = count(use, labels equal | different, dist < t[j])        strict; NaN < t is False
//   totals = count(use, equal), count(use, different), and of each those whose dist is NaN
// Every used pair is put into ONE bin,  bin(d) = number of thresholds <= d  in 0 .. T  (a NaN distance: a bin of its own,
// T + 1), so accept[j] is the sum of bins 0 .. j and the totals are sums of all of them.  Counts are integers from the first
// addition on: the result depends on no block or thread order.
//
//  1. roc_table_kernel  -- per threshold j two search edges, probe-independent:
//        metric 1 (similarity space, key / |q|):  c(t) = -cos(pi t) in double, rounded once; -inf for t < 0, +inf for t >= 1
//        metric 0 (key + |q|^2):                  c(t) = t
//     A[j] = c(t_j)  and  B[j] = c(t_j'),  t_j' = nextafterf(t_j, -inf):  dist < t_j  iff  dist <= t_j'  (rank_prep_kernel's
//     device for a strict comparison).  A is padded with +inf to P - 1 entries, P the power of two above T; B[T] = +inf.
//  2. roc_prep_kernel   -- per probe the scale (1 / |q|, or |q|^2), the half width e of the band in that space, and H.
//  3. roc_census_kernel -- a sibling of key_tiles (key_tiles.hpp): the same tiles, the same f32 MFMA main loop on the rows
//     themselves, the same XCD-aware block order, the same key.  One pass whatever T is.  The epilogue normalises each key,
//        kn = key / |q|  (metric 1)     kn = key + |q|^2  (metric 0)
//     finds  b = number of j with A[j] < kn - e  by a branch-free binary search of log2 P LDS reads, and calls the pair
//        SURE in bin b   when  kn + e <= B[b]  and  |key| < H
//        BORDERLINE      otherwise (a NaN key, a probe outside the bound's validity: H = -inf)
//     Why SURE is sure: A[b - 1] < kn - e gives key > T(t_{b-1}) + E, so dist > t_{b-1} (within_band's OUT), hence every
//     threshold below b is <= dist; kn + e <= B[b] with |key| < H gives key <= T(t_b') - E, so dist <= t_b' < t_b
//     (within_band's SURE), hence every threshold from b on is above dist -- the thresholds are sorted, and the argument runs
//     on the exact edges, which are monotone, so the table need not be.  e is within_band's E, untouched, divided by |q| for
//     metric 1, plus what the normalisation adds:
//        metric 1:  + 6 u  -- fl(1 / sqrtf(s)) (1.5 u), the product key * that (u; |kn| <= 1.001), sqrtf against the double
//                   sqrt of within_band's T (u), the table entry rounded once (u) and cos's own 1e-16: 4.6 u in all
//        metric 0:  + 2 u ((|q| + gmax)^2 + |q|^2)  -- the one rounding of key + |q|^2, |key| <= (|q| + gmax)^2; the table
//                   holds t_j itself, so the u (|t| + |q|^2) that within_band spends on fl(t - |q|^2) is spare
//     A SURE pair goes to a per-block histogram in LDS ([T + 1][2] words, ds_add_u32); a BORDERLINE pair sets its bit in
//     a 128-bit row mask per (gallery tile, probe), written by every block for every word it owns: no list, no overflow
//     path, no atomics on global memory for it.  The labels and first_row are applied here: a skipped pair is in no bin, no
//     mask, no total.
//     LDS: the histogram and the two tables (up to 20.5 KB at T = 1024) do not fit beside the main loop's 72 KB at two blocks
//     per CU, so they ALIAS it: gemm_mainloop ends on a barrier and leaves LDS free.  Each tile re-reads the tables (12 KB
//     from L2 against the 256 KB of rows it streams) and zeroes the histogram; after the epilogue thread i adds words
//     i, i + 256, ... to registers of its own (9 of them), and the block flushes those once, at its end, with 64-bit integer
//     atomics on global memory.  Atomics rather than a slab per block and a reduce kernel: a block adds only the bins it
//     met -- a few dozen of 2050 -- where a slab would write and re-read every bin of every block, and integer addition
//     commutes, so nothing about the result depends on the order.
//  4. roc_resolve_kernel -- scans the masks; for every set bit one wave evaluates that pair with ref_distance and bins the
//     distance against the float32 thresholds themselves (dist < t_j exactly as stated).  Per-block histogram in LDS, the
//     same flush.  Exactly the flagged pairs are evaluated, not their 128-row tiles.  A block takes ROC_CHUNK masks per trip
//     ("roc_blocks" caps the grid; tests force many trips); the queue's two counters are used in turn.
//  5. roc_finish_kernel -- prefix sums of the bins -> accept, totals.
#include "key_tiles.hpp"

namespace dif {

constexpr int ROC_MAX_T = 1024;                               // DIF_ROC_MAX_THRESHOLDS
constexpr int ROC_TAB = 2048;                                 // floats per table in global memory: P <= 2048
constexpr int ROC_BINS = 2 * (ROC_MAX_T + 2);                 // 64-bit words of the call's bins: [T + 2][equal | different]; one more
                                                              // word behind them counts the pairs the resolve stage evaluated
constexpr int ROC_NT = 256;                                   // threads of a census block, whatever the tile shape
constexpr int ROC_NREG = (2 * (ROC_MAX_T + 1) + ROC_NT - 1) / ROC_NT;   // histogram words a census thread keeps in registers
constexpr size_t ROC_MASK_MAX = (size_t)16 << 20;             // masks (16 bytes each) per launch (256 MB); more probes go in rounds
constexpr int ROC_CHUNK = 64 * WITHIN_NW;                     // masks a resolve block looks at per step
constexpr int64_t ROC_BLOCK_TILES = 131072;                   // tiles a census block may walk: its 32-bit counters stay below 2^31 (16384 pairs a tile)

__device__ __forceinline__ float roc_edge(int metric, float t) {
  if (metric != 1) return t;
  const float inf = __builtin_inff();
  return t >= 1.f ? inf : (t < 0.f ? -inf : (float)(-cos(3.14159265358979323846 * (double)t)));
}

__global__ __launch_bounds__(256) void roc_table_kernel(const float* __restrict__ thresholds, int nT, int metric,
                                                        float* __restrict__ tab, unsigned long long* __restrict__ bins) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j <= ROC_BINS) bins[j] = 0ull;
  if (j >= ROC_TAB) return;
  const float inf = __builtin_inff();
  float a = inf, b = inf;
  if (j < nT) {
    const float t = thresholds[j];
    a = roc_edge(metric, t);
    b = roc_edge(metric, nextafterf(t, -inf));
  }
  tab[j] = a;
  tab[ROC_TAB + j] = b;
}

// per probe: {scale, e, H, -}; a probe outside the bound's validity gets H = -inf: none of its pairs is SURE
__global__ __launch_bounds__(256) void roc_prep_kernel(const float* __restrict__ probes, int B, int D, int metric, float cdot,
                                                       const unsigned* __restrict__ sqmax_bits, f32x4* __restrict__ thr) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= B) return;
  const float s = probe_sq(probes + (int64_t)p * D, D, lane);
  if (lane != 0) return;
  const float inf = __builtin_inff(), u = U24;
  const Band b = within_band(metric, 0.f, s, D, cdot, sqmax_bits);   // E and H do not depend on the tolerance
  f32x4 v;
  if (metric == 1) {
    const float rq = 1.f / sqrtf(s);
    v = f32x4{rq, b.E * rq + 6.f * u, b.H, 0.f};
  } else {
    const float qn = sqrtf(s) * 1.0001f, gmax = sqrtf(__builtin_bit_cast(float, *sqmax_bits)) * 1.0001f;
    v = f32x4{s, b.E + 2.f * u * ((qn + gmax) * (qn + gmax) + qn * qn), inf, 0.f};
  }
  if (b.odd) v[2] = -inf;
  thr[p] = v;
}

template <class T>
__global__ __launch_bounds__(T::NT, 2) void roc_census_kernel(const float* __restrict__ gallery, int64_t G,
                                                            const float* __restrict__ probes, int B, int D,
                                                            const float* __restrict__ aux, int metric, int nparts,
                                                            const f32x4* __restrict__ thr, const float* __restrict__ tab,
                                                            int nT, int P, const int64_t* __restrict__ probe_labels,
                                                            const int64_t* __restrict__ row_labels,
                                                            const int64_t* __restrict__ first_row, int64_t index_base,
                                                            unsigned* __restrict__ mask,
                                                            unsigned long long* __restrict__ bins) {
  constexpr int WM = T::WM, WN = T::WN;
  static_assert(T::BM == WITHIN_BM && T::WGM * WM == 4, "four 32-bit mask words per 128 gallery rows, one per wave row and m");
  static_assert(T::NT == ROC_NT, "the register copy of the histogram is laid out for 256 threads");
  static_assert(T::LDS_FLOATS >= ROC_TAB + (ROC_MAX_T + 1) + 2 * (ROC_MAX_T + 1), "the tables and the histogram alias the main loop's LDS");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TileBlock tb = tile_block((B + T::BN - 1) / T::BN);
  const int part = tb.part;
  if (part >= nparts) return;
  // valid between the main loop's last barrier and the next tile's first store only
  float* sA = smem;                                            // [P - 1] (+inf from T on)
  float* sB = smem + ROC_TAB;                                  // [T + 1]
  unsigned* sH = reinterpret_cast<unsigned*>(smem + ROC_TAB + ROC_MAX_T + 1);   // [T + 1][2]
  const int tid = threadIdx.x;
  const int wc = T::wave_col();
  const int p0 = tb.cblk * T::BN;
  const int ksteps = D / BK;
  const int64_t gtiles = (G + T::BM - 1) / T::BM;
  const int nhist = 2 * (nT + 1);

  float sc[WN], ee[WN], hk[WN];
  int64_t pl[WN];
  int fr[WN], col[WN];
#pragma unroll
  for (int n = 0; n < WN; ++n) {
    col[n] = (wc * WN + n) * 32 + (tid & 31);
    const bool live = p0 + col[n] < B;                        // (a column that pads the probe block: label -1, in no pair)
    const f32x4 v = live ? thr[p0 + col[n]] : f32x4{0.f, 0.f, 0.f, 0.f};
    sc[n] = v[0];
    ee[n] = v[1];
    hk[n] = v[2];
    pl[n] = live ? probe_labels[p0 + col[n]] : (int64_t)-1;
    // first_row counts global rows; as a local row it is clamped to [0, 2^31 - 1] (a shard holds fewer rows than that)
    int64_t f = 0;
    if (live && first_row) {
      const int64_t fg = first_row[p0 + col[n]];
      if (__builtin_sub_overflow(fg, index_base, &f)) f = fg < 0 ? 0 : 0x7fffffffLL;
    }
    fr[n] = f < 0 ? 0 : (f > 0x7fffffffLL ? 0x7fffffff : (int)f);
  }
  unsigned reg[ROC_NREG];
#pragma unroll
  for (int k = 0; k < ROC_NREG; ++k) reg[k] = 0u;

  for (int64_t gt = part; gt < gtiles; gt += nparts) {
    const int64_t g0 = gt * T::BM;
    f32x16 acc[WM][WN];
    zero_acc<T>(acc);
    RowLoader<T::NA, T::RP> al(gallery + g0 * D, G - g0, D);
    RowLoader<T::NB, T::RP> bl(probes + (int64_t)p0 * D, (int64_t)B - p0, D);
    gemm_mainloop<T>(al, bl, 0, ksteps, smem, acc);          // ends on a barrier: LDS is free

    for (int i = tid; i < P; i += ROC_NT) sA[i] = tab[i];
    for (int i = tid; i <= nT; i += ROC_NT) sB[i] = tab[ROC_TAB + i];
    for (int i = tid; i < nhist; i += ROC_NT) sH[i] = 0u;
    lds_barrier();

    // dots -> keys -> a bin or a mask bit per pair.  aux[g] = -1/|g| (metric 1) or |g|^2 (metric 0), NaN for the rows kept
    // out of the filter: a NaN key fails every comparison and is BORDERLINE.  Rows past G carry label -1: in no pair.
    int lane = tid & 63;
    asm volatile("" : "+v"(lane));                           // opaque per tile, as in key_tiles
    const int wr = T::wave_row();
    const int64_t rows_left = G - g0;
    const __amdgpu_buffer_rsrc_t arsrc = make_rsrc(aux + g0, (uint32_t)((rows_left < T::BM ? rows_left : T::BM) * 4));
#pragma unroll
    for (int m = 0; m < WM; ++m) {
      const int rbase = (wr * WM + m) * 32 + 4 * (lane >> 5);
      unsigned mw[WN];
#pragma unroll
      for (int n = 0; n < WN; ++n) mw[n] = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {                          // rows rbase + 8q .. +3 <-> registers 4q .. 4q+3
        const f32x4 ax = buf_load4(arsrc, (uint32_t)(rbase + 8 * q) * 4u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = rbase + 8 * q + j;
          const int64_t rl = r < rows_left ? row_labels[g0 + r] : (int64_t)-1;
          const int grow = (int)(g0 + r);
          const unsigned bit = 1u << (4 * (lane >> 5) + 8 * q + j);   // row r is bit r % 32 of word r / 32
#pragma unroll
          for (int n = 0; n < WN; ++n) {
            const float dot = acc[m][n][4 * q + j];
            const float key = (metric == 1) ? dot * ax[j] : fmaf(-2.f, dot, ax[j]);
            const float kn = (metric == 1) ? key * sc[n] : key + sc[n];
            const float x = kn - ee[n];
            int pos = 0;
            for (int step = P >> 1; step > 0; step >>= 1) pos += (sA[pos + step - 1] < x) ? step : 0;   // pos <= T: the padding is +inf
            const bool sure = kn + ee[n] <= sB[pos] && fabsf(key) < hk[n];
            if (rl >= 0 && pl[n] >= 0 && grow >= fr[n]) {
              if (sure) atomicAdd(&sH[2 * pos + (rl == pl[n] ? 0 : 1)], 1u);
              else mw[n] |= bit;
            }
          }
        }
      }
      // lanes l and l + 32 hold the two halves of one word of the same probe column; every word has one owner
#pragma unroll
      for (int n = 0; n < WN; ++n) {
        const unsigned w = mw[n] | (unsigned)__shfl_xor((int)mw[n], 32);
        if (lane < 32 && p0 + col[n] < B) mask[(gt * B + p0 + col[n]) * 4 + (wr * WM + m)] = w;
      }
    }
    lds_barrier();
#pragma unroll
    for (int k = 0; k < ROC_NREG; ++k) {
      const int i = tid + k * ROC_NT;
      if (i < nhist) reg[k] += sH[i];
    }
    lds_barrier();                                           // the next main loop writes over the tables
  }
#pragma unroll
  for (int k = 0; k < ROC_NREG; ++k) {
    const int i = tid + k * ROC_NT;
    if (i < nhist && reg[k]) atomicAdd(&bins[i], (unsigned long long)reg[k]);   // integer: order-free
  }
}

// Masks are [gallery tile][probe], four words each.  A block looks at ROC_CHUNK of them per step; the ones with a bit set
// are queued in LDS and taken a wave each, a pair at a time.  All that differs between two runs is the order of the queue,
// and the counts do not depend on it.
__global__ __launch_bounds__(ROC_CHUNK) void roc_resolve_kernel(const u32x4* __restrict__ mask, int64_t nmask, int B,
                                                              const float* __restrict__ probes,
                                                              const float* __restrict__ gallery, int D, int metric, int clamp,
                                                              const SumPlan plan, const float* __restrict__ thresholds, int nT,
                                                              const int64_t* __restrict__ probe_labels,
                                                              const int64_t* __restrict__ row_labels,
                                                              unsigned long long* __restrict__ bins) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];  // thresholds [T], then the histogram [T + 2][2]
  __shared__ float scratch[WITHIN_NW][NP_SCRATCH];
  __shared__ int s_list[ROC_CHUNK];
  __shared__ int s_n[2];                                       // the queue's length, of this trip and of the next
  __shared__ unsigned s_pairs;                                // pairs this block evaluated (dif_gallery_get_stat "roc_resolved")
  float* s_thr = dyn;
  unsigned* s_hist = reinterpret_cast<unsigned*>(dyn + nT);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nhist = 2 * (nT + 2);
  for (int i = tid; i < nT; i += ROC_CHUNK) s_thr[i] = thresholds[i];
  for (int i = tid; i < nhist; i += ROC_CHUNK) s_hist[i] = 0u;
  if (tid == 0) s_n[0] = s_n[1] = 0, s_pairs = 0u;
  __syncthreads();
  int par = 0;
  for (int64_t c0 = (int64_t)blockIdx.x * ROC_CHUNK; c0 < nmask; c0 += (int64_t)gridDim.x * ROC_CHUNK, par ^= 1) {
    const int64_t e = c0 + tid;
    bool any = false;
    if (e < nmask) {
      const u32x4 w = mask[e];
      any = (w[0] | w[1] | w[2] | w[3]) != 0u;
    }
    if (any) s_list[atomicAdd(&s_n[par], 1)] = tid;
    __syncthreads();
    const int nlist = s_n[par];
    // the other counter was last read behind the previous trip's first barrier, which every wave has left, and is added to
    // again only behind this trip's last barrier
    if (tid == 0) s_n[par ^ 1] = 0;
    for (int i = wave; i < nlist; i += WITHIN_NW) {            // (wave-uniform from here on)
      const int64_t ei = c0 + s_list[i];
      const int64_t gt = ei / B;
      const int p = (int)(ei - gt * B);
      const u32x4 w = mask[ei];
      const float* q = probes + (int64_t)p * D;
      const int64_t lp = probe_labels[p];
      if (lane == 0) atomicAdd(&s_pairs, (unsigned)(__popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3])));
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        unsigned bits = (unsigned)__builtin_amdgcn_readfirstlane((int)w[k]);
        while (bits) {
          const int b = __builtin_ctz(bits);
          bits &= bits - 1u;
          const int64_t row = gt * WITHIN_BM + k * 32 + b;
          float d;
          (void)ref_distance(plan, scratch[wave], q, gallery + row * D, metric, lane, &d, clamp != 0);
          int bin = nT + 1;                                   // NaN: the bin no threshold accepts
          if (d == d) {
            int lo = 0, n = nT;                               // bin = number of thresholds <= d
            while (n > 0) {
              const int half = n >> 1;
              if (s_thr[lo + half] <= d) {
                lo += half + 1;
                n -= half + 1;
              } else {
                n = half;
              }
            }
            bin = lo;
          }
          if (lane == 0) atomicAdd(&s_hist[2 * bin + (row_labels[row] == lp ? 0 : 1)], 1u);
        }
      }
    }
    __syncthreads();                                          // s_list is rewritten by the next trip
  }
  __syncthreads();
  // (a block's 32-bit counters: roc_run keeps a launch's pairs per block below 2^32)
  for (int i = tid; i < nhist; i += ROC_CHUNK)
    if (s_hist[i]) atomicAdd(&bins[i], (unsigned long long)s_hist[i]);   // integer: order-free
  if (tid == 0 && s_pairs) atomicAdd(&bins[ROC_BINS], (unsigned long long)s_pairs);
}

__global__ __launch_bounds__(256) void roc_finish_kernel(const unsigned long long* __restrict__ bins, int nT,
                                                         int64_t* __restrict__ accept, int64_t* __restrict__ totals) {
  __shared__ unsigned long long s_bin[ROC_BINS];
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * (nT + 2); i += 256) s_bin[i] = bins[i];
  __syncthreads();
  for (int i = tid; i < 2 * nT; i += 256) {                   // accept[j][c] = bins 0 .. j of column c
    const int j = i >> 1, c = i & 1;
    unsigned long long a = 0;
    for (int b = 0; b <= j; ++b) a += s_bin[2 * b + c];
    accept[i] = (int64_t)a;
  }
  if (tid < 2) {
    unsigned long long a = 0;
    for (int b = 0; b <= nT + 1; ++b) a += s_bin[2 * b + tid];
    totals[tid] = (int64_t)a;
    totals[2 + tid] = (int64_t)s_bin[2 * (nT + 1) + tid];
  }
}

int roc_run(Gallery* g, const float* probes, int B, int metric, const int64_t* probe_labels, const int64_t* row_labels,
            const int64_t* first_row, const float* thresholds, int nT, int64_t* accept_out, int64_t* totals_out,
            hipStream_t st) {
  if (B <= 0 || g->n <= 0) {                                 // no pair: zeros
    DIF_HIP(hipMemsetAsync(accept_out, 0, (size_t)nT * 2 * sizeof(int64_t), st));
    DIF_HIP(hipMemsetAsync(totals_out, 0, 4 * sizeof(int64_t), st));
    return 0;
  }
  SumPlan plan;
  if (make_sum_plan(g->d, &plan)) return -1;
  const int clamp = g->clamp_nan ? 1 : 0;
  const int64_t gtiles = (g->n + WITHIN_BM - 1) / WITHIN_BM;
  const Rounds rounds = plan_rounds(gtiles, B, ROC_MASK_MAX, g->roc_round, 128);   // ("roc_round"; a word here is a mask)
  if (ensure(st, workspace(&g->roc_mask, &g->roc_mask_cap, (size_t)gtiles * (size_t)rounds.per, 4 * sizeof(unsigned)),
             workspace(&g->roc_thr, &g->roc_thr_cap, (size_t)rounds.per, 4 * sizeof(float))))
    return -1;
  if (!g->roc_tab) DIF_HIP(hipMalloc(&g->roc_tab, 2 * ROC_TAB * sizeof(float)));
  if (!g->roc_bins) DIF_HIP(hipMalloc(&g->roc_bins, (ROC_BINS + 1) * sizeof(unsigned long long)));
  int P = 2;
  while (P <= nT) P <<= 1;                                   // the power of two above T: P - 1 searchable entries
  hipLaunchKernelGGL(roc_table_kernel, dim3((ROC_BINS + 255) / 256), dim3(256), 0, st, thresholds, nT, metric, g->roc_tab,
                     g->roc_bins);
  DIF_HIP(hipGetLastError());
  const float cdot = g->d * U24;                              // the f32 MFMA: a D-term fma chain
  const size_t res_lds = (size_t)(nT + 2 * (nT + 2)) * 4;
  const int rc = for_rounds(rounds, 0, B, [&](int64_t b0, int nb) {
    const float* pr = probes + b0 * g->d;
    const int64_t* fr = first_row ? first_row + b0 : nullptr;
    hipLaunchKernelGGL(roc_prep_kernel, dim3((nb + 3) / 4), dim3(256), 0, st, pr, nb, g->d, metric, cdot, g->sqmax_bits,
                       reinterpret_cast<f32x4*>(g->roc_thr));
    DIF_HIP(hipGetLastError());
    const int nparts = key_tiles_parts(g, nb);
    if ((gtiles + nparts - 1) / nparts > ROC_BLOCK_TILES)      // (16 M rows per block: no device holds such a gallery)
      return set_error("dif_match_roc: %lld gallery tiles over %d blocks would overflow a block's 32-bit counters", (long long)gtiles, nparts);
    if (with_census_tile(nb, [&](auto tile) {
          using T = decltype(tile);
          return launch_key_tiles<roc_census_kernel<T>, T>(g, pr, nb, metric, st, T::LDS_BYTES, -1, nparts,
                                                           reinterpret_cast<const f32x4*>(g->roc_thr), g->roc_tab, nT, P,
                                                           probe_labels + b0, row_labels, fr, g->index_base, g->roc_mask,
                                                           g->roc_bins);
        }))
      return -1;
    const int64_t nmask = gtiles * nb;
    const int64_t chunks = (nmask + ROC_CHUNK - 1) / ROC_CHUNK, cap = g->roc_blocks > 0 ? g->roc_blocks : 2048;
    const int64_t blocks = chunks < cap ? chunks : cap;
    if (nmask * WITHIN_BM / blocks >= ((int64_t)1 << 32))
      return set_error("dif_match_roc: %lld pairs over %lld resolve blocks would overflow a block's 32-bit counters", (long long)(nmask * WITHIN_BM), (long long)blocks);
    hipLaunchKernelGGL(roc_resolve_kernel, dim3((unsigned)blocks), dim3(ROC_CHUNK), res_lds, st,
                       reinterpret_cast<const u32x4*>(g->roc_mask), nmask, nb, pr, g->rows, g->d, metric, clamp, plan,
                       thresholds, nT, probe_labels + b0, row_labels, g->roc_bins);
    DIF_HIP(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(roc_finish_kernel, dim3(1), dim3(256), 0, st, g->roc_bins, nT, accept_out, totals_out);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dif
