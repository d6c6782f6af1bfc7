// What the exact gallery queries (match_within.hip, match_roc.hip) share beyond the band of match_band.hpp:
//   device  the MFMA pass that turns (gallery tile of 128 rows, probe) into one word -- key_tiles, with the part each query
//           differs in as an epilogue policy --, the walk of one probe's words in tile order (walk_words), and the block order
//   host    the launch of such a pass (launch_key_tiles; allow_lds_once is match_ref.hpp's), the rounds of probes a call is cut into (plan_rounds)
//           and the rule by which its workspace grows (ensure)
// Every translation unit that includes this file is built with -ffp-contract=off, as match_ref.hpp asks.
#pragma once
#include "gemm_core.hpp"
#include "dif_internal.hpp"
#include "match_ref.hpp"
#include "match_band.hpp"

namespace dif {

// block -> (gallery part, probe block), in groups of 8 parts x all probe blocks: the probe blocks of one part share an XCD
// (see match_tile_kernel).  A block whose part is >= nparts pads the last group and has nothing to do.
struct TileBlock {
  int part, cblk;
};
__device__ __forceinline__ TileBlock tile_block(int cblocks) {
  const int grp = (int)blockIdx.x / (8 * cblocks), rem = (int)blockIdx.x % (8 * cblocks);
  return TileBlock{grp * 8 + (rem & 7), rem >> 3};
}

// The parts of an epilogue policy that only some queries need; a policy derives from this and overrides what it uses.
struct KeyEpi {
  struct Col {};                                              // what a probe column keeps for the whole block
  struct Tile {};                                             // ... a block for one tile
  struct Rows {};                                             // ... a thread for four consecutive rows of the tile
  __device__ __forceinline__ Col column(int p, int B) const { return Col{}; }
  __device__ __forceinline__ Tile tile(int64_t g0, int rows, int p0, int cols) const { return Tile{}; }   // rows, cols: those that exist
  __device__ __forceinline__ Rows rows(const Tile&, int r) const { return Rows{}; }
};

// The MFMA pass: a sibling of match_tile_kernel<T, false> -- the same tiles, the same f32 MFMA main loop on the rows themselves,
// the same XCD-aware block order, the same search key in the epilogue
//    metric 1: key = -dot / |g|        metric 0: key = |g|^2 - 2 dot
// (aux[g] = -1/|g| or |g|^2, NaN for the rows kept out of the filter).  Every tile belongs to exactly one block, which stores
// one word per (tile, probe): nothing is accumulated in global memory.  The policy `Epi` decides what the word is:
//    Meet                      the 4-byte partial state of a column, as it is combined across lanes and waves
//    column / tile / rows      see KeyEpi
//    start(tile, c)            the State of column c of the probe block at the start of a tile
//    visit(state, col, rows, j, key, ok)   row j of the four: its key for this column; ok: the row is below G
//    partial(state)            the thread's Meet;  combine(a, b)  of two of them
//    store(word index, meet)   the final word of the column
// It is a compile-time type: nothing here asks which query it serves.
template <class T, class Epi>
__device__ __forceinline__ void key_tiles(const float* __restrict__ gallery, int64_t G, const float* __restrict__ probes, int B,
                                          int D, const float* __restrict__ aux, int metric, int nparts, const Epi epi) {
  constexpr int WM = T::WM, WN = T::WN;
  using Meet = typename Epi::Meet;
  static_assert(T::BM == WITHIN_BM, "one word per 128 gallery rows");
  static_assert(sizeof(Meet) == 4, "the columns meet in [WGM][BN] 4-byte words behind the main loop's staging");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int cblocks = (B + T::BN - 1) / T::BN;
  const TileBlock tb = tile_block(cblocks);
  if (tb.part >= nparts) return;
  Meet* s_meet = reinterpret_cast<Meet*>(smem + T::LDS_FLOATS);   // [WGM][BN]: the partial state per wave row
  const int tid = threadIdx.x;
  const int wc = T::wave_col();
  const int p0 = tb.cblk * T::BN;
  const int ksteps = D / BK;
  const int64_t gtiles = (G + T::BM - 1) / T::BM;

  int col[WN];
  typename Epi::Col pc[WN];
#pragma unroll
  for (int n = 0; n < WN; ++n) {
    col[n] = (wc * WN + n) * 32 + (tid & 31);
    pc[n] = epi.column(p0 + col[n], B);
  }

  for (int64_t gt = tb.part; gt < gtiles; gt += nparts) {
    const int64_t g0 = gt * T::BM;
    f32x16 acc[WM][WN];
    zero_acc<T>(acc);
    RowLoader<T::NA, T::RP> al(gallery + g0 * D, G - g0, D);
    RowLoader<T::NB, T::RP> bl(probes + (int64_t)p0 * D, (int64_t)B - p0, D);
    gemm_mainloop<T>(al, bl, 0, ksteps, smem, acc);

    int lane = tid & 63;
    asm volatile("" : "+v"(lane));                           // opaque per tile, as in match_tile_epilogue: no row index is hoisted
    const int wr = T::wave_row();
    const int64_t rows_left = G - g0;
    const int rows_in = (int)(rows_left < T::BM ? rows_left : T::BM), cols_in = B - p0 < T::BN ? B - p0 : T::BN;
    const __amdgpu_buffer_rsrc_t arsrc = make_rsrc(aux + g0, (uint32_t)(rows_in * 4));
    const typename Epi::Tile tile = epi.tile(g0, rows_in, p0, cols_in);
    typename Epi::State s[WN];
#pragma unroll
    for (int n = 0; n < WN; ++n) s[n] = epi.start(tile, col[n]);
#pragma unroll
    for (int m = 0; m < WM; ++m) {
      const int rbase = (wr * WM + m) * 32 + 4 * (lane >> 5);
#pragma unroll
      for (int q = 0; q < 4; ++q) {                          // rows rbase + 8q .. +3 <-> registers 4q .. 4q+3
        const f32x4 ax = buf_load4(arsrc, (uint32_t)(rbase + 8 * q) * 4u);
        const typename Epi::Rows rw = epi.rows(tile, rbase + 8 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool ok = rbase + 8 * q + j < rows_left;
#pragma unroll
          for (int n = 0; n < WN; ++n) {
            const float dot = acc[m][n][4 * q + j];
            const float key = (metric == 1) ? dot * ax[j] : fmaf(-2.f, dot, ax[j]);
            epi.visit(s[n], pc[n], rw, j, key, ok);
          }
        }
      }
    }
    // lanes l and l + 32 hold different rows of the same probe column; the WGM waves stacked on M meet in LDS
#pragma unroll
    for (int n = 0; n < WN; ++n) {
      Meet v = epi.partial(s[n]);
      v = Epi::combine(v, __shfl_xor(v, 32));
      if (lane < 32) s_meet[wr * T::BN + col[n]] = v;
    }
    lds_barrier();
    for (int c = tid; c < T::BN; c += T::NT) {
      Meet v = s_meet[c];
#pragma unroll
      for (int w = 1; w < T::WGM; ++w) v = Epi::combine(v, s_meet[w * T::BN + c]);
      if (p0 + c < B) epi.store(gt * B + p0 + c, v);
    }
    // (s_meet is written again only after the next tile's main loop, i.e. behind several barriers)
  }
}

// One probe's words (`words` rows are B apart) in ascending tile order, 64 * WITHIN_NW of them at a time through s_word.
// wants(word) says whether a thread's word needs its tile looked at; where no thread's does, the words are skipped.  Otherwise
// tile(index, word) runs for each of them, in every thread: it may synchronise the block.  Both callables and gtiles are
// block-uniform, so all control flow is.  (For rank_resolve_kernel and edge_walk; the kernels that synchronise inside a
// tile keep this loop written out -- see within_resolve_kernel.)
template <class Word, class Wants, class TileF>
__device__ __forceinline__ void walk_words(const Word* __restrict__ words, int B, int p, int64_t gtiles, Word* s_word,
                                           Wants wants, TileF tile) {
  constexpr int NT = 64 * WITHIN_NW;
  const int tid = threadIdx.x;
  for (int64_t t0 = 0; t0 < gtiles; t0 += NT) {
    const bool live = t0 + tid < gtiles;
    const Word w = live ? words[(t0 + tid) * B + p] : Word();
    s_word[tid] = w;
    if (!__syncthreads_or(live && wants(w))) continue;        // (also the barrier between two rounds of words)
    const int nw = gtiles - t0 < NT ? (int)(gtiles - t0) : NT;
    for (int j = 0; j < nw; ++j) tile(t0 + j, s_word[j]);
    __syncthreads();                                          // s_word is rewritten by the next round
  }
}

// dynamic LDS of a key_tiles kernel: the main loop's staging, then the [WGM][BN] words the columns meet in
template <class T>
constexpr int key_tiles_lds = T::LDS_BYTES + T::WGM * T::BN * 4;

// The gallery parts of a key-tile launch of B probes over gallery rows [0, rows) (-1: all of them): match_plan_parts'
static int key_tiles_parts(const Gallery* g, int B, int64_t rows = -1) {
  return match_plan_parts(g, B, false, rows < 0 ? g->n : rows);
}

// One launch of a key-tile kernel Kern(gallery, G, probes, B, D, aux, metric, nparts, args...) of tile shape T over gallery
// rows [0, rows) (-1: all of them; the words are laid out as for a gallery of `rows` rows) in the nparts parts of
// key_tiles_parts: the grid is whole groups of 8 parts x all probe blocks (tile_block)
template <auto Kern, class T, class... Args>
static int launch_key_tiles(const Gallery* g, const float* probes, int B, int metric, hipStream_t st, int lds, int64_t rows,
                            int nparts, Args... args) {
  if (allow_lds_once<Kern>(lds)) return -1;
  if (rows < 0) rows = g->n;
  const int cblocks = (B + T::BN - 1) / T::BN;
  dim3 grid((unsigned)(((nparts + 7) / 8) * 8 * cblocks));
  hipLaunchKernelGGL(Kern, grid, dim3(T::NT), lds, st, g->rows, rows, probes, B, g->d, metric == 1 ? g->ninv : g->sq, metric,
                     nparts, args...);
  DIF_HIP(hipGetLastError());
  return 0;
}

// Probes (or rows) per round of a call over n of them whose workspace holds gtiles words each: whole 128-probe blocks that
// keep a round below words_cap words, at least one block; fewer where the option (> 0) asks for fewer, though not below
// `floor`; never more than n.  An empty gallery has no words: one round.
struct Rounds {
  int64_t per;
};
static Rounds plan_rounds(int64_t gtiles, int64_t n, size_t words_cap, int64_t option, int64_t floor) {
  int64_t per = gtiles > 0 ? (int64_t)(words_cap / (size_t)gtiles) / 128 * 128 : n;
  if (per < 128) per = 128;
  if (option > 0 && option < per) per = option;
  if (per < floor) per = floor;
  if (per > n) per = n;
  return Rounds{per};
}
// f(b0, nb) for every round of [first, n); stops at the first non-zero return
template <class F>
static int for_rounds(const Rounds& r, int64_t first, int64_t n, F&& f) {
  for (int64_t b0 = first; b0 < n; b0 += r.per) {
    const int rc = f(b0, (int)(n - b0 < r.per ? n - b0 : r.per));
    if (rc) return rc;
  }
  return 0;
}

// A workspace buffer, its OWN capacity field, and what this call needs of it (in elements of `elem` bytes)
template <class P>
struct Workspace {
  P** buf;
  size_t* cap;
  size_t need, elem;
};
template <class P>
static Workspace<P> workspace(P** buf, size_t* cap, size_t need, size_t elem) {
  return Workspace<P>{buf, cap, need, elem};
}
// If any is short: one stream synchronise (an earlier call on this stream may still read them), then each grows against its
// own capacity
template <class... W>
static int ensure(hipStream_t st, W... w) {
  if (!((w.need > *w.cap) || ...)) return 0;
  DIF_HIP(hipStreamSynchronize(st));
  int rc = 0;
  ((rc = rc ? rc : grow(w.buf, w.cap, w.need, w.elem)), ...);
  return rc;
}

}  // namespace dif
