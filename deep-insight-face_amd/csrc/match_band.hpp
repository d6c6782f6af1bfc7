// The pieces of the range search (match_within.hip) that the all-pairs verification counts (match_roc.hip) share: the census
// tile height, the band of one probe at a tolerance -- the proven bound; its derivation is the header comment of
// match_within.hip -- and the |q|^2 it is formed from.
// Every translation unit that includes this file is built with -ffp-contract=off, as match_ref.hpp asks.
#pragma once
#include "gemm_core.hpp"
#include "match_ref.hpp"

namespace dif {

constexpr int WITHIN_BM = 128;          // gallery rows per census word: every f32 tile shape of the match has 128-row tiles
constexpr int WITHIN_NW = 8;            // waves of a resolve block

// The f32 tile shape of a census over nb probes, as the match chooses it (match_tile_kind): f(Tile<...>{}) launches the kernel
// built for that shape.  Every shape has 128-row tiles and 256 threads.
template <class F>
static int with_census_tile(int nb, F&& f) {
  const int kind = match_tile_kind(nb);
  if (kind == 4 && nb <= 32) return f(Tile<1, 1, 4, 1>{});
  if (kind == 1 || nb <= 64) return f(Tile<2, 1>{});
  return f(Tile<2, 2>{});
}

// The band of one probe at tolerance t (the formulas of the header comment); s = |q|^2 summed as an fma chain over 64 lanes.
struct Band {
  float T, E, H;
  bool odd;                                                   // outside the bound's validity: every tile is resolved
};
__device__ __forceinline__ Band within_band(int metric, float t, float s, int D, float cdot,
                                            const unsigned* __restrict__ sqmax_bits) {
  const float u = U24, qn = sqrtf(s) * 1.0001f, inf = __builtin_inff();
  Band b;
  if (metric == 1) {
    b.odd = !(s >= NORM_LO && s <= NORM_HI);
    b.E = key_err1_rel(cdot) * qn + (96.f + (float)(D / 64)) * u * qn;
    b.T = t >= 1.f ? inf : (t < 0.f ? -inf : (float)(-sqrt((double)s) * cos(3.14159265358979323846 * (double)t)));
    b.H = sqrtf(s) * (1.f - (2e-4f + 1.01f * (cdot + 136.f * u)));
  } else {
    b.odd = !(s <= NORM_HI);
    const float gmax = sqrtf(__builtin_bit_cast(float, *sqmax_bits)) * 1.0001f;
    b.E = key_err0(cdot, qn, gmax) + 32.f * u * (qn + gmax) * (qn + gmax) +
          ((float)(D / 64) + 8.f) * u * (qn * qn + gmax * gmax) + u * (fabsf(t) + qn * qn);
    b.T = t - s;
    b.H = inf;
  }
  return b;
}

// |q|^2 of one probe row by one wave: an fma chain per lane, then the butterfly (every lane returns the sum)
__device__ __forceinline__ float probe_sq(const float* __restrict__ q, int D, int lane) {
  float s = 0.f;
  for (int k = lane; k < D; k += 64) {
    const float x = q[k];
    s = fmaf(x, x, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

}  // namespace dif
