// What the kernels over the rows of a batch of frames share (redact.hip, annotate.hip, deteval.hip, tracks.hip): the region
// of a box -- steps 1 to 8 of the rule in include/dif.h, "redaction" --, the two searches for the frame of a row, the rows of a
// frame, and the list of a frame's lower faces that the two paint kernels test their pixels against.  The box arithmetic
// restates tests/redact_ref.py's float32 operation by operation, so every file that includes this pins -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dif {

struct FrameRegion {                             // the unclipped region [X0, X1) x [Y0, Y1)
  int X0, Y0, X1, Y1;
};

__device__ __forceinline__ bool frame_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }   // false for NaN
__device__ __forceinline__ float frame_clamp(float v) { return __builtin_fminf(__builtin_fmaxf(v, -4096.0f), 12288.0f); }

// steps 1 to 8 of the rule
__device__ inline bool frame_region(const float* __restrict__ box, float margin, FrameRegion* out) {
#pragma clang fp contract(off)
  const float l = box[0], t = box[1], r = box[2], b = box[3];
  const float bw = r - l, bh = b - t;
  if (!(frame_finite(l) && frame_finite(t) && frame_finite(r) && frame_finite(b)) || !(bw > 0.0f) || !(bh > 0.0f)) return false;
  const float mw = margin * bw, mh = margin * bh;
  const float le = l - mw, re = r + mw, te = t - mh, be = b + mh;
  if (!(frame_finite(le) && frame_finite(re) && frame_finite(te) && frame_finite(be)) || !(re > le) || !(be > te)) return false;
  out->X0 = (int)__builtin_floorf(frame_clamp(le));
  out->X1 = (int)__builtin_ceilf(frame_clamp(re));
  out->Y0 = (int)__builtin_floorf(frame_clamp(te));
  out->Y1 = (int)__builtin_ceilf(frame_clamp(be));
  return out->X1 > out->X0 && out->Y1 > out->Y0;
}

// Two searches for the frame of a row.  Which one is right depends on who asks:
//   frame_of_row   all lanes of a wave ask for the SAME row (a block per face: redact, annotate).  The 64-way search: one
//                  chain of ceil(log64 n) dependent loads, and that chain is most of what a short block costs.
//   frame_bisect   every thread asks for a row of its OWN (deteval, tracks).  log2 n loads per thread, no lane waits for
//                  another.
// Neither is a form of the other: the 64-way search spends a whole wave on one row.

// The frame of row i and that frame's first row, for offsets[0] <= i < offsets[n]; every lane of the wave calls it with the
// same i.  offsets[lo] <= i < offsets[hi], narrowed 64-fold per step: every lane looks at one of 64 evenly spaced entries and
// the wave counts the lanes at or below i (ascending offsets make them a prefix).  Whatever offsets hold, lo and hi stay inside
// [0, n], the span shrinks to 1, and `first` lies in [0, i].
__device__ inline void frame_of_row(long long i, long long n, const long long* __restrict__ offsets, long long* frame, long long* first_row) {
  const int lane = threadIdx.x & 63;
  long long lo = 0, hi = n;
  while (hi - lo > 1) {
    const long long step = (hi - lo + 63) / 64, at = lo + lane * step;
    const int below = __popcll(__ballot(at < hi && offsets[at] <= i));
    const long long next = lo + (below > 0 ? below - 1 : 0) * step;
    hi = next + step < hi ? next + step : hi;
    lo = next;
  }
  *frame = lo;
  const long long first = offsets[lo];
  *first_row = first < 0 ? 0 : (first > i ? i : first);
}

// the frame of row d, per thread: the last f in [0, n) with offsets[f] <= d (offsets[0] = 0; n >= 1)
__device__ __forceinline__ int64_t frame_bisect(const int64_t* __restrict__ offsets, int64_t n, int64_t d) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] <= d) lo = mid; else hi = mid;
  }
  return lo;
}

// rows [begin, end) of frame f, whatever `offsets` holds: never outside [0, total]
__device__ __forceinline__ void frame_rows(const int64_t* __restrict__ offsets, int64_t f, int64_t total, int64_t* begin, int64_t* end) {
  int64_t b = offsets[f], e = offsets[f + 1];
  b = b < 0 ? 0 : (b > total ? total : b);
  e = e < b ? b : (e > total ? total : e);
  *begin = b;
  *end = e;
}

// The faces of rows [first, first + lower) -- the lower rows of the block's frame, at most one per thread -- that `item(row,
// &out)` accepts (a selected face whose region or footprint meets the block's band), compacted in row order into `listed` by
// ballot: no atomics.  Returns their number.  Every thread of the block calls it; the list may be read after the NEXT
// __syncthreads(), which is the caller's to place.  wave_hits: one int per wave.
template <int WAVES, typename T, typename Item>
__device__ __forceinline__ int frame_list_lower(int tid, int lane, int wave, long long lower, long long first, Item&& item, T* listed,
                                                int* wave_hits) {
  bool hit = false;
  T q;
  if (tid < lower) hit = item(first + tid, &q);
  const unsigned long long votes = __ballot(hit);
  if (lane == 0) wave_hits[wave] = __popcll(votes);
  __syncthreads();
  int before = 0, n_listed = 0;
#pragma unroll
  for (int v = 0; v < WAVES; ++v) {
    if (v < wave) before += wave_hits[v];
    n_listed += wave_hits[v];
  }
  if (hit) listed[before + __popcll(votes & ((1ull << lane) - 1ull))] = q;
  return n_listed;
}

// Does a lower face of the frame take the pixel that `covers(face)` asks about?  The listed faces, or -- use_list false: the
// frame has more lower faces than the block lists -- rows [first, i) one by one, as `face(row, &out)` builds them.
template <typename T, typename Face, typename Covers>
__device__ __forceinline__ bool frame_lower_covers(bool use_list, const T* listed, int n_listed, long long first, long long i, Face&& face,
                                                   Covers&& covers) {
  bool taken = false;
  if (use_list) {
    for (int e = 0; e < n_listed && !taken; ++e) taken = covers(listed[e]);
  } else {
    for (long long r = first; r < i && !taken; ++r) {
      T q;
      taken = face(r, &q) && covers(q);
    }
  }
  return taken;
}

}  // namespace dif
