// What the kernels that write into frames share (redact.hip, annotate.hip): the region of a box -- steps 1 to 8 of the rule
// in include/dif.h, "redaction" -- and the search for the frame of a row of faces.  The box arithmetic restates
// tests/redact_ref.py's float32 operation by operation, so every file that includes this pins -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

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

// The frame of row i and that frame's first row, for offsets[0] <= i < offsets[n]; every lane of the wave calls it with the
// same i.  offsets[lo] <= i < offsets[hi], narrowed 64-fold per step: every lane looks at one of 64 evenly spaced entries and
// the wave counts the lanes at or below i (ascending offsets make them a prefix).  A chain of ceil(log64 n) loads instead of
// log2 n; whatever offsets hold, lo and hi stay inside [0, n], the span shrinks to 1, and `first` lies in [0, i].
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

}  // namespace dif
