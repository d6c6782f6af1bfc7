// The float32 IoU of two boxes that non-max suppression (detector.hip) and the tracks' gate (tracks.hip) share.  It restates
// float32 arithmetic operation by operation through a pragma, so a file that includes this is compiled with -ffp-contract=off
// or -ffp-contract=fast-honor-pragmas: plain -ffp-contract=fast, build.py's default, disregards the pragma.
#pragma once
#include <hip/hip_runtime.h>

namespace dif {

// IoU with the corner normalisation of tf.image.non_max_suppression, every product rounded to float32 before it is added:
// contracted, the union became fma(-ih, iw, ap + aq), one rounding fewer than the float32 statement the tests compare
// with, and an IoU that lands exactly on the threshold was suppressed.  The min / max normalisation pairs element 0 with 2
// and 1 with 3, so it serves left, top, right, bottom as it serves y0, x0, y1, x1.
__device__ __forceinline__ float box_iou(const float* p, const float* q) {
#pragma clang fp contract(off)
  const float py0 = fminf(p[0], p[2]), py1 = fmaxf(p[0], p[2]), px0 = fminf(p[1], p[3]), px1 = fmaxf(p[1], p[3]);
  const float qy0 = fminf(q[0], q[2]), qy1 = fmaxf(q[0], q[2]), qx0 = fminf(q[1], q[3]), qx1 = fmaxf(q[1], q[3]);
  const float ap = (py1 - py0) * (px1 - px0), aq = (qy1 - qy0) * (qx1 - qx0);
  if (ap <= 0.f || aq <= 0.f) return 0.f;
  const float ih = fmaxf(fminf(py1, qy1) - fmaxf(py0, qy0), 0.f);
  const float iw = fmaxf(fminf(px1, qx1) - fmaxf(px0, qx0), 0.f);
  const float inter = ih * iw;
  return inter / (ap + aq - inter);
}

}  // namespace dif
