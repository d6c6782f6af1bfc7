// Area-coverage resampling of one destination pixel (cv2.resize INTER_AREA for uint8 images) and the crop rectangle of
// filter_bounding_box, shared by imageops.hip (dif_crop_resize, dif_crop_resize_multi, dif_area_resize) and faces.hip
// (dif_crop_resize_list).  The functions carry `#pragma clang fp contract(off)`: a translation unit that includes this
// header is compiled with -ffp-contract=fast-honor-pragmas or -ffp-contract=off, never plain =fast, which disregards
// the pragma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dif {

// One destination pixel of cv2.resize(src[ch x cw], (SW, SH), interpolation=INTER_AREA) for uint8 images, operation by
// operation as OpenCV's resize.cpp performs it (the test suite's checker restates the same paths and must be equalled bit for
// bit; PARITY UNPINNED against cv2 itself, which is not installed here):
//   both axes shrink or stay: 2 x 2 blocks (a + b + c + d + 2) >> 2; other integer ratios cvRound(float(sum) * (1.f / area));
//     fractional ratios the DecimateAlpha tables -- per axis (source index, float32 weight) pairs from double arithmetic --
//     with buf = sum_k S * alpha_k per source row and sum = sum_j beta_j * buf_j, every product and addition rounded to
//     float32 in table order (no fused multiply-add), cvRound at the end;
//   an axis enlarges: both axes take the linear path with area-mode coefficients in 11-bit fixed point.
// `src` points at the crop's first pixel, `pitch` = pixels per source row.
struct AreaTaps {                 // computeResizeAreaTab for one destination index: a head, a run of full cells, a tail
  int s_head, s_run0, s_run1, s_tail;       // -1: absent
  float a_head, a_run, a_tail;
};
__device__ __forceinline__ AreaTaps area_taps(int d, int ssize, double scale) {
#pragma clang fp contract(off)      // (HIP's __fmul_rn / __dmul_rn are plain products: without this the compiler fuses them)
  AreaTaps t;
  const double f1 = (double)d * scale;                      // (no fused multiply-add: cv2 rounds the product)
  const double f2 = f1 + scale;
  const double cell = fmin(scale, ssize - f1);
  int s1 = (int)ceil(f1), s2 = (int)floor(f2);
  s2 = s2 < ssize - 1 ? s2 : ssize - 1;
  s1 = s1 < s2 ? s1 : s2;
  t.s_head = (s1 - f1 > 1e-3) ? s1 - 1 : -1;
  t.a_head = (float)((s1 - f1) / cell);
  t.s_run0 = s1;
  t.s_run1 = s2;
  t.a_run = (float)(1.0 / cell);
  t.s_tail = (f2 - s2 > 1e-3) ? s2 : -1;
  t.a_tail = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
  return t;
}
__device__ __forceinline__ void linear_taps(int d, int ssize, int dsize, int& s0, int& s1, int& a0, int& a1) {
#pragma clang fp contract(off)
  const double inv = (double)dsize / ssize, scale = 1.0 / inv;
  const double dsc = (double)d * scale;
  int sx = (int)floor(dsc);
  const double back = (double)(sx + 1) * inv;
  float fx = (float)((double)(d + 1) - back);
  fx = fx <= 0.f ? 0.f : fx - floorf(fx);
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= ssize - 1) { fx = 0.f; sx = ssize - 1; }
  s0 = sx;
  s1 = sx + 1 < ssize ? sx + 1 : ssize - 1;
  const float c0 = 1.f - fx;
  a0 = (int)rintf(c0 * 2048.f);
  a1 = (int)rintf(fx * 2048.f);
}
__device__ __forceinline__ void area_pixel(const uint8_t* __restrict__ src, int pitch, int cw, int ch, int SW, int SH, int x, int y,
                                           uint8_t* __restrict__ o) {
#pragma clang fp contract(off)      // every product and sum below is rounded by itself, as in OpenCV's scalar code
  const double scale_x = 1.0 / ((double)SW / cw), scale_y = 1.0 / ((double)SH / ch);
  if (scale_x >= 1.0 && scale_y >= 1.0) {
    const int ix = (int)scale_x, iy = (int)scale_y;
    if (fabs(scale_x - ix) < 2.220446049250313e-16 && fabs(scale_y - iy) < 2.220446049250313e-16) {
      int sum[3] = {0, 0, 0};
      for (int yy = 0; yy < iy; ++yy)
        for (int xx = 0; xx < ix; ++xx) {
          const uint8_t* p = src + ((int64_t)(y * iy + yy) * pitch + (x * ix + xx)) * 3;
          sum[0] += p[0];
          sum[1] += p[1];
          sum[2] += p[2];
        }
      const float sc = 1.f / (float)(ix * iy);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        o[c] = (ix == 2 && iy == 2) ? (uint8_t)((sum[c] + 2) >> 2) : (uint8_t)fminf(fmaxf(rintf((float)sum[c] * sc), 0.f), 255.f);
      return;
    }
    const AreaTaps tx = area_taps(x, cw, scale_x), ty = area_taps(y, ch, scale_y);
    float sum[3] = {0.f, 0.f, 0.f};
    bool first = true;
    auto row = [&](int sy, float beta) {
#pragma clang fp contract(off)      // (the pragma of the enclosing function does not reach into a lambda's body)
      const uint8_t* r = src + (int64_t)sy * pitch * 3;
      float buf[3] = {0.f, 0.f, 0.f};
      auto tap = [&](int sx, float alpha) {
#pragma clang fp contract(off)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float prod = (float)r[sx * 3 + c] * alpha;      // plain operators under the pragma (HIP's __fmul_rn / __fadd_rn
          buf[c] = buf[c] + prod;                                // are header functions compiled with contraction ON)
        }
      };
      if (tx.s_head >= 0) tap(tx.s_head, tx.a_head);
      for (int sx = tx.s_run0; sx < tx.s_run1; ++sx) tap(sx, tx.a_run);
      if (tx.s_tail >= 0) tap(tx.s_tail, tx.a_tail);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float prod = beta * buf[c];
        sum[c] = first ? prod : sum[c] + prod;
      }
      first = false;
    };
    if (ty.s_head >= 0) row(ty.s_head, ty.a_head);
    for (int sy = ty.s_run0; sy < ty.s_run1; ++sy) row(sy, ty.a_run);
    if (ty.s_tail >= 0) row(ty.s_tail, ty.a_tail);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)fminf(fmaxf(rintf(sum[c]), 0.f), 255.f);
    return;
  }
  int x0, x1, a0, a1, y0, y1, b0, b1;
  linear_taps(x, cw, SW, x0, x1, a0, a1);
  linear_taps(y, ch, SH, y0, y1, b0, b1);
  const uint8_t* r0 = src + (int64_t)y0 * pitch * 3;
  const uint8_t* r1 = src + (int64_t)y1 * pitch * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = r0[x0 * 3 + c] * a0 + r0[x1 * 3 + c] * a1, h1 = r1[x0 * 3 + c] * a0 + r1[x1 * 3 + c] * a1;
    int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    o[c] = (uint8_t)v;
  }
}

// One output pixel (x, y) of the crop of box b = (left, top, right, bottom) out of the frame `img` [H][W][3]:
// filter_bounding_box (run.py:76-80) -- margin/2 on every side, clamped, truncated to int32 -- then area_pixel.
// `empty`, a NaN coordinate or an empty rectangle give a black pixel.
__device__ __forceinline__ void crop_pixel(const uint8_t* __restrict__ img, int H, int W, const float* __restrict__ b, float mg, bool empty,
                                           int SW, int SH, int x, int y, uint8_t* __restrict__ o) {
  int l = (int)fmaxf(b[0] - mg / 2, 0.f), t = (int)fmaxf(b[1] - mg / 2, 0.f);
  int r = (int)fminf(b[2] + mg / 2, (float)W), bt = (int)fminf(b[3] + mg / 2, (float)H);
  const int cw = r - l, ch = bt - t;
  const bool nodet = b[0] != b[0] || b[1] != b[1] || b[2] != b[2] || b[3] != b[3] || empty;   // NaN = no detection
  if (nodet || !(cw > 0 && ch > 0)) {
    o[0] = o[1] = o[2] = 0;
    return;
  }
  area_pixel(img + ((int64_t)t * W + l) * 3, W, cw, ch, SW, SH, x, y, o);
}

}  // namespace dif
