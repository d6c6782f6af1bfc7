// The five-point similarity fit and the bilinear warp of one output pixel, shared by align.hip (dif_warp_affine,
// dif_align_crop) and faces.hip (dif_align_crop_list).  The float32 arithmetic is pinned operation by operation
// (include/dif.h): a translation unit that includes this header is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dif {

struct AlignTemplate {
  float q[10];      // five (x, y) points in output pixels
};

// Least-squares similarity (rotation, uniform scale, translation; no reflection) taking the landmarks p to the template q,
// inverted: m maps output pixels to frame positions.  Closed form in 2-D:
//   q - mq ~ [[a, -b], [b, a]] (p - mp),  a = sum pc.qc / sum |pc|^2,  b = sum pc x qc / sum |pc|^2
__device__ void similarity_fit(const float* __restrict__ p, const float* q, bool dead, float* m) {
  bool ok = !dead;
  float mpx = 0.f, mpy = 0.f, mqx = 0.f, mqy = 0.f;
  for (int k = 0; k < 5; ++k) {
    ok = ok && __builtin_isfinite(p[2 * k]) && __builtin_isfinite(p[2 * k + 1]);
    mpx = mpx + p[2 * k];
    mpy = mpy + p[2 * k + 1];
    mqx = mqx + q[2 * k];
    mqy = mqy + q[2 * k + 1];
  }
  mpx = mpx / 5.f;
  mpy = mpy / 5.f;
  mqx = mqx / 5.f;
  mqy = mqy / 5.f;
  float den = 0.f, dot = 0.f, cr = 0.f;
  for (int k = 0; k < 5; ++k) {
    const float pcx = p[2 * k] - mpx, pcy = p[2 * k + 1] - mpy;
    const float qcx = q[2 * k] - mqx, qcy = q[2 * k + 1] - mqy;
    den = den + (pcx * pcx + pcy * pcy);
    dot = dot + (pcx * qcx + pcy * qcy);
    cr = cr + (pcx * qcy - pcy * qcx);
  }
  const float a = dot / den, b = cr / den;
  const float n2 = a * a + b * b;
  if (!ok || den == 0.f || n2 == 0.f) {
    for (int e = 0; e < 6; ++e) m[e] = __builtin_nanf("");
    return;
  }
  const float ia = a / n2, ib = b / n2;
  m[0] = ia;
  m[1] = ib;
  m[2] = mpx - (ia * mqx + ib * mqy);
  m[3] = -ib;
  m[4] = ia;
  m[5] = mpy - (-ib * mqx + ia * mqy);
}

// One output pixel (x, y) -> three bytes.  A matrix holding a NaN or an infinity makes sx or sy non-finite for every pixel.
__device__ __forceinline__ void warp_pixel(const uint8_t* __restrict__ img, int H, int W, const float* m, int x, int y, uint8_t* o) {
  const float xf = (float)x, yf = (float)y;
  const float sx = (m[0] * xf + m[1] * yf) + m[2];
  const float sy = (m[3] * xf + m[4] * yf) + m[5];
  const float x0 = floorf(sx), y0 = floorf(sy);
  // the 2 x 2 footprint x0 .. x0 + 1 must touch the frame; decided in float, so the conversions below see [-1, size - 1] only
  if (!(__builtin_isfinite(sx) && __builtin_isfinite(sy)) || x0 < -1.f || x0 > (float)(W - 1) || y0 < -1.f || y0 > (float)(H - 1)) {
    o[0] = o[1] = o[2] = 0;
    return;
  }
  const float fx = sx - x0, fy = sy - y0;
  const int ix = (int)x0, iy = (int)y0;
  const bool l = ix >= 0, r = ix + 1 < W, t = iy >= 0, b = iy + 1 < H;
  const int64_t i00 = ((int64_t)iy * W + ix) * 3, i10 = i00 + (int64_t)W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p00 = (l && t) ? (float)img[i00 + c] : 0.f;
    const float p01 = (r && t) ? (float)img[i00 + 3 + c] : 0.f;
    const float p10 = (l && b) ? (float)img[i10 + c] : 0.f;
    const float p11 = (r && b) ? (float)img[i10 + 3 + c] : 0.f;
    const float top = p00 + (p01 - p00) * fx;
    const float bot = p10 + (p11 - p10) * fx;
    const float v = top + (bot - top) * fy;
    o[c] = (uint8_t)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
  }
}

// Four consecutive output pixels g .. g + 3 of one crop (`crop` = its first byte, npix = OH * OW pixels) through the matrix m.
// vec: the crop starts on a dword and holds a multiple of four pixels -> three dword stores; bytes otherwise.
__device__ __forceinline__ void warp_four(const uint8_t* __restrict__ img, int H, int W, const float* m, uint8_t* __restrict__ crop, int npix,
                                          int OW, int g, int vec) {
  uint8_t* o = crop + (int64_t)g * 3;
  uint8_t px[12];
  const int cnt = npix - g < 4 ? npix - g : 4;
  int x = g % OW, y = g / OW;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < cnt)
      warp_pixel(img, H, W, m, x, y, px + 3 * q);
    else
      px[3 * q] = px[3 * q + 1] = px[3 * q + 2] = 0;
    if (++x == OW) {
      x = 0;
      ++y;
    }
  }
  if (vec) {      // (cnt == 4 here: the crop holds a multiple of four pixels)
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int e = 0; e < 3; ++e)
      o4[e] = (uint32_t)px[4 * e] | ((uint32_t)px[4 * e + 1] << 8) | ((uint32_t)px[4 * e + 2] << 16) | ((uint32_t)px[4 * e + 3] << 24);
  } else {
#pragma unroll
    for (int e = 0; e < 12; ++e)
      if (e < 3 * cnt) o[e] = px[e];
  }
}

// (38.2946, 51.6963) ... : the five-point template of the public ArcFace preprocessing for 112 x 112 crops
static const float kArcfaceTemplate112[10] = {38.2946f, 51.6963f, 73.5318f, 51.5014f, 56.0252f, 71.7366f, 41.5493f, 92.3655f, 70.7299f, 92.2041f};

}  // namespace dif
