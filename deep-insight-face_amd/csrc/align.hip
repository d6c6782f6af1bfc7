// hipcc-flags: -ffp-contract=off
// Five-point landmark alignment on the device: MTCNN's O-Net landmarks -> similarity transform -> aligned crop, the
// preprocessing every public ArcFace-family embedder is trained on.  The reference aligns on the host (api.py:132-145:
// cv2.getAffineTransform on three landmarks + cv2.warpAffine); PARITY WITH cv2.warpAffine IS UNPINNED -- cv2 quantises the
// coordinates to 1/32 pixel and weighs in 15-bit fixed point; what is pinned is the float32 arithmetic written out below,
// which the tests restate in NumPy operation by operation (hence no FMA contraction in this file).
//   warp_affine_kernel       uint8 NHWC frames -> bilinear warp through a per-crop 2 x 3 matrix that maps an OUTPUT pixel
//                            index to a FRAME position (integer indices are sample positions), constant-zero border.  The
//                            matrix is either read (dif_warp_affine) or fitted in the same launch from five landmarks and
//                            five template points (dif_align_crop): it is uniform per block, thread 0 derives it into LDS.
//   mtcnn_landmarks_kernel   O-Net outputs + the boxes O-Net was shown + the last suppression's keep -> landmarks of the
//                            cascade's output slots in frame pixels.
// Thread -> pixel map: a thread owns four consecutive output pixels = 12 bytes = three dword stores, a wave writes 768
// contiguous bytes; the source taps of neighbouring pixels are neighbours along a line of the frame.
#include "../../include/dif.h"
#include "dif_internal.hpp"

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

// grid (crops, tiles of 1024 pixels); crop j reads frame j / K.  FIT: `src` = landmarks [crops][5][2], the matrix is fitted
// here (and written to matrices_out by the crop's first block when that is not null); otherwise `src` = matrices [crops][6].
// vec: every crop's output starts on a dword and holds a multiple of four pixels -> dword stores; bytes otherwise.
template <bool FIT>
__global__ __launch_bounds__(256) void warp_affine_kernel(const uint8_t* __restrict__ frames, int H, int W,
                                                          const float* __restrict__ src, const float* __restrict__ valid,
                                                          AlignTemplate tpl, int K, uint8_t* __restrict__ out, int OH, int OW,
                                                          float* __restrict__ matrices_out, int vec) {
  __shared__ float sm[6];
  const int j = blockIdx.x;
  if (threadIdx.x == 0) {
    float m[6];
    if (FIT) {
      similarity_fit(src + (int64_t)j * 10, tpl.q, valid && valid[j] < 0.f, m);
      if (matrices_out && blockIdx.y == 0)
        for (int e = 0; e < 6; ++e) matrices_out[(int64_t)j * 6 + e] = m[e];
    } else {
      for (int e = 0; e < 6; ++e) m[e] = src[(int64_t)j * 6 + e];
    }
    for (int e = 0; e < 6; ++e) sm[e] = m[e];
  }
  __syncthreads();
  const int npix = OH * OW;
  const int g = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (g >= npix) return;
  float m[6];
  for (int e = 0; e < 6; ++e) m[e] = sm[e];
  const uint8_t* img = frames + (int64_t)(j / K) * H * W * 3;
  uint8_t* o = out + ((int64_t)j * npix + g) * 3;
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

// out: O-Net outputs [n * nsrc][ld] (logits 2 | box 4 | landmark x 5 | landmark y 5, relative to the crop O-Net saw);
// boxes: [n][nsrc][4], the slots' boxes as dif_crop_resize_multi was given them; keep: [n][k] source slots, < 0 = empty
__global__ __launch_bounds__(256) void mtcnn_landmarks_kernel(const float* __restrict__ out, int ld, const float* __restrict__ boxes,
                                                              const int* __restrict__ keep, int n, int nsrc, int k, int H, int W,
                                                              float* __restrict__ lm) {
  const int total = n * k;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int f = i / k;
    const int s = keep[i];
    float* d = lm + (int64_t)i * 10;
    if (s < 0) {
      for (int e = 0; e < 10; ++e) d[e] = 0.f;
      continue;
    }
    const int64_t q = (int64_t)f * nsrc + s;
    const float* b = boxes + q * 4;
    const float* o = out + q * ld;
    // the rectangle crop_resize_kernel cut out (margin 0): clamped to the frame, truncated
    const int l = (int)fmaxf(b[0], 0.f), t = (int)fmaxf(b[1], 0.f);
    const int r = (int)fminf(b[2], (float)W), bt = (int)fminf(b[3], (float)H);
    const float cw = (float)(r - l), ch = (float)(bt - t);
    for (int e = 0; e < 5; ++e) {
      d[2 * e] = (float)l + o[6 + e] * cw;
      d[2 * e + 1] = (float)t + o[11 + e] * ch;
    }
  }
}

// (38.2946, 51.6963) ... : the five-point template of the public ArcFace preprocessing for 112 x 112 crops
static const float kArcfaceTemplate112[10] = {38.2946f, 51.6963f, 73.5318f, 51.5014f, 56.0252f, 71.7366f, 41.5493f, 92.3655f, 70.7299f, 92.2041f};

template <bool FIT>
static int launch_warp(const char* who, const uint8_t* frames, int n, int h, int w, const float* src, const float* valid,
                       const AlignTemplate& tpl, int k, uint8_t* out, int out_h, int out_w, float* matrices_out, void* stream) {
  if (n < 0 || h <= 0 || w <= 0 || k < 1 || out_h <= 0 || out_w <= 0 || (int64_t)n * k > 0x7fffffff ||
      (int64_t)out_h * out_w > (int64_t)65535 * 1024)
    return set_error("%s: bad sizes", who);
  if (n == 0) return 0;
  if (!frames || !src || !out) return set_error("%s: null pointer", who);
  const int npix = out_h * out_w;
  const int vec = npix % 4 == 0 && ((uintptr_t)out & 3) == 0;
  hipLaunchKernelGGL(warp_affine_kernel<FIT>, dim3((unsigned)(n * k), (unsigned)((npix + 1023) / 1024)), dim3(256), 0,
                     (hipStream_t)stream, frames, h, w, src, valid, tpl, k, out, out_h, out_w, matrices_out, vec);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dif

using namespace dif;

extern "C" {

int dif_warp_affine(const uint8_t* frames_dev, int n_frames, int h, int w, const float* matrices_dev, int k, uint8_t* out_dev,
                    int out_h, int out_w, void* stream) {
  return launch_warp<false>("dif_warp_affine", frames_dev, n_frames, h, w, matrices_dev, nullptr, AlignTemplate{}, k, out_dev, out_h,
                            out_w, nullptr, stream);
}

int dif_align_crop(const uint8_t* frames_dev, int n_frames, int h, int w, const float* landmarks_dev, const float* valid_dev, int k,
                   const float* template_host, uint8_t* out_dev, int size, float* matrices_out_dev, void* stream) {
  AlignTemplate tpl;
  const float s = (float)size / 112.f;
  for (int e = 0; e < 10; ++e) tpl.q[e] = template_host ? template_host[e] : kArcfaceTemplate112[e] * s;
  return launch_warp<true>("dif_align_crop", frames_dev, n_frames, h, w, landmarks_dev, valid_dev, tpl, k, out_dev, size, size,
                           matrices_out_dev, stream);
}

int dif_mtcnn_landmarks(const float* out_dev, int ld, const float* boxes_dev, const int32_t* keep_dev, int n, int n_src, int k, int h,
                        int w, float* landmarks_dev, void* stream) {
  if (n < 0 || ld < 16 || n_src < 1 || k < 1 || h <= 0 || w <= 0 || (int64_t)n * k > 0x7fffffff)
    return set_error("dif_mtcnn_landmarks: bad sizes");
  if (n == 0) return 0;
  if (!out_dev || !boxes_dev || !keep_dev || !landmarks_dev) return set_error("dif_mtcnn_landmarks: null pointer");
  int blocks = (n * k + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mtcnn_landmarks_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, out_dev, ld, boxes_dev, keep_dev,
                     n, n_src, k, h, w, landmarks_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
