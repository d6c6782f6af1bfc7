// hipcc-flags: -ffp-contract=fast-honor-pragmas
// (build.py compiles with -ffp-contract=fast, which DISREGARDS `#pragma clang fp contract(off)`: area_pixel below restates cv2's
// float32 arithmetic operation by operation and needs the pragma honoured; the other kernels of this file keep contraction)
// Image resampling around the detector (BASELINE configs[4]: raw frames -> detect -> crop -> embed,
// all on the device):
//   letterbox_kernel   detector/yolov3.py:108-119 (letterbox_image): aspect-preserving resize with
//                      PIL's BICUBIC filter (Keys a = -0.5, support widened by the scale factor
//                      when shrinking, i.e. PIL's antialiasing) pasted on a (128,128,128) canvas;
//                      PIL's fixed-point arithmetic, and its extent in Python's doubles.
//   crop_resize_kernel detector/run.py:63-87 (filter_bounding_box: margin, clamp, crop) followed by
//                      the resize predictions.py:93,154 applies: cv2.resize(..., interpolation=
//                      Image.BICUBIC) -- PIL's constant 3, which cv2 reads as INTER_AREA (area
//                      coverage resampling).
// uint8 in, uint8 out, one thread per output pixel; memory-bound and tiny next to the networks.
#include "../../include/dif.h"
#include "dif_internal.hpp"
#include "area_resample.hpp"

namespace dif {

// PIL resamples 8-bit images in fixed point (Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
// ImagingResampleHorizontal_8bpc / Vertical_8bpc): per output coordinate the filter weights in double, normalised by their
// sum, each rounded to an int with 22 fractional bits; the taps are accumulated in int32 from 1 << 21 and shifted down by 22,
// clipped to 0..255; the horizontal pass leaves an 8-bit image to the vertical one.  The functions below are those
// statements, operation by operation (no fused multiply-add), so the result is PIL's own bytes; float32 weights were
// within one grey level of them on most frames and two levels off on a few values of an enlarged frame.
#define PIL_PRECISION_BITS 22

__device__ __forceinline__ double bicubic_w(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// One output coordinate `o` of a 1-D pass: the taps [lo, hi) of the input, and what their weights are made from.
struct PilTaps {
  int lo, hi;
  double center, ss, ww;      // the filter is evaluated at (x - center + 0.5) * ss; ww = the sum of the taps' weights
};
__device__ __forceinline__ PilTaps pil_taps(int o, double scale, int in_size) {
#pragma clang fp contract(off)
  PilTaps t;
  const double filterscale = scale < 1.0 ? 1.0 : scale;      // shrinking widens the support: PIL's antialiasing
  const double support = 2.0 * filterscale;
  t.center = (o + 0.5) * scale;
  t.ss = 1.0 / filterscale;
  t.lo = (int)(t.center - support + 0.5);
  if (t.lo < 0) t.lo = 0;
  t.hi = (int)(t.center + support + 0.5);
  if (t.hi > in_size) t.hi = in_size;
  t.ww = 0.0;
  for (int x = t.lo; x < t.hi; ++x) t.ww += bicubic_w((x - t.center + 0.5) * t.ss);
  return t;
}
// the fixed-point coefficient of tap x
__device__ __forceinline__ int pil_coeff(const PilTaps& t, int x) {
#pragma clang fp contract(off)
  double k = bicubic_w((x - t.center + 0.5) * t.ss);
  if (t.ww != 0.0) k /= t.ww;
  return k < 0 ? (int)(-0.5 + k * (double)(1 << PIL_PRECISION_BITS)) : (int)(0.5 + k * (double)(1 << PIL_PRECISION_BITS));
}
__device__ __forceinline__ int pil_clip8(int ss) {
  const int v = ss >> PIL_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// A block takes tiles of LB_TW x LB_TH canvas pixels, one thread per pixel.  As PIL tabulates a pass's coefficients once, the
// block tabulates its tile's: LB_TW columns and LB_TH rows are LB_TW + LB_TH coordinates for 256 pixels, where every pixel
// would evaluate two.  A coordinate's first LB_KEEP coefficients go to LDS (all of them up to a shrink of 3.7: a coordinate
// has at most 4 * scale + 1 taps); the taps beyond are evaluated where they are used.
constexpr int LB_TW = 32, LB_TH = 8, LB_KEEP = 16;

__global__ __launch_bounds__(LB_TW * LB_TH) void letterbox_kernel(const uint8_t* __restrict__ frames, int N, int H, int W,
                                                                  uint8_t* __restrict__ out, int S, int nw, int nh) {
  __shared__ PilTaps s_taps[LB_TW + LB_TH];              // the tile's columns, then its rows
  __shared__ int s_coeff[LB_TW + LB_TH][LB_KEEP];
  const int tiles_x = (S + LB_TW - 1) / LB_TW, tiles_y = (S + LB_TH - 1) / LB_TH;
  const int64_t total = (int64_t)N * tiles_x * tiles_y;
  const int ox0 = (S - nw) / 2, oy0 = (S - nh) / 2;
  const double sx = (double)W / nw, sy = (double)H / nh;
  const int tid = threadIdx.x, lx = tid % LB_TW, ly = tid / LB_TW;
  const int half = 1 << (PIL_PRECISION_BITS - 1);
  // (the trip count depends on the block alone: every thread reaches both barriers of every trip)
  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int x0 = (int)(tile % tiles_x) * LB_TW, y0 = (int)((tile / tiles_x) % tiles_y) * LB_TH;
    const int64_t n = tile / ((int64_t)tiles_x * tiles_y);
    __syncthreads();                                     // the previous tile's tables have been read
    if (tid < LB_TW + LB_TH) {
      const bool col = tid < LB_TW;
      const int r = col ? x0 + tid - ox0 : y0 + (tid - LB_TW) - oy0;      // the coordinate inside the picture
      if (r >= 0 && r < (col ? nw : nh)) {
        const PilTaps t = pil_taps(r, col ? sx : sy, col ? W : H);
        s_taps[tid] = t;
        for (int j = 0; j < LB_KEEP && t.lo + j < t.hi; ++j) s_coeff[tid][j] = pil_coeff(t, t.lo + j);
      }
    }
    __syncthreads();
    const int x = x0 + lx, y = y0 + ly;
    if (x >= S || y >= S) continue;
    uint8_t* o = out + ((n * S + y) * S + x) * 3;
    const int rx = x - ox0, ry = y - oy0;
    if (rx < 0 || rx >= nw || ry < 0 || ry >= nh) {      // (no table entry was written for such a column or row)
      o[0] = o[1] = o[2] = 128;
      continue;
    }
    // PIL resamples in two passes (horizontal, then vertical), each with its own coefficients and an 8-bit
    // intermediate; do the same per output pixel: the intermediate of every source row the vertical taps touch
    const PilTaps tx = s_taps[lx], ty = s_taps[LB_TW + ly];
    const int* kxs = s_coeff[lx];
    const int* kys = s_coeff[LB_TW + ly];
    const int ntx = tx.hi - tx.lo, nkeep = ntx < LB_KEEP ? ntx : LB_KEEP;
    int acc[3] = {half, half, half};
    for (int yy = ty.lo; yy < ty.hi; ++yy) {
      const int ky = yy - ty.lo < LB_KEEP ? kys[yy - ty.lo] : pil_coeff(ty, yy);
      const uint8_t* row = frames + ((n * H + yy) * W + tx.lo) * 3;
      int r[3] = {half, half, half};
      for (int j = 0; j < nkeep; ++j) {
        const int kx = kxs[j];
        r[0] += row[j * 3] * kx;
        r[1] += row[j * 3 + 1] * kx;
        r[2] += row[j * 3 + 2] * kx;
      }
      for (int j = LB_KEEP; j < ntx; ++j) {
        const int kx = pil_coeff(tx, tx.lo + j);
        r[0] += row[j * 3] * kx;
        r[1] += row[j * 3 + 1] * kx;
        r[2] += row[j * 3 + 2] * kx;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += pil_clip8(r[c]) * ky;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)pil_clip8(acc[c]);
  }
}

// boxes: [N][4] = left, top, right, bottom in frame pixels (as detector/run.py:114 returns them)
// N crops; crop n comes from frame n / K (K boxes per frame: dif_crop_resize_multi; K = 1 otherwise); `valid`: per crop, a
// negative value = an empty slot -> a black crop
__global__ __launch_bounds__(256) void crop_resize_kernel(const uint8_t* __restrict__ frames, int N, int H, int W,
                                                          const float* __restrict__ boxes, float margin,
                                                          uint8_t* __restrict__ out, int SW, int SH, int K = 1,
                                                          const float* __restrict__ valid = nullptr) {
  const int64_t total = (int64_t)N * SW * SH;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % SW);
    const int y = (int)((i / SW) % SH);
    const int64_t n = i / ((int64_t)SW * SH);
    // boxes == nullptr: the whole image (dif_area_resize)
    const float whole[4] = {0.f, 0.f, (float)W, (float)H};
    const float* b = boxes ? boxes + n * 4 : whole;
    crop_pixel(frames + (n / K) * (int64_t)H * W * 3, H, W, b, boxes ? margin : 0.f, valid && valid[n] < 0.f, SW, SH, x, y, out + i * 3);
  }
}

// The resized extent of letterbox_image (yolov3.py:113-115): scale = min(size / w, size / h), nw = int(w * scale), nh =
// int(h * scale), in Python's floats, i.e. IEEE double, one rounding per operation.  The limiting axis lands on an integer
// or one ulp below it, and the truncation makes a pixel of that ulp: float32 disagrees with Python on 8 % of the frame
// sizes up to 640 x 640 at canvas 416 (1280 x 720 among them).  Host only; products only, nothing to contract.
static int letterbox_extent(const char* who, int h, int w, int size, int* nw, int* nh) {
#pragma clang fp contract(off)
  if (h <= 0 || w <= 0 || size <= 0) return set_error("%s: bad sizes", who);
  const double scale = fmin((double)size / (double)w, (double)size / (double)h);
  const double fw = (double)w * scale, fh = (double)h * scale;
  *nw = (int)fw;
  *nh = (int)fh;
  if (*nw < 1 || *nh < 1) return set_error("%s: image too thin", who);
  return 0;
}

}  // namespace dif

using namespace dif;

extern "C" {

int dif_letterbox_extent(int h, int w, int size, int* nw_out, int* nh_out) {
  if (!nw_out || !nh_out) return set_error("dif_letterbox_extent: null pointer");
  return letterbox_extent("dif_letterbox_extent", h, w, size, nw_out, nh_out);
}

int dif_letterbox(const uint8_t* frames_dev, int n, int h, int w, uint8_t* out_dev, int size, void* stream) {
  if (n < 0 || h <= 0 || w <= 0 || size <= 0) return set_error("dif_letterbox: bad sizes");
  if (n == 0) return 0;
  if (!frames_dev || !out_dev) return set_error("dif_letterbox: null pointer");
  int nw, nh;
  if (int rc = letterbox_extent("dif_letterbox", h, w, size, &nw, &nh)) return rc;
  int64_t blocks = (int64_t)n * ((size + LB_TW - 1) / LB_TW) * ((size + LB_TH - 1) / LB_TH);      // one per tile, up to the cap
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(letterbox_kernel, dim3((unsigned)blocks), dim3(LB_TW * LB_TH), 0, (hipStream_t)stream, frames_dev, n, h, w,
                     out_dev, size, nw, nh);
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_crop_resize(const uint8_t* frames_dev, int n, int h, int w, const float* boxes_ltrb_dev, float margin,
                    uint8_t* out_dev, int size, void* stream) {
  if (n < 0 || h <= 0 || w <= 0 || size <= 0) return set_error("dif_crop_resize: bad sizes");
  if (n == 0) return 0;
  if (!frames_dev || !boxes_ltrb_dev || !out_dev) return set_error("dif_crop_resize: null pointer");
  int64_t blocks = ((int64_t)n * size * size + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(crop_resize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_dev, n, h, w,
                     boxes_ltrb_dev, margin, out_dev, size, size);
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_crop_resize_multi(const uint8_t* frames_dev, int n, int h, int w, const float* boxes_ltrb_dev, const float* valid_dev,
                          int k, float margin, uint8_t* out_dev, int size, void* stream) {
  if (n < 0 || h <= 0 || w <= 0 || size <= 0 || k < 1) return set_error("dif_crop_resize_multi: bad sizes");
  if (n == 0) return 0;
  if (!frames_dev || !boxes_ltrb_dev || !out_dev) return set_error("dif_crop_resize_multi: null pointer");
  int64_t blocks = ((int64_t)n * k * size * size + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(crop_resize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_dev, n * k, h, w,
                     boxes_ltrb_dev, margin, out_dev, size, size, k, valid_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_area_resize(const uint8_t* images_dev, int n, int h, int w, uint8_t* out_dev, int out_h, int out_w,
                    void* stream) {
  if (n < 0 || h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) return set_error("dif_area_resize: bad sizes");
  if (n == 0) return 0;
  if (!images_dev || !out_dev) return set_error("dif_area_resize: null pointer");
  int64_t blocks = ((int64_t)n * out_h * out_w + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(crop_resize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, images_dev, n, h, w,
                     (const float*)nullptr, 0.f, out_dev, out_w, out_h);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
