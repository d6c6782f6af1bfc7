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
#include "warp_pixel.hpp"

namespace dif {

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
  warp_four(frames + (int64_t)(j / K) * H * W * 3, H, W, m, out + (int64_t)j * npix * 3, npix, OW, g, vec);
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
