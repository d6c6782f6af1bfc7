// hipcc-flags: -ffp-contract=off
// (warp_pixel.hpp pins its float32 arithmetic operation by operation, as align.hip does; area_resample.hpp carries
// `#pragma clang fp contract(off)` in every function, which this flag honours too: the list forms below are bit-identical
// to the slot forms of imageops.hip and align.hip)
// Every face in a frame: the step between the detectors' fixed slots ([n][k] per batch, score -1 = empty) and the embedder.
//   faces_compact_kernel    scores [n][k] -> the list of slots that hold a face, frame-major and in slot order, the CSR
//                           offsets per frame and the exact total.  ONE block of 1024 threads walks the n * k slots in
//                           passes of 1024: a ballot per wave gives the rank inside the wave, sixteen wave totals go through
//                           LDS, the running total is carried in a register.  No global atomics: the order is fixed by the
//                           slot index alone.  n * k is a few thousand to a few tens of thousands, i.e. tens of passes.
//   crop_resize_list_kernel crop j = the box of slot (frame[j], slot[j]) out of frame frame[j]; arithmetic of
//                           crop_resize_kernel (area_resample.hpp: crop_pixel).
//   align_crop_list_kernel  crop j = the similarity-aligned face of slot (frame[j], slot[j]); arithmetic of
//                           warp_affine_kernel<FIT> (warp_pixel.hpp: similarity_fit, warp_four).
//   faces_gather_kernel     dense rows [m][row_floats] <- the listed slots of [n][k][row_floats].
// A list entry outside [0, n) x [0, k) -- -1 by convention, what the compaction pads with -- reads nothing: a black crop,
// six NaNs, a row of zeros.
#include "../../include/dif.h"
#include "dif_internal.hpp"
#include "area_resample.hpp"
#include "warp_pixel.hpp"

namespace dif {

constexpr int kCompactThreads = 1024;

__global__ __launch_bounds__(kCompactThreads) void faces_compact_kernel(const float* __restrict__ scores, int total, int k, float min_score,
                                                                        int max_faces, int* __restrict__ count, int* __restrict__ offsets,
                                                                        int* __restrict__ frame, int* __restrict__ slot) {
  __shared__ int wave_total[kCompactThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;                                         // faces in the passes before this one (the same in every thread)
  for (int i0 = 0; i0 < total; i0 += kCompactThreads) {
    const int i = i0 + tid;
    const bool face = i < total && scores[i] >= min_score;          // (false for a NaN)
    const unsigned long long mask = __ballot(face);
    const int in_wave = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kCompactThreads / 64; ++w) {
      const int c = wave_total[w];
      before += w < wave ? c : 0;
      all += c;
    }
    __syncthreads();                                    // wave_total is rewritten by the next pass
    const int pos = base + before + in_wave;            // faces in front of slot i
    if (i < total) {
      const int f = i / k, s = i - f * k;
      if (s == 0) offsets[f] = pos;
      if (face && pos < max_faces) {
        frame[pos] = f;
        slot[pos] = s;
      }
    }
    base += all;
  }
  for (int j = (base < max_faces ? base : max_faces) + tid; j < max_faces; j += kCompactThreads) frame[j] = slot[j] = -1;
  if (tid == 0) {
    offsets[total / k] = base;
    count[0] = base;
  }
}

// entry j of the lists -> the slot's index f * k + s, or -1
__device__ __forceinline__ int64_t listed_slot(const int* __restrict__ frame, const int* __restrict__ slot, int64_t j, int n, int k) {
  const int f = frame[j], s = slot[j];
  return (f >= 0 && f < n && s >= 0 && s < k) ? (int64_t)f * k + s : -1;
}

__global__ __launch_bounds__(256) void crop_resize_list_kernel(const uint8_t* __restrict__ frames, int n, int H, int W,
                                                               const float* __restrict__ boxes, int k, const int* __restrict__ frame,
                                                               const int* __restrict__ slot, int m, float margin,
                                                               uint8_t* __restrict__ out, int S) {
  const int64_t total = (int64_t)m * S * S;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % S);
    const int y = (int)((i / S) % S);
    const int64_t j = i / ((int64_t)S * S);
    const int64_t q = listed_slot(frame, slot, j, n, k);
    uint8_t* o = out + i * 3;
    if (q < 0) {
      o[0] = o[1] = o[2] = 0;
      continue;
    }
    crop_pixel(frames + (q / k) * (int64_t)H * W * 3, H, W, boxes + q * 4, margin, false, S, S, x, y, o);
  }
}

// grid (m, tiles of 1024 pixels), as warp_affine_kernel
__global__ __launch_bounds__(256) void align_crop_list_kernel(const uint8_t* __restrict__ frames, int n, int H, int W,
                                                              const float* __restrict__ landmarks, int k, const int* __restrict__ frame,
                                                              const int* __restrict__ slot, AlignTemplate tpl, uint8_t* __restrict__ out,
                                                              int S, float* __restrict__ matrices_out, int vec) {
  __shared__ float sm[6];
  const int j = blockIdx.x;
  const int64_t q = listed_slot(frame, slot, j, n, k);
  if (threadIdx.x == 0) {
    float m[6];
    if (q < 0)
      for (int e = 0; e < 6; ++e) m[e] = __builtin_nanf("");
    else
      similarity_fit(landmarks + q * 10, tpl.q, false, m);
    if (matrices_out && blockIdx.y == 0)
      for (int e = 0; e < 6; ++e) matrices_out[(int64_t)j * 6 + e] = m[e];
    for (int e = 0; e < 6; ++e) sm[e] = m[e];
  }
  __syncthreads();
  const int npix = S * S;
  const int g = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (g >= npix) return;
  float m[6];
  for (int e = 0; e < 6; ++e) m[e] = sm[e];
  warp_four(frames + (q < 0 ? 0 : q / k) * (int64_t)H * W * 3, H, W, m, out + (int64_t)j * npix * 3, npix, S, g, vec);
}

__global__ __launch_bounds__(256) void faces_gather_kernel(const float* __restrict__ src, int row, int n, int k,
                                                           const int* __restrict__ frame, const int* __restrict__ slot, int m,
                                                           float* __restrict__ dst) {
  const int64_t total = (int64_t)m * row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t j = i / row;
    const int e = (int)(i - j * row);
    const int64_t q = listed_slot(frame, slot, j, n, k);
    dst[i] = q < 0 ? 0.f : src[q * row + e];
  }
}

}  // namespace dif

using namespace dif;

extern "C" {

int dif_faces_compact(const float* scores_dev, int n, int k, float min_score, int max_faces, int32_t* count_dev, int32_t* offsets_dev,
                      int32_t* frame_dev, int32_t* slot_dev, void* stream) {
  if (n < 0 || k < 1 || max_faces < 0 || (int64_t)n * k > 0x7fffffff - kCompactThreads) return set_error("dif_faces_compact: bad sizes");
  if (!count_dev || !offsets_dev || (n > 0 && !scores_dev) || (max_faces > 0 && (!frame_dev || !slot_dev)))
    return set_error("dif_faces_compact: null pointer");
  // (n = 0: no pass; the kernel writes count = 0, offsets[0] = 0 and pads the lists)
  hipLaunchKernelGGL(faces_compact_kernel, dim3(1), dim3(kCompactThreads), 0, (hipStream_t)stream, scores_dev, n * k, k, min_score, max_faces,
                     count_dev, offsets_dev, frame_dev, slot_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

static int list_args(const char* who, int n, int h, int w, int k, int m, int size) {
  if (n < 0 || h <= 0 || w <= 0 || k < 1 || m < 0 || size <= 0 || (int64_t)n * k > 0x7fffffff) return set_error("%s: bad sizes", who);
  return 0;
}

int dif_crop_resize_list(const uint8_t* frames_dev, int n, int h, int w, const float* boxes_ltrb_dev, int k, const int32_t* frame_dev,
                         const int32_t* slot_dev, int m, float margin, uint8_t* out_dev, int size, void* stream) {
  if (list_args("dif_crop_resize_list", n, h, w, k, m, size)) return -1;
  if (m == 0) return 0;
  if (!frame_dev || !slot_dev || !out_dev || (n > 0 && (!frames_dev || !boxes_ltrb_dev))) return set_error("dif_crop_resize_list: null pointer");
  int64_t blocks = ((int64_t)m * size * size + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(crop_resize_list_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_dev, n, h, w, boxes_ltrb_dev,
                     k, frame_dev, slot_dev, m, margin, out_dev, size);
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_align_crop_list(const uint8_t* frames_dev, int n, int h, int w, const float* landmarks_dev, int k, const int32_t* frame_dev,
                        const int32_t* slot_dev, int m, const float* template_host, uint8_t* out_dev, int size, float* matrices_out_dev,
                        void* stream) {
  if (list_args("dif_align_crop_list", n, h, w, k, m, size)) return -1;
  if ((int64_t)size * size > (int64_t)65535 * 1024 || m > 0x7fffffff / 6) return set_error("dif_align_crop_list: bad sizes");
  if (m == 0) return 0;
  if (!frame_dev || !slot_dev || !out_dev || (n > 0 && (!frames_dev || !landmarks_dev))) return set_error("dif_align_crop_list: null pointer");
  AlignTemplate tpl;
  const float s = (float)size / 112.f;
  for (int e = 0; e < 10; ++e) tpl.q[e] = template_host ? template_host[e] : kArcfaceTemplate112[e] * s;
  const int npix = size * size;
  const int vec = npix % 4 == 0 && ((uintptr_t)out_dev & 3) == 0;
  hipLaunchKernelGGL(align_crop_list_kernel, dim3((unsigned)m, (unsigned)((npix + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream,
                     frames_dev, n, h, w, landmarks_dev, k, frame_dev, slot_dev, tpl, out_dev, size, matrices_out_dev, vec);
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_faces_gather(const float* src_dev, int row_floats, int n, int k, const int32_t* frame_dev, const int32_t* slot_dev, int m,
                     float* dst_dev, void* stream) {
  if (row_floats < 1 || n < 0 || k < 1 || m < 0 || (int64_t)n * k > 0x7fffffff) return set_error("dif_faces_gather: bad sizes");
  if (m == 0) return 0;
  if (!frame_dev || !slot_dev || !dst_dev || (n > 0 && !src_dev)) return set_error("dif_faces_gather: null pointer");
  int64_t blocks = ((int64_t)m * row_floats + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(faces_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src_dev, row_floats, n, k, frame_dev,
                     slot_dev, m, dst_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
