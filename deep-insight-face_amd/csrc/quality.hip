// hipcc-flags: -ffp-contract=off
// (the float columns restate tests/quality_ref.py's float64 arithmetic operation by operation: a product is rounded before
// it is added)
// Face quality: per-face image and pose measures (include/dif.h, "face quality").
//   quality_kernel   one block per crop.  Pass 1 reads the crop once -- 16 pixels = 48 bytes = three 16-byte loads per
//                    thread and step, from the first pixel whose address is aligned to 16 bytes; the pixels in front of
//                    it and behind the last full group go one by one --, writes gray into LDS as bytes and keeps the
//                    sums over all pixels.  Pass 2 takes the Laplacian of the interior from LDS: a wave per band of rows
//                    and chunk of 64 columns, a lane per column walking down, so no index is ever divided, nothing
//                    wraps from a row into the next and a pixel costs three byte reads.  The partials
//                    are 32-bit per thread (bounds below), 64-bit from the wave reduction on, and cross the waves
//                    through the gray buffer, which is free by then.  Thread 0 forms the float columns in double.
// No atomics; every sum is an integer, so the order of the reduction does not show.
#include "../../include/dif.h"
#include "dif_internal.hpp"

namespace dif {

constexpr int kQualityThreads = 512;             // measured against 256 and 1024 at M = 8 and M = 512 (DESIGN): the fastest of the three
constexpr int kQualityWaves = kQualityThreads / 64;
constexpr int kQualityMaxSize = 256;
constexpr int kQualitySums = 6;

// Per-thread 32-bit partials, S <= 256.  Pass 1: a thread takes at most 65536 / 16 / 512 = 8 groups of 16 pixels and
// one pixel each of head and tail, 130 pixels: sum g <= 130 * 255, sum g*g <= 130 * 65025 = 8.5e6.  Pass 2: a lane takes
// one column of one band of rows, and there are at least two bands: at most ceil(254 / 2) = 127 pixels with
// |L| <= 4 * 255 = 1020: |sum L| <= 1.3e5, sum L*L <= 127 * 1040400 = 1.4e8 < 2^32.
static_assert(kQualityMaxSize * kQualityMaxSize / 16 / kQualityThreads * 16 + 2 <= 258, "pass 1 bound");
static_assert(kQualityWaves / ((kQualityMaxSize - 2 + 63) / 64) >= 2 && (kQualityMaxSize - 2 + 1) / 2 <= 128, "pass 2 bound");

struct QualityPartial {
  unsigned sg = 0, sg2 = 0, dark = 0, bright = 0;

  __device__ __forceinline__ unsigned char add(unsigned c0, unsigned c1, unsigned c2, unsigned lo, unsigned hi) {
    const unsigned g = (c0 + 2u * c1 + c2 + 2u) >> 2;
    sg += g;
    sg2 += g * g;
    dark += g <= lo;
    bright += g >= hi;
    return (unsigned char)g;
  }
};

__device__ __forceinline__ double quality_nan() { return __builtin_nan(""); }
// np.minimum / np.maximum: a NaN operand is the result
__device__ __forceinline__ double np_min(double a, double b) { return (a != a || b != b) ? quality_nan() : (a < b ? a : b); }
__device__ __forceinline__ double np_max(double a, double b) { return (a != a || b != b) ? quality_nan() : (a > b ? a : b); }

__device__ void quality_columns(const long long* __restrict__ s, int S, const float* __restrict__ lm, const float* __restrict__ box, float frame_h,
                                float frame_w, float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long n = (long long)S * S, k = (long long)(S - 2) * (S - 2);
  const float brightness = (float)((double)s[0] / (double)(n * 255));
  const float contrast = (float)(__builtin_sqrt((double)(n * s[1] - s[0] * s[0]) / (double)(n * n)) / 255.0);
  const float sharpness = (float)((double)(k * s[3] - s[2] * s[2]) / (double)(k * k));
  const float clipped = (float)((double)(s[4] + s[5]) / (double)n);
  float eye_dist = __builtin_nanf(""), roll = eye_dist, yaw = eye_dist, nose_drop = eye_dist, inside = eye_dist;
  if (lm) {
    const double lx = lm[0], ly = lm[1], rx = lm[2], ry = lm[3], nx = lm[4], ny = lm[5];
    const double mlx = lm[6], mly = lm[7], mrx = lm[8], mry = lm[9];
    const double ex = rx - lx, ey = ry - ly;
    const double e2 = ex * ex + ey * ey;
    const double ed = __builtin_sqrt(e2);
    eye_dist = (float)ed;
    roll = (float)(ey / ed);
    const double t = ((nx - lx) * ex + (ny - ly) * ey) / e2;
    yaw = (float)(2.0 * t - 1.0);
    const double cx = (lx + rx) * 0.5, cy = (ly + ry) * 0.5;
    const double vx = (mlx + mrx) * 0.5 - cx, vy = (mly + mry) * 0.5 - cy;
    nose_drop = (float)(((nx - cx) * vx + (ny - cy) * vy) / (vx * vx + vy * vy));
  }
  if (box) {
    const double l = box[0], t = box[1], r = box[2], b = box[3], W = frame_w, H = frame_h;
    const double iw = np_max(np_min(r, W) - np_max(l, 0.0), 0.0);
    const double ih = np_max(np_min(b, H) - np_max(t, 0.0), 0.0);
    inside = (float)((iw * ih) / ((r - l) * (b - t)));
  }
  double score = (double)sharpness * (1.0 - (double)clipped);
  if (lm) score = score * np_max(0.0, 1.0 - __builtin_fabs((double)yaw));
  if (box) score = score * (double)inside;
  out[0] = brightness;
  out[1] = contrast;
  out[2] = sharpness;
  out[3] = clipped;
  out[4] = eye_dist;
  out[5] = roll;
  out[6] = yaw;
  out[7] = nose_drop;
  out[8] = inside;
  out[9] = (float)score;
}

__global__ __launch_bounds__(kQualityThreads) void quality_kernel(const unsigned char* __restrict__ crops, int S, const float* __restrict__ landmarks,
                                                                  const float* __restrict__ boxes, float frame_h, float frame_w, int lo, int hi,
                                                                  long long* __restrict__ stats, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gray[];   // [S * S]; the waves' sums once pass 2 is done
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = S * S;
  const unsigned char* __restrict__ crop = crops + (size_t)blockIdx.x * (size_t)n * 3;
  // pixel p0 is the first whose address is a multiple of 16: 3 * p0 = -address (mod 16), and 3 * 11 = 1 (mod 16)
  int head = (int)((5u * (unsigned)(uintptr_t)crop) & 15u);
  if (head > n) head = n;
  const int groups = (n - head) / 16;
  const int tail = head + groups * 16;
  QualityPartial part;
  const unsigned ulo = (unsigned)lo, uhi = (unsigned)hi;
  for (int p = tid; p < head; p += kQualityThreads) gray[p] = part.add(crop[3 * p], crop[3 * p + 1], crop[3 * p + 2], ulo, uhi);
  for (int p = tail + tid; p < n; p += kQualityThreads) gray[p] = part.add(crop[3 * p], crop[3 * p + 1], crop[3 * p + 2], ulo, uhi);
  const uint4* __restrict__ wide = (const uint4*)(crop + 3 * head);
  for (int j = tid; j < groups; j += kQualityThreads) {
    const uint4 a = wide[3 * j], b = wide[3 * j + 1], c = wide[3 * j + 2];
    const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    unsigned packed[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                 // four pixels = three words: c0 c1 c2 c0 | c1 c2 c0 c1 | c2 c0 c1 c2
      const unsigned w0 = w[3 * q], w1 = w[3 * q + 1], w2 = w[3 * q + 2];
      const unsigned g0 = part.add(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, ulo, uhi);
      const unsigned g1 = part.add(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, ulo, uhi);
      const unsigned g2 = part.add((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, ulo, uhi);
      const unsigned g3 = part.add((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, ulo, uhi);
      packed[q] = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    }
    unsigned char* dst = gray + head + 16 * j;
    if (head == 0) {
      *(uint4*)dst = make_uint4(packed[0], packed[1], packed[2], packed[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q) dst[q] = (unsigned char)(packed[q >> 2] >> (8 * (q & 3)));
    }
  }
  __syncthreads();
  // a wave walks one band of rows of one chunk of 64 columns downwards, a lane per column: the pixels above and below come
  // from the rows the lane has read already, so a pixel costs three byte reads whose addresses no sum waits on
  int sl = 0;
  unsigned sl2 = 0;
  const int inner = S - 2;
  const int chunks = (inner + 63) >> 6;           // 1 .. 4
  const int bands = kQualityWaves / chunks;       // 8, 4, 2, 2 (of three chunks two waves stay idle)
  const int rows = (inner + bands - 1) / bands;
  const int band = wave / chunks, x = 1 + (wave % chunks) * 64 + lane;
  const int y0 = 1 + band * rows, y1 = y0 + rows < S - 1 ? y0 + rows : S - 1;
  if (band < bands && x <= S - 2 && y0 < y1) {
    const unsigned char* col = gray + x;
    int up = col[(y0 - 1) * S], mid = col[y0 * S];
#pragma unroll 4
    for (int y = y0; y < y1; ++y) {
      const unsigned char* row = col + y * S;
      const int down = row[S];
      const int l = up + down + (int)row[-1] + (int)row[1] - 4 * mid;
      sl += l;
      sl2 += (unsigned)(l * l);
      up = mid;
      mid = down;
    }
  }
  long long v[kQualitySums] = {(long long)part.sg, (long long)part.sg2, (long long)sl, (long long)sl2, (long long)part.dark, (long long)part.bright};
#pragma unroll
  for (int c = 0; c < kQualitySums; ++c)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off);
  __syncthreads();                                // every wave is done with gray
  long long* wave_sums = (long long*)gray;        // [kQualityWaves][kQualitySums]
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kQualitySums; ++c) wave_sums[wave * kQualitySums + c] = v[c];
  }
  __syncthreads();
  if (tid == 0) {
    long long s[kQualitySums];
#pragma unroll
    for (int c = 0; c < kQualitySums; ++c) {
      s[c] = 0;
#pragma unroll
      for (int w = 0; w < kQualityWaves; ++w) s[c] += wave_sums[w * kQualitySums + c];
      stats[(size_t)blockIdx.x * kQualitySums + c] = s[c];
    }
    quality_columns(s, S, landmarks ? landmarks + (size_t)blockIdx.x * 10 : nullptr, boxes ? boxes + (size_t)blockIdx.x * 4 : nullptr, frame_h,
                    frame_w, out + (size_t)blockIdx.x * DIF_QUALITY_COLS);
  }
}

}  // namespace dif

using namespace dif;

extern "C" int dif_face_quality(const uint8_t* crops_dev, int64_t m, int size, const float* landmarks_dev, const float* boxes_dev, float frame_h,
                                float frame_w, int lo, int hi, int64_t* stats_out_dev, float* out_dev, void* stream) {
  if (size < 3 || size > kQualityMaxSize) return set_error("dif_face_quality: crop size must lie in [3, %d] (got %d)", kQualityMaxSize, size);
  if (lo < 0 || lo > 255 || hi < 0 || hi > 255) return set_error("dif_face_quality: lo and hi must lie in [0, 255] (got %d, %d)", lo, hi);
  if (m < 0 || m > 0x7fffffff) return set_error("dif_face_quality: m %lld out of range", (long long)m);
  if (m == 0) return 0;
  if (!crops_dev || !stats_out_dev || !out_dev) return set_error("dif_face_quality: null pointer");
  static_assert(sizeof(long long) == sizeof(int64_t), "stats are int64");
  size_t lds = (size_t)size * size;
  const size_t sums = sizeof(long long) * kQualityWaves * kQualitySums;
  if (lds < sums) lds = sums;
  lds = (lds + 15) & ~(size_t)15;                 // at most 64 KB: no opt-in needed
  hipLaunchKernelGGL(quality_kernel, dim3((unsigned)m), dim3(kQualityThreads), lds, (hipStream_t)stream, (const unsigned char*)crops_dev, size,
                     landmarks_dev, boxes_dev, frame_h, frame_w, lo, hi, (long long*)stats_out_dev, out_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}
