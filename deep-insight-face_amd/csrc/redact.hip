// hipcc-flags: -ffp-contract=off
// (the box arithmetic restates tests/redact_ref.py's float32 operation by operation: margin * bw is rounded before it is added)
// Redaction: the faces of a batch of frames pixelated, smoothed or filled (include/dif.h, "redaction").
//   redact_means_kernel   pass 1, one block of 16 waves per (face, row of cells).  The waves share out the cells of the row:
//                         with fewer than 16 cells several waves take one cell, row by row in turn, so a cell of millions
//                         of pixels is summed by up to 16 waves; with more, a wave takes one cell per round.  The waves'
//                         64-bit partial sums cross through LDS and one thread per cell adds them in wave order, rounds the
//                         mean and writes three bytes in one word of the workspace.
//   redact_paint_kernel   pass 2, one block of 4 waves per (face, row of cells): a wave per pixel row, a lane per pixel.  It
//                         reads the workspace and the boxes only, never a frame, so out may be the frames.  A pixel that a
//                         selected face of a lower row of its frame covers is left to that face: the block first lists the
//                         lower faces whose region meets its band in LDS (by ballot, no atomics) and tests each pixel against
//                         the list.  A frame with more than kListFaces lower faces tests them one by one from the boxes.
// Every pixel loop is bounded by h and w, the face loops by two values of offsets, the search for a face's frame by n.
// The blocks are short, so what a call costs is mostly the chain of dependent loads in front of the first pixel: the search
// is 64-way for that reason.
// No atomics, one writer per output byte, nothing read back.
#include "../../include/dif.h"
#include "dif_internal.hpp"
#include "frame_rows.hpp"

namespace dif {

constexpr int kMeanThreads = 1024;
constexpr int kMeanWaves = kMeanThreads / 64;
constexpr int kPaintThreads = 256;
constexpr int kPaintWaves = kPaintThreads / 64;
constexpr int kListFaces = kPaintThreads;        // lower faces of the frame that one pass of the block can list

struct RedactFace {
  FrameRegion g;
  int cx0, cy0, cx1, cy1;                        // the clipped region
  int c;                                         // side of a cell
  long long frame, first;                        // the face's frame and that frame's first row
};

// is pixel (x, y) of the frame covered by the face of region g?
__device__ __forceinline__ bool redact_covers(const FrameRegion& g, int shape, int x, int y) {
  if (x < g.X0 || x >= g.X1 || y < g.Y0 || y >= g.Y1) return false;
  if (shape == 0) return true;
  const long long rw = g.X1 - g.X0, rh = g.Y1 - g.Y0;
  const long long ex = 2 * (long long)(x - g.X0) + 1 - rw, ey = 2 * (long long)(y - g.Y0) + 1 - rh;
  return rh * rh * ex * ex + rw * rw * ey * ey <= rw * rw * rh * rh;
}

// the block's face: selected, inside a frame, with a region that meets the frame?  Uniform over the block.
__device__ bool redact_face(long long i, long long n, long long m, int h, int w, const long long* __restrict__ offsets,
                            const float* __restrict__ boxes, const unsigned char* __restrict__ select, int cells, int min_cell, float margin,
                            RedactFace* face) {
  if (select && !select[i]) return false;
  if (i < offsets[0] || i >= offsets[n]) return false;       // a row that no frame covers
  frame_of_row(i, n, offsets, &face->frame, &face->first);   // the 64-way search
  if (!frame_region(boxes + 4 * i, margin, &face->g)) return false;
  const FrameRegion& g = face->g;
  face->cx0 = g.X0 > 0 ? g.X0 : 0;
  face->cy0 = g.Y0 > 0 ? g.Y0 : 0;
  face->cx1 = g.X1 < w ? g.X1 : w;
  face->cy1 = g.Y1 < h ? g.Y1 : h;
  if (face->cx1 <= face->cx0 || face->cy1 <= face->cy0) return false;
  const int rw = g.X1 - g.X0, rh = g.Y1 - g.Y0, side = rw > rh ? rw : rh;
  const int c = (side + cells - 1) / cells;
  face->c = c > min_cell ? c : min_cell;
  return true;
}

__global__ __launch_bounds__(kMeanThreads) void redact_means_kernel(const unsigned char* __restrict__ frames, long long n, long long m, int h, int w,
                                                                    const long long* __restrict__ offsets, const float* __restrict__ boxes,
                                                                    const unsigned char* __restrict__ select, int cells, int min_cell,
                                                                    float margin, unsigned* __restrict__ means) {
  __shared__ unsigned long long part[kMeanWaves][3];
  const long long i = blockIdx.x / (unsigned)cells;
  const int j = (int)(blockIdx.x % (unsigned)cells);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  RedactFace face;
  if (!redact_face(i, n, m, h, w, offsets, boxes, select, cells, min_cell, margin, &face)) return;
  const int c = face.c;
  const int top = face.g.Y0 + j * c;                         // j * c <= 63 * 16384
  const int y0 = top > face.cy0 ? top : face.cy0, y1 = top + c < face.cy1 ? top + c : face.cy1;
  if (y0 >= y1) return;                                      // the row of cells has no pixel in the frame
  const unsigned char* __restrict__ src = frames + (size_t)face.frame * (size_t)h * (size_t)w * 3;
  const int per_cell = cells >= kMeanWaves ? 1 : kMeanWaves / cells;   // waves on one cell
  const int groups = kMeanWaves / per_cell;                  // cells in flight per round
  for (int base = 0; base < cells; base += groups) {
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    const int grp = wave / per_cell, turn = wave % per_cell, ci = base + grp;
    if (grp < groups && ci < cells) {
      const int left = face.g.X0 + ci * c;
      const int x0 = left > face.cx0 ? left : face.cx0, x1 = left + c < face.cx1 ? left + c : face.cx1;
      // a cell narrower than half a wave puts 64 / width pixel rows side by side in the lanes (integer sums: any order)
      const int width = x1 - x0;
      const int rows = width > 0 && width < 64 ? 64 / width : 1;
      const int sub = rows > 1 ? lane / width : 0, xo = lane - sub * width;
      if (sub < rows) {
        for (int y = y0 + turn * rows + sub; y < y1; y += per_cell * rows) {
          const unsigned char* __restrict__ row = src + (size_t)y * (size_t)w * 3;
#pragma unroll 4
          for (int x = x0 + xo; x < x1; x += 64) {
            s0 += row[3 * x];
            s1 += row[3 * x + 1];
            s2 += row[3 * x + 2];
          }
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off);
      s1 += __shfl_xor(s1, off);
      s2 += __shfl_xor(s2, off);
    }
    if (lane == 0) {
      part[wave][0] = s0;
      part[wave][1] = s1;
      part[wave][2] = s2;
    }
    __syncthreads();
    if (tid < groups && base + tid < cells) {
      const int left = face.g.X0 + (base + tid) * c;
      const int x0 = left > face.cx0 ? left : face.cx0, x1 = left + c < face.cx1 ? left + c : face.cx1;
      if (x0 < x1) {
        const unsigned long long k = (unsigned long long)(x1 - x0) * (unsigned long long)(y1 - y0);
        unsigned v = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          unsigned long long s = 0;
          for (int p = 0; p < per_cell; ++p) s += part[tid * per_cell + p][ch];   // wave order
          v |= (unsigned)((2 * s + k) / (2 * k)) << (8 * ch);
        }
        means[((size_t)i * cells + j) * cells + base + tid] = v;
      }
    }
    __syncthreads();
  }
}

// (num + den / 2) / den for num <= 255 * den, den = 4 c^2 <= 2^30: the quotient fits a byte, so a float estimate is within one of it
__device__ __forceinline__ unsigned redact_round_div(unsigned long long num, unsigned den) {
  const unsigned long long t = num + (den >> 1);
  unsigned q = (unsigned)((float)t / (float)den);
  if ((unsigned long long)q * den > t) --q;
  else if ((unsigned long long)(q + 1) * den <= t) ++q;
  return q;
}

__global__ __launch_bounds__(kPaintThreads) void redact_paint_kernel(unsigned char* __restrict__ out, long long n, long long m, int h, int w,
                                                                     const long long* __restrict__ offsets, const float* __restrict__ boxes,
                                                                     const unsigned char* __restrict__ select, int mode, int shape, int cells,
                                                                     int min_cell, float margin, unsigned fill,
                                                                     const unsigned* __restrict__ means) {
  __shared__ FrameRegion listed[kListFaces];
  __shared__ int wave_hits[kPaintWaves];
  const long long i = blockIdx.x / (unsigned)cells;
  const int j = (int)(blockIdx.x % (unsigned)cells);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  RedactFace face;
  if (!redact_face(i, n, m, h, w, offsets, boxes, select, cells, min_cell, margin, &face)) return;
  const FrameRegion g = face.g;
  const int c = face.c;
  const int top = g.Y0 + j * c;
  const int y0 = top > face.cy0 ? top : face.cy0, y1 = top + c < face.cy1 ? top + c : face.cy1;
  if (y0 >= y1) return;
  // the selected faces of lower rows of the frame: listed once when one pass of the block covers them
  const long long lower = i - face.first;
  const bool use_list = lower <= kListFaces;
  auto lower_face = [&](long long r, FrameRegion* q) { return (!select || select[r]) && frame_region(boxes + 4 * r, margin, q); };
  int n_listed = 0;
  if (use_list) {
    n_listed = frame_list_lower<kPaintWaves>(tid, lane, wave, lower, face.first, [&](long long r, FrameRegion* q) {
      return lower_face(r, q) && q->X0 < face.cx1 && q->X1 > face.cx0 && q->Y0 < y1 && q->Y1 > y0;
    }, listed, wave_hits);
    __syncthreads();
  }
  unsigned char* __restrict__ dst = out + (size_t)face.frame * (size_t)h * (size_t)w * 3;
  const unsigned* __restrict__ mine = means + (size_t)i * cells * cells;
  const int two_c = 2 * c;
  const unsigned den = 4u * (unsigned)c * (unsigned)c;       // <= 2^30
  // smooth: the cells that meet the frame
  const int ilo = (face.cx0 - g.X0) / c, ihi = (face.cx1 - 1 - g.X0) / c;
  const int jlo = (face.cy0 - g.Y0) / c, jhi = (face.cy1 - 1 - g.Y0) / c;
  for (int y = y0 + wave; y < y1; y += kPaintWaves) {
    const int dy = y - g.Y0;
    int j0 = j, j1 = j;
    unsigned fb = 0;
    if (mode == 2) {
      const int b = 2 * dy + 1 - c;                          // >= 1 - c: floor(b / 2c) is -1 below 0
      const int jf = b < 0 ? -1 : b / two_c;
      fb = (unsigned)(b - two_c * jf);
      j0 = jf < jlo ? jlo : (jf > jhi ? jhi : jf);
      j1 = jf + 1 < jlo ? jlo : (jf + 1 > jhi ? jhi : jf + 1);
    }
    for (int x = face.cx0 + lane; x < face.cx1; x += 64) {
      if (!redact_covers(g, shape, x, y)) continue;
      if (frame_lower_covers(use_list, listed, n_listed, face.first, i, lower_face,
                             [&](const FrameRegion& q) { return redact_covers(q, shape, x, y); }))
        continue;
      const int dx = x - g.X0;
      unsigned v;
      if (mode == 0) {
        v = fill;
      } else if (mode == 1) {
        v = mine[j * cells + dx / c];
      } else {
        const int a = 2 * dx + 1 - c;
        const int jf = a < 0 ? -1 : a / two_c;
        const unsigned fa = (unsigned)(a - two_c * jf);
        const int i0 = jf < ilo ? ilo : (jf > ihi ? ihi : jf);
        const int i1 = jf + 1 < ilo ? ilo : (jf + 1 > ihi ? ihi : jf + 1);
        const unsigned v00 = mine[j0 * cells + i0], v01 = mine[j0 * cells + i1];
        const unsigned v10 = mine[j1 * cells + i0], v11 = mine[j1 * cells + i1];
        const unsigned ga = (unsigned)two_c - fa, gb = (unsigned)two_c - fb;
        const unsigned w00 = ga * gb, w01 = fa * gb, w10 = ga * fb, w11 = fa * fb;   // each <= 4 c^2 <= 2^30
        v = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const unsigned long long sum = (unsigned long long)w00 * ((v00 >> (8 * ch)) & 255u) + (unsigned long long)w01 * ((v01 >> (8 * ch)) & 255u) +
                                         (unsigned long long)w10 * ((v10 >> (8 * ch)) & 255u) + (unsigned long long)w11 * ((v11 >> (8 * ch)) & 255u);
          v |= redact_round_div(sum, den) << (8 * ch);
        }
      }
      unsigned char* p = dst + ((size_t)y * (size_t)w + (size_t)x) * 3;
      p[0] = (unsigned char)v;
      p[1] = (unsigned char)(v >> 8);
      p[2] = (unsigned char)(v >> 16);
    }
  }
}

}  // namespace dif

using namespace dif;

extern "C" int64_t dif_frames_redact_workspace_size(int64_t m, int cells) {
  if (m < 0 || m > 0x7fffffffLL || cells < 1 || cells > DIF_REDACT_MAX_CELLS || m * cells > 0x7fffffffLL) return -1;
  return m * cells * cells * 4;
}

extern "C" int dif_frames_redact(const uint8_t* frames_dev, int64_t n, int h, int w, const int64_t* offsets_dev, const float* boxes_dev, int64_t m,
                                 const uint8_t* select_dev, int mode, int shape, int cells, int min_cell, float margin, const uint8_t* fill,
                                 uint8_t* out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  if (h < 1 || h > DIF_REDACT_MAX_SIDE || w < 1 || w > DIF_REDACT_MAX_SIDE)
    return set_error("dif_frames_redact: h and w must lie in [1, %d] (got %d, %d)", DIF_REDACT_MAX_SIDE, h, w);
  if (cells < 1 || cells > DIF_REDACT_MAX_CELLS) return set_error("dif_frames_redact: cells must lie in [1, %d] (got %d)", DIF_REDACT_MAX_CELLS, cells);
  if (min_cell < 1 || min_cell > DIF_REDACT_MAX_SIDE)
    return set_error("dif_frames_redact: min_cell must lie in [1, %d] (got %d)", DIF_REDACT_MAX_SIDE, min_cell);
  if (mode < 0 || mode > 2) return set_error("dif_frames_redact: mode must be 0 (fill), 1 (pixelate) or 2 (smooth) (got %d)", mode);
  if (shape < 0 || shape > 1) return set_error("dif_frames_redact: shape must be 0 (box) or 1 (ellipse) (got %d)", shape);
  if (!(__builtin_fabsf(margin) < __builtin_inff())) return set_error("dif_frames_redact: margin must be finite");
  if (n < 0 || m < 0) return set_error("dif_frames_redact: negative size (n %lld, m %lld)", (long long)n, (long long)m);
  const int64_t need = dif_frames_redact_workspace_size(m, cells);
  if (need < 0 || n > 0x7fffffffLL) return set_error("dif_frames_redact: n %lld or m %lld out of range", (long long)n, (long long)m);
  if (n == 0 || m == 0) return 0;
  if (!frames_dev || !offsets_dev || !boxes_dev || !fill || !out_dev || !workspace_dev) return set_error("dif_frames_redact: null pointer");
  if (workspace_bytes < need)
    return set_error("dif_frames_redact: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  if ((uintptr_t)workspace_dev & 3u) return set_error("dif_frames_redact: workspace not aligned to 4 bytes");
  const uintptr_t bytes = (uintptr_t)n * (uintptr_t)h * (uintptr_t)w * 3, src = (uintptr_t)frames_dev, dst = (uintptr_t)out_dev;
  if (src != dst && src < dst + bytes && dst < src + bytes) return set_error("dif_frames_redact: out overlaps frames in part");
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are int64");
  const unsigned blocks = (unsigned)(m * cells);
  const hipStream_t st = (hipStream_t)stream;
  if (mode != 0) {
    hipLaunchKernelGGL(redact_means_kernel, dim3(blocks), dim3(kMeanThreads), 0, st, (const unsigned char*)frames_dev, (long long)n, (long long)m, h, w,
                       (const long long*)offsets_dev, boxes_dev, (const unsigned char*)select_dev, cells, min_cell, margin, (unsigned*)workspace_dev);
    DIF_HIP(hipGetLastError());
  }
  const unsigned packed = (unsigned)fill[0] | ((unsigned)fill[1] << 8) | ((unsigned)fill[2] << 16);
  hipLaunchKernelGGL(redact_paint_kernel, dim3(blocks), dim3(kPaintThreads), 0, st, (unsigned char*)out_dev, (long long)n, (long long)m, h, w,
                     (const long long*)offsets_dev, boxes_dev, (const unsigned char*)select_dev, mode, shape, cells, min_cell, margin, packed,
                     (const unsigned*)workspace_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}
