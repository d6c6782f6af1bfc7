// hipcc-flags: -ffp-contract=off
// (the box and landmark arithmetic restates tests/annotate_ref.py's float32 operation by operation, and the label's number is
// one float64 product and one sum)
// Annotation: a ring round every face of a batch of frames, a plate with its label and a square on each landmark, painted
// into the frames (include/dif.h, "annotation").  The sibling of redact.hip: opaque paint, no pixel read.
//   annotate_compose_kernel  one thread per face writes its label -- the gallery name or `unknown`, then a number -- into text.
//   annotate_paint_kernel    1 to kAnnMaxBands blocks of 4 waves per face (ann_bands); a block takes a band of rows of the face's
//                            footprint and walks the face's ten elements in their priority -- the plate, five marks, four ring strips --
//                            with the pixels of an element laid out flat over the threads, so a strip two pixels wide fills
//                            its waves as a plate does.  A pixel that a higher element of the face, or the footprint of a
//                            selected face of a lower row of the frame, paints is left to that one: the block first lists
//                            the lower faces whose footprints meet its band in LDS (by ballot, no atomics) and tests each
//                            pixel against the list.  A frame with more than kAnnListFaces lower faces tests them one by one.
//                            The face's glyph rows are staged in LDS.
// Every pixel loop is bounded by h and w, the text loops by l, the face loops by two values of offsets, the search for a
// face's frame by n.  No atomics, one writer per output byte, nothing read back.
#include <string.h>

#include "../../include/dif.h"
#include "dif_internal.hpp"
#include "font5x7.hpp"
#include "frame_rows.hpp"

namespace dif {

constexpr int kAnnThreads = 256;
constexpr int kAnnWaves = kAnnThreads / 64;
constexpr int kAnnMaxBands = 4;                  // most blocks per face
// Blocks of annotate_paint_kernel that an MI355X holds at once, which ann_bands fills and no more: 256 CUs x kAnnBlocksPerCu.
// Six per CU is the kernel's occupancy in profiles/frame_shared_resource_usage.txt: its 24 KB of LDS allow six blocks (its 49
// VGPRs would allow more).  If -Rpass-analysis=kernel-resource-usage reports another occupancy for the kernel, this constant
// and that table move with it; only the speed depends on it, never a byte of the output.
constexpr int kAnnBlocksPerCu = 6;
constexpr int kAnnResident = 256 * kAnnBlocksPerCu;
constexpr int kAnnListFaces = kAnnThreads;       // lower faces of the frame that one pass of the block can list
constexpr int kAnnElements = 10;                 // plate, 5 marks, 4 ring strips
constexpr int kNoMark = -(1 << 20);              // the centre of a mark that is not there: its square meets no frame

struct AnnRect {                                 // [x0, x1) x [y0, y1); empty when x1 <= x0 or y1 <= y0
  int x0, y0, x1, y1;
};

struct AnnFoot {                                 // what one face paints
  FrameRegion g;                                 // the box: the ring lies round it
  AnnRect plate;
  AnnRect bound;                                 // the bounding box of ring, plate and marks, unclipped
  int mx[5], my[5];
  int len;                                       // bytes of text before the first NUL
};

static_assert((kAnnThreads + 1) * sizeof(AnnFoot) * kAnnBlocksPerCu <= 160 * 1024, "kAnnBlocksPerCu blocks' lists fit a CU's LDS");

struct AnnUnknown {
  unsigned char bytes[DIF_ANNOTATE_MAX_TEXT];
  int len;
};

__device__ __forceinline__ bool ann_in(const AnnRect& a, int x, int y) { return x >= a.x0 && x < a.x1 && y >= a.y0 && y < a.y1; }

__device__ __forceinline__ void ann_grow(AnnRect* b, int x0, int y0, int x1, int y1) {
  if (x1 <= x0 || y1 <= y0) return;
  b->x0 = x0 < b->x0 ? x0 : b->x0;
  b->y0 = y0 < b->y0 ? y0 : b->y0;
  b->x1 = x1 > b->x1 ? x1 : b->x1;
  b->y1 = y1 > b->y1 ? y1 : b->y1;
}

// the bytes of a row of text before its first NUL, at most l
__device__ inline int ann_text_length(const unsigned char* __restrict__ row, int l) {
  int len = 0;
  while (len < l && row[len]) ++len;
  return len;
}

// the footprint of row r; false: the face has no region and paints nothing
__device__ inline bool ann_foot(long long r, const float* __restrict__ boxes, const float* __restrict__ landmarks,
                                const unsigned char* __restrict__ text, int l, float margin, int t, int s, int mark, int w, AnnFoot* f) {
#pragma clang fp contract(off)
  const bool marks = landmarks && mark >= 0;
  if (!frame_region(boxes + 4 * r, margin, &f->g)) return false;
  const int len = text ? ann_text_length(text + (size_t)r * (size_t)l, l) : 0;
  const FrameRegion g = f->g;
  f->bound = {1 << 30, 1 << 30, -(1 << 30), -(1 << 30)};
  if (t > 0) ann_grow(&f->bound, g.X0 - t, g.Y0 - t, g.X1 + t, g.Y1 + t);
  f->len = len;
  f->plate = {0, 0, 0, 0};
  if (len > 0) {
    const int pw = (6 * len - 1) * s + 2 * s, ph = 9 * s;    // <= 3080, 72
    int px0 = g.X0 - t;
    if (px0 + pw > w) px0 = w - pw;
    if (px0 < 0) px0 = 0;
    int py0 = g.Y0 - t - ph;
    if (py0 < 0) py0 = g.Y1 + t;
    f->plate = {px0, py0, px0 + pw, py0 + ph};
    ann_grow(&f->bound, px0, py0, px0 + pw, py0 + ph);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    f->mx[k] = kNoMark;
    f->my[k] = kNoMark;
    if (marks) {
      const float px = landmarks[(r * 5 + k) * 2], py = landmarks[(r * 5 + k) * 2 + 1];
      if (frame_finite(px) && frame_finite(py)) {
        const float sx = frame_clamp(px) + 0.5f, sy = frame_clamp(py) + 0.5f;
        const int mx = (int)__builtin_floorf(sx), my = (int)__builtin_floorf(sy);
        f->mx[k] = mx;
        f->my[k] = my;
        ann_grow(&f->bound, mx - mark, my - mark, mx + mark + 1, my + mark + 1);
      }
    }
  }
  return true;
}

__device__ __forceinline__ bool ann_in_mark(int mx, int my, int mark, int x, int y) {
  const int dx = x - mx, dy = y - my;                        // a mark that is not there is 2^20 away
  return dx >= -mark && dx <= mark && dy >= -mark && dy <= mark;
}

// does the face of footprint f paint pixel (x, y)?
__device__ inline bool ann_covers(const AnnFoot& f, int t, int mark, int x, int y) {
  if (!ann_in(f.bound, x, y)) return false;
  if (ann_in(f.plate, x, y)) return true;
  const FrameRegion& g = f.g;
  if (x >= g.X0 - t && x < g.X1 + t && y >= g.Y0 - t && y < g.Y1 + t && !(x >= g.X0 && x < g.X1 && y >= g.Y0 && y < g.Y1)) return true;
  bool hit = false;
#pragma unroll
  for (int k = 0; k < 5; ++k) hit = hit || ann_in_mark(f.mx[k], f.my[k], mark, x, y);
  return hit;
}

// element e of a face, in the order of their priority: 0 the plate, 1 .. 5 the marks, 6 .. 9 the ring's strips (top, bottom,
// left, right: disjoint)
__device__ inline AnnRect ann_element(const AnnFoot& f, int e, int t, int mark) {
  const FrameRegion& g = f.g;
  if (e == 0) return f.plate;
  if (e <= 5) {
    const int mx = f.mx[e - 1], my = f.my[e - 1];
    if (mark < 0 || mx == kNoMark) return {0, 0, 0, 0};
    return {mx - mark, my - mark, mx + mark + 1, my + mark + 1};
  }
  if (e == 6) return {g.X0 - t, g.Y0 - t, g.X1 + t, g.Y0};
  if (e == 7) return {g.X0 - t, g.Y1, g.X1 + t, g.Y1 + t};
  if (e == 8) return {g.X0 - t, g.Y0, g.X0, g.Y1};
  return {g.X1, g.Y0, g.X1 + t, g.Y1};
}

__global__ __launch_bounds__(kAnnThreads) void annotate_paint_kernel(unsigned char* __restrict__ out, long long n, long long m, int h, int w,
                                                                     const long long* __restrict__ offsets, const float* __restrict__ boxes,
                                                                     const float* __restrict__ landmarks, const unsigned char* __restrict__ text, int l,
                                                                     const unsigned char* __restrict__ colors, unsigned color,
                                                                     const unsigned char* __restrict__ select, float margin, int t, int s, int mark, int bands) {
  __shared__ AnnFoot listed[kAnnListFaces];
  __shared__ AnnFoot mine;
  __shared__ int wave_hits[kAnnWaves];
  __shared__ unsigned char glyph_rows[DIF_ANNOTATE_MAX_TEXT * 7];
  const long long i = blockIdx.x / (unsigned)bands;
  const int j = (int)(blockIdx.x % (unsigned)bands);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // every return below is taken by the whole block or by none of it
  const long long row_lo = offsets[0], row_hi = offsets[n];  // (loaded next to select[i], not behind it)
  if (select && !select[i]) return;
  if (i < row_lo || i >= row_hi) return;                     // a row that no frame covers
  long long frame, first;
  frame_of_row(i, n, offsets, &frame, &first);
  AnnFoot me;
  if (!ann_foot(i, boxes, landmarks, text, l, margin, t, s, mark, w, &me)) return;
  // the footprint's bounding box inside the frame, and the block's band of its rows
  const int cx0 = me.bound.x0 > 0 ? me.bound.x0 : 0, cx1 = me.bound.x1 < w ? me.bound.x1 : w;
  const int cy0 = me.bound.y0 > 0 ? me.bound.y0 : 0, cy1 = me.bound.y1 < h ? me.bound.y1 : h;
  if (cx1 <= cx0 || cy1 <= cy0) return;
  const int band = (cy1 - cy0 + bands - 1) / bands;
  const int y0 = cy0 + j * band, y1 = y0 + band < cy1 ? y0 + band : cy1;
  if (y0 >= y1) return;
  if (tid == 0) mine = me;
  // the face's colour and its glyph rows -- at most 64 * 7 = 448, two per thread -- are asked for here and used behind the list
  unsigned paint = color;
  if (colors) paint = (unsigned)colors[3 * i] | ((unsigned)colors[3 * i + 1] << 8) | ((unsigned)colors[3 * i + 2] << 16);
  unsigned glyph_row[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int e = tid + k * kAnnThreads;
    if (e < me.len * 7) glyph_row[k] = font5x7_row(font5x7_glyph(text[(size_t)i * (size_t)l + e / 7]), e % 7);   // me.len <= l <= 64
  }
  static_assert(2 * kAnnThreads >= DIF_ANNOTATE_MAX_TEXT * 7, "two glyph rows per thread cover a text");
  // the selected faces of lower rows of the frame: listed once when one pass of the block covers them
  const long long lower = i - first;
  const bool use_list = lower <= kAnnListFaces;
  auto lower_face = [&](long long r, AnnFoot* q) {
    return (!select || select[r]) && ann_foot(r, boxes, landmarks, text, l, margin, t, s, mark, w, q);
  };
  int n_listed = 0;
  if (use_list)
    n_listed = frame_list_lower<kAnnWaves>(tid, lane, wave, lower, first, [&](long long r, AnnFoot* q) {
      return lower_face(r, q) && q->bound.x0 < cx1 && q->bound.x1 > cx0 && q->bound.y0 < y1 && q->bound.y1 > y0;
    }, listed, wave_hits);
  // (the glyph rows go to LDS between the list and the barrier that closes both)
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (tid + k * kAnnThreads < me.len * 7) glyph_rows[tid + k * kAnnThreads] = (unsigned char)glyph_row[k];
  __syncthreads();
  const unsigned luma = 299u * (paint & 255u) + 587u * ((paint >> 8) & 255u) + 114u * ((paint >> 16) & 255u);
  const unsigned ink = luma >= 128000u ? 0u : 0xFFFFFFu;
  unsigned char* __restrict__ dst = out + (size_t)frame * (size_t)h * (size_t)w * 3;
  const int tw = (6 * mine.len - 1) * s, th = 7 * s, six_s = 6 * s;
  for (int e = 0; e < kAnnElements; ++e) {
    const AnnRect q = ann_element(mine, e, t, mark);
    const int rx0 = q.x0 > 0 ? q.x0 : 0, rx1 = q.x1 < w ? q.x1 : w;
    const int ry0 = q.y0 > y0 ? q.y0 : y0, ry1 = q.y1 < y1 ? q.y1 : y1;
    if (rx1 <= rx0 || ry1 <= ry0) continue;
    const unsigned rw = (unsigned)(rx1 - rx0), count = rw * (unsigned)(ry1 - ry0);   // <= 8192 * 8192
    const int marks_before = e <= 5 ? e - 1 : 5;
    for (unsigned p = tid; p < count; p += kAnnThreads) {
      const int y = ry0 + (int)(p / rw), x = rx0 + (int)(p % rw);
      bool taken = e > 0 && ann_in(mine.plate, x, y);        // a higher element of the face itself
      for (int k = 0; k < marks_before && !taken; ++k) taken = ann_in_mark(mine.mx[k], mine.my[k], mark, x, y);
      if (taken || frame_lower_covers(use_list, listed, n_listed, first, i, lower_face,
                                      [&](const AnnFoot& f) { return ann_covers(f, t, mark, x, y); }))
        continue;
      unsigned v = paint;
      if (e == 0) {
        const int gu = x - q.x0 - s, gv = y - q.y0 - s;
        if (gu >= 0 && gu < tw && gv >= 0 && gv < th) {
          const int col = (gu % six_s) / s;                  // column 5 is the gap between characters
          if (col < 5 && ((glyph_rows[(gu / six_s) * 7 + gv / s] >> (4 - col)) & 1u)) v = ink;
        }
      }
      unsigned char* p3 = dst + ((size_t)y * (size_t)w + (size_t)x) * 3;
      p3[0] = (unsigned char)v;
      p3[1] = (unsigned char)(v >> 8);
      p3[2] = (unsigned char)(v >> 16);
    }
  }
}

__global__ __launch_bounds__(kAnnThreads) void annotate_compose_kernel(const unsigned char* __restrict__ names, long long g, int ln,
                                                                       const long long* __restrict__ idx, const unsigned char* __restrict__ known,
                                                                       const float* __restrict__ values, int decimals, AnnUnknown unknown,
                                                                       long long m, unsigned char* __restrict__ text, int l) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kAnnThreads + threadIdx.x;
  if (i >= m) return;
  unsigned char* __restrict__ dst = text + (size_t)i * (size_t)l;
  int pos = 0;                                               // bytes of the untruncated text so far
  auto put = [&](unsigned char ch) {
    if (pos < l) dst[pos] = ch;
    ++pos;
  };
  long long row = -1;
  if (names && idx && (!known || known[i])) row = idx[i];
  if (row >= 0 && row < g) {
    const unsigned char* __restrict__ name = names + (size_t)row * (size_t)ln;
    for (int p = 0; p < ln && p < l && name[p]; ++p) put(name[p]);
  } else {
    for (int p = 0; p < unknown.len && p < l; ++p) put(unknown.bytes[p]);
  }
  if (values) {
    if (pos > 0) put(' ');
    const float v = values[i];
    if (v != v) {
      put('n');
      put('a');
      put('n');
    } else {
      const float a = __builtin_fminf(__builtin_fabsf(v), 99999.0f);
      long long p10 = 1;
      for (int d = 0; d < decimals; ++d) p10 *= 10;
      const double scaled = (double)a * (double)p10;
      const long long c = (long long)__builtin_floor(scaled + 0.5);   // <= 99999 * 10^4
      if (v < 0.0f && c > 0) put('-');
      const long long whole = c / p10, frac = c % p10;
      long long div = 1;
      while (whole / div >= 10) div *= 10;
      for (; div > 0; div /= 10) put((unsigned char)('0' + (whole / div) % 10));
      if (decimals > 0) {
        put('.');
        for (long long d = p10 / 10; d > 0; d /= 10) put((unsigned char)('0' + (frac / d) % 10));
      }
    }
  }
  while (pos < l) put(0);
}

// Blocks per face.  A block is short and most of what it costs is the chain of loads in front of its first pixel, so a call is
// fastest when all its blocks are resident at once: as many bands as keep m * bands within kAnnResident, at most kAnnMaxBands
// (few faces: their footprints are shared out) and at least one.  The bits do not depend on it: every pixel has one writer.
static int ann_bands(int64_t m) {
  const int64_t fit = kAnnResident / (m > 0 ? m : 1);
  return fit >= kAnnMaxBands ? kAnnMaxBands : (fit >= 2 ? 2 : 1);
}

}  // namespace dif

using namespace dif;

extern "C" int dif_annotate_glyph(int code, uint8_t* rows) {
  if (!rows) return set_error("dif_annotate_glyph: null pointer");
  const int glyph = font5x7_glyph(code);
  for (int r = 0; r < 7; ++r) rows[r] = (uint8_t)font5x7_row(glyph, r);
  return 0;
}

extern "C" int dif_annotate_compose(const uint8_t* names_dev, int64_t g, int ln, const int64_t* idx_dev, const uint8_t* known_dev,
                                    const float* values_dev, int decimals, const char* unknown, int64_t m, uint8_t* text_dev, int l, void* stream) {
  if (decimals < 0 || decimals > 4) return set_error("dif_annotate_compose: decimals must lie in [0, 4] (got %d)", decimals);
  if (l < 1 || l > DIF_ANNOTATE_MAX_TEXT) return set_error("dif_annotate_compose: l must lie in [1, %d] (got %d)", DIF_ANNOTATE_MAX_TEXT, l);
  if (!unknown) return set_error("dif_annotate_compose: null pointer (unknown; it may be empty)");
  AnnUnknown u;
  memset(&u, 0, sizeof(u));
  const size_t ulen = strnlen(unknown, DIF_ANNOTATE_MAX_TEXT + 1);
  if (ulen > DIF_ANNOTATE_MAX_TEXT) return set_error("dif_annotate_compose: unknown is longer than %d bytes", DIF_ANNOTATE_MAX_TEXT);
  memcpy(u.bytes, unknown, ulen);
  u.len = (int)ulen;
  if (m < 0 || m > 0x7fffffffLL) return set_error("dif_annotate_compose: m %lld out of range", (long long)m);
  if (names_dev && (g < 0 || ln < 1)) return set_error("dif_annotate_compose: names of %lld rows of %d bytes", (long long)g, ln);
  if (m == 0) return 0;
  if (!text_dev) return set_error("dif_annotate_compose: null pointer (text)");
  static_assert(sizeof(long long) == sizeof(int64_t), "idx is int64");
  const unsigned blocks = (unsigned)((m + kAnnThreads - 1) / kAnnThreads);
  hipLaunchKernelGGL(annotate_compose_kernel, dim3(blocks), dim3(kAnnThreads), 0, (hipStream_t)stream, (const unsigned char*)names_dev, (long long)g, ln,
                     (const long long*)idx_dev, (const unsigned char*)known_dev, values_dev, decimals, u, (long long)m, (unsigned char*)text_dev, l);
  DIF_HIP(hipGetLastError());
  return 0;
}

extern "C" int dif_frames_annotate(uint8_t* out_dev, int64_t n, int h, int w, const int64_t* offsets_dev, const float* boxes_dev, int64_t m,
                                   const float* landmarks_dev, const uint8_t* text_dev, int l, const uint8_t* colors_dev, const uint8_t* color,
                                   const uint8_t* select_dev, float margin, int thickness, int scale, int mark, void* stream) {
  if (h < 1 || h > DIF_REDACT_MAX_SIDE || w < 1 || w > DIF_REDACT_MAX_SIDE)
    return set_error("dif_frames_annotate: h and w must lie in [1, %d] (got %d, %d)", DIF_REDACT_MAX_SIDE, h, w);
  if (thickness < 0 || thickness > DIF_ANNOTATE_MAX_THICKNESS)
    return set_error("dif_frames_annotate: thickness must lie in [0, %d] (got %d)", DIF_ANNOTATE_MAX_THICKNESS, thickness);
  if (scale < 1 || scale > DIF_ANNOTATE_MAX_SCALE) return set_error("dif_frames_annotate: scale must lie in [1, %d] (got %d)", DIF_ANNOTATE_MAX_SCALE, scale);
  if (mark < -1 || mark > DIF_ANNOTATE_MAX_MARK) return set_error("dif_frames_annotate: mark must lie in [-1, %d] (got %d)", DIF_ANNOTATE_MAX_MARK, mark);
  if (!(__builtin_fabsf(margin) < __builtin_inff())) return set_error("dif_frames_annotate: margin must be finite");
  if (text_dev && (l < 1 || l > DIF_ANNOTATE_MAX_TEXT))
    return set_error("dif_frames_annotate: l must lie in [1, %d] (got %d)", DIF_ANNOTATE_MAX_TEXT, l);
  if (n < 0 || m < 0) return set_error("dif_frames_annotate: negative size (n %lld, m %lld)", (long long)n, (long long)m);
  if (n > 0x7fffffffLL || m * kAnnMaxBands > 0x7fffffffLL) return set_error("dif_frames_annotate: n %lld or m %lld out of range", (long long)n, (long long)m);
  if (n == 0 || m == 0) return 0;
  if (!out_dev || !offsets_dev || !boxes_dev || (!colors_dev && !color)) return set_error("dif_frames_annotate: null pointer");
  const int bands = ann_bands(m);
  const unsigned packed = color ? (unsigned)color[0] | ((unsigned)color[1] << 8) | ((unsigned)color[2] << 16) : 0u;
  hipLaunchKernelGGL(annotate_paint_kernel, dim3((unsigned)(m * bands)), dim3(kAnnThreads), 0, (hipStream_t)stream, (unsigned char*)out_dev, (long long)n,
                     (long long)m, h, w, (const long long*)offsets_dev, boxes_dev, landmarks_dev, (const unsigned char*)text_dev, text_dev ? l : 1,
                     (const unsigned char*)colors_dev, packed, (const unsigned char*)select_dev, margin, thickness, scale, mark, bands);
  DIF_HIP(hipGetLastError());
  return 0;
}
