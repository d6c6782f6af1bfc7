// hipcc-flags: -ffp-contract=off
// (det_overlap restates the reference's float64 arithmetic operation by operation: a product is rounded before it is added)
// Detector evaluation: the detections of a batch of frames matched to the ground truth, and the precision / recall curve
// and the average precision of all detections seen (include/dif.h, "detector evaluation").  The rule is that of the
// consumers of the reference's detector/utility.py compute_overlap and compute_ap (keras-retinanet / keras-yolo3
// `evaluate`), with Pascal VOC's "difficult" flags:
//   overlap  compute_overlap in float64 on the float32 coordinates: no +1, the union clamped below at DBL_EPSILON.  A pair
//            with a coordinate that is not finite has overlap 0 (the reference: NaN).
//   best     assigned[d] = the first maximum of d's overlaps with the truths of its frame (np.argmax), -1 in a frame
//            without truths; iou[d] = that maximum, 0 without one.  Neither looks at a threshold.
//   order    descending score, ties to the lower row, NaN last (np.argsort(-scores, kind='stable')).
//   outcome  per threshold j, a frame's detections in that order: assigned < 0 or iou < thr[j] -> 0 (false positive); else
//            the truth is ignored -> 2 (dropped: neither); else the truth is free -> 1 (true positive), and it is taken;
//            else 0.  A detection never falls through to its second-best truth, so it has ONE candidate truth, and the
//            true positive of a truth is the first in order of the detections that are eligible for it: claim[j][g] =
//            the least rank among them (an integer atomicMin, whose result knows no order), outcome 1 iff rank == claim.
//            The rank of ONE sort over the batch serves every frame: restricted to a frame it is the frame's order.
//   curve    over all detections in order: tp_cum / fp_cum inclusive counts of outcomes 1 / 0, recall = tp_cum / n_truth
//            (0 with n_truth = 0: the non-ignored truths), precision = tp_cum / max(tp_cum + fp_cum, DBL_EPSILON).
//   ap       compute_ap: sentinels, the envelope (reverse running maximum), the sum of (step of recall) x envelope.
// Kernels:
//   det_overlap_kernel    one thread per pair (dif_box_overlap)
//   det_best_kernel       one thread per detection over the truths of its frame; a block whose detections share a frame
//                         stages that frame's truths through LDS, kDetGtChunk at a time
//   det_keys_kernel       (monotone uint32 key of the score, row) pairs, which the stable LSD radix sort of
//                         csrc/radix_sort.hip orders in four 8-bit passes (radix_sort_run without a plan)
//   det_truth_kernel      claim <- none, n_truth
//   det_claim_kernel, det_classify_kernel    the outcome rule above
//   det_count_kernel      } the J scans in reduce / scan / apply form: per tile of kDetScanTile ranks the counts, one wave
//   det_count_scan_kernel } per threshold turns them into the counts in front of each tile, and every tile scans itself
//   det_apply_kernel      } again on top of that and writes the four curves
//   det_tile_max_kernel   } the envelope and the sum likewise: per tile the maximum, one wave per threshold turns them
//   det_carry_kernel      } into the maximum behind each tile, every tile takes the envelope from there and sums its
//   det_tile_ap_kernel    } terms, and one wave adds the tiles' sums, last tile first
//   det_ap_sum_kernel     }
//   det_ap_kernel         dif_det_ap on a curve of the caller's: ONE block walks the tiles last to first with the same
//                         tile body, the same bits as the four above
// No block waits for another: every hand-off between blocks is the end of a launch.  The only atomics are the integer
// minimum of the claim and the integer sum of n_truth; every output is a function of the input alone.
#include "../../include/dif.h"
#include "dif_internal.hpp"
#include "frame_rows.hpp"

namespace dif {

constexpr int kDetThreads = 256;
constexpr int kDetWaves = kDetThreads / 64;
constexpr int kDetGtChunk = 256;                            // truths of a frame in LDS at a time: one per thread
constexpr int kDetScanItems = 4;                            // ranks per thread: thread t holds ranks [4 t, 4 t + 4) of its tile
constexpr int kDetScanTile = DIF_DET_SCAN_TILE;
static_assert(kDetScanTile == kDetThreads * kDetScanItems, "DIF_DET_SCAN_TILE");
constexpr int kDetNoClaim = 0x7fffffff;
constexpr double kDetEps = 2.220446049250313e-16;           // np.finfo(float).eps

struct DetThr {
  double v[DIF_DET_MAX_THRESHOLDS];
};

// np.maximum / np.minimum on numbers: the first operand unless the second is strictly greater / less
__device__ __forceinline__ double det_max(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double det_min(double a, double b) { return a < b ? a : b; }
// np.maximum as compute_ap uses it: a NaN on either side is the result
__device__ __forceinline__ double det_npmax(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

__device__ __forceinline__ bool det_load_box(const float* __restrict__ p, double* q) {
  const float x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
  q[0] = x0, q[1] = x1, q[2] = x2, q[3] = x3;
  return __builtin_isfinite(x0) && __builtin_isfinite(x1) && __builtin_isfinite(x2) && __builtin_isfinite(x3);
}

// compute_overlap for one pair of finite boxes: a the detection, b the truth
__device__ __forceinline__ double det_overlap(const double* a, const double* b) {
#pragma clang fp contract(off)
  const double area = (b[2] - b[0]) * (b[3] - b[1]);
  double iw = det_min(a[2], b[2]) - det_max(a[0], b[0]);
  double ih = det_min(a[3], b[3]) - det_max(a[1], b[1]);
  iw = det_max(iw, 0.0);
  ih = det_max(ih, 0.0);
  double ua = (a[2] - a[0]) * (a[3] - a[1]) + area - iw * ih;
  ua = det_max(ua, kDetEps);
  return iw * ih / ua;
}

__global__ __launch_bounds__(kDetThreads) void det_overlap_kernel(const float* __restrict__ a, int64_t n, const float* __restrict__ b, int64_t k,
                                                                  double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kDetThreads + threadIdx.x;
  if (i >= n * k) return;
  const int64_t r = i / k, c = i - r * k;
  double qa[4], qb[4];
  const bool fa = det_load_box(a + r * 4, qa), fb = det_load_box(b + c * 4, qb);
  out[i] = fa && fb ? det_overlap(qa, qb) : 0.0;
}

__global__ __launch_bounds__(kDetThreads) void det_best_kernel(const int64_t* __restrict__ doff, const int64_t* __restrict__ goff, int64_t n,
                                                               const float* __restrict__ dbox, int64_t m, const float* __restrict__ gbox,
                                                               int64_t t, int* __restrict__ assigned, double* __restrict__ iou) {
  __shared__ double sg[kDetGtChunk][4];
  __shared__ int sfin[kDetGtChunk];
  const int tid = threadIdx.x;
  const int64_t d0 = (int64_t)blockIdx.x * kDetThreads, d = d0 + tid;
  const bool live = d < m;
  const int64_t dd = live ? d : m - 1;          // a thread past the end walks with the last row and writes nothing
  const int64_t f = frame_bisect(doff, n, dd);
  int64_t b, e, gb = 0, ge = 0;
  frame_rows(doff, f, m, &b, &e);
  const bool in = dd >= b && dd < e;            // (false only when offsets is no prefix sum: the row is in no frame)
  if (in) frame_rows(goff, f, t, &gb, &ge);
  const int64_t f0 = frame_bisect(doff, n, d0);
  const int shared = __syncthreads_and(in && f == f0);     // the block's detections share a frame: gb, ge are uniform
  double a[4];
  const bool fa = det_load_box(dbox + dd * 4, a);
  double best = -1.0;
  int64_t arg = -1;
  if (shared) {
    for (int64_t c = gb; c < ge; c += kDetGtChunk) {
      const int cnt = ge - c < kDetGtChunk ? (int)(ge - c) : kDetGtChunk;
      __syncthreads();                          // the chunk before has been read
      if (tid < cnt) sfin[tid] = det_load_box(gbox + (c + tid) * 4, sg[tid]);
      __syncthreads();
      for (int k = 0; k < cnt; ++k) {
        const double ov = fa && sfin[k] ? det_overlap(a, sg[k]) : 0.0;
        if (ov > best) best = ov, arg = c + k;  // (strictly: the first maximum stays)
      }
    }
  } else {
    for (int64_t g = gb; g < ge; ++g) {
      double q[4];
      const bool fg = det_load_box(gbox + g * 4, q);
      const double ov = fa && fg ? det_overlap(a, q) : 0.0;
      if (ov > best) best = ov, arg = g;
    }
  }
  if (live) {
    assigned[d] = (int)arg;
    iou[d] = arg >= 0 ? best : 0.0;
  }
}

// ---- the order: ascending key = descending score, -0 = +0, every NaN the one key above all others
__global__ __launch_bounds__(kDetThreads) void det_keys_kernel(const float* __restrict__ scores, int m, unsigned* __restrict__ keys,
                                                               int* __restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * kDetThreads + threadIdx.x;
  if (i >= m) return;
  const float s = scores[i];
  unsigned u = __float_as_uint(s);
  if (s == 0.f) u = 0u;
  const unsigned mono = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);     // ascending with the score
  keys[i] = s != s ? 0xffffffffu : ~mono;       // (~mono = 0xffffffff takes a NaN's bits: no number shares the key)
  pos[i] = (int)i;
}

// the sorted rows -> rank_out[row] = rank (dif_det_match) and / or order_out[rank] = row (dif_det_curve)
__global__ __launch_bounds__(kDetThreads) void det_rank_kernel(const int* __restrict__ pos, int m, int* __restrict__ rank_out,
                                                               int64_t* __restrict__ order_out) {
  const int64_t i = (int64_t)blockIdx.x * kDetThreads + threadIdx.x;
  if (i >= m) return;
  const int row = pos[i];
  if (rank_out) rank_out[row] = (int)i;
  if (order_out) order_out[i] = row;
}

// ---- claim and classify
__global__ __launch_bounds__(kDetThreads) void det_truth_kernel(const uint8_t* __restrict__ ignore, int64_t t, int J, int* __restrict__ claim,
                                                                unsigned long long* __restrict__ n_truth) {
  __shared__ int wave_total[kDetWaves];
  const int64_t g = (int64_t)blockIdx.x * kDetThreads + threadIdx.x;
  int live = 0;
  if (g < t) {
    live = !(ignore && ignore[g]);
    for (int j = 0; j < J; ++j) claim[(int64_t)j * t + g] = kDetNoClaim;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) live += __shfl_xor(live, off);
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = live;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kDetWaves; ++w) s += wave_total[w];
    if (s) atomicAdd(n_truth, (unsigned long long)s);
  }
}

__global__ __launch_bounds__(kDetThreads) void det_claim_kernel(const int* __restrict__ assigned, const double* __restrict__ iou,
                                                                const int* __restrict__ rank, const uint8_t* __restrict__ ignore, int m,
                                                                int64_t t, const DetThr thr, int J, int* __restrict__ claim) {
  const int64_t d = (int64_t)blockIdx.x * kDetThreads + threadIdx.x;
  if (d >= m) return;
  const int g = assigned[d];
  if (g < 0 || (ignore && ignore[g])) return;
  const double v = iou[d];
  const int r = rank[d];
  for (int j = 0; j < J; ++j)
    if (v >= thr.v[j]) atomicMin(&claim[(int64_t)j * t + g], r);
}

__global__ __launch_bounds__(kDetThreads) void det_classify_kernel(const int* __restrict__ assigned, const double* __restrict__ iou,
                                                                   const int* __restrict__ rank, const uint8_t* __restrict__ ignore, int m,
                                                                   int64_t t, const DetThr thr, int J, const int* __restrict__ claim,
                                                                   uint8_t* __restrict__ outcome) {
  const int64_t d = (int64_t)blockIdx.x * kDetThreads + threadIdx.x;
  if (d >= m) return;
  const int g = assigned[d];
  const bool ign = g >= 0 && ignore && ignore[g];
  const double v = iou[d];
  const int r = rank[d];
  for (int j = 0; j < J; ++j) {
    uint8_t o = DIF_DET_FP;
    if (g >= 0 && v >= thr.v[j]) o = ign ? DIF_DET_DROPPED : (claim[(int64_t)j * t + g] == r ? DIF_DET_TP : DIF_DET_FP);
    outcome[(int64_t)j * m + d] = o;
  }
}

// ---- the counts.  Block (tile, j); thread t holds ranks tile * kDetScanTile + 4 t .. + 3.
__device__ __forceinline__ void det_flags(const uint8_t* __restrict__ outcome, const int* __restrict__ pos, int64_t i0, int m, int* tp, int* fp) {
#pragma unroll
  for (int r = 0; r < kDetScanItems; ++r) {
    const int64_t i = i0 + r;
    const int o = i < m ? outcome[pos[i]] : DIF_DET_DROPPED;
    tp[r] = o == DIF_DET_TP;
    fp[r] = o == DIF_DET_FP;
  }
}

__global__ __launch_bounds__(kDetThreads) void det_count_kernel(const uint8_t* __restrict__ outcome, const int* __restrict__ pos, int m, int nt,
                                                                int64_t* __restrict__ part) {
  __shared__ int wtp[kDetWaves], wfp[kDetWaves];
  const int tid = threadIdx.x, j = blockIdx.y;
  int tp[kDetScanItems], fp[kDetScanItems];
  det_flags(outcome + (int64_t)j * m, pos, (int64_t)blockIdx.x * kDetScanTile + tid * kDetScanItems, m, tp, fp);
  int a = tp[0] + tp[1] + tp[2] + tp[3], b = fp[0] + fp[1] + fp[2] + fp[3];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off), b += __shfl_xor(b, off);
  if ((tid & 63) == 0) wtp[tid >> 6] = a, wfp[tid >> 6] = b;
  __syncthreads();
  if (tid == 0) {
    int64_t* q = part + ((int64_t)j * nt + blockIdx.x) * 2;
    q[0] = wtp[0] + wtp[1] + wtp[2] + wtp[3];
    q[1] = wfp[0] + wfp[1] + wfp[2] + wfp[3];
  }
}

// One wave per threshold: part[j][tile] <- the counts of the tiles in front of it.  A lane sums a contiguous share of the
// tiles, the shares are scanned across the wave, and the lane rewrites its share.
__global__ __launch_bounds__(64) void det_count_scan_kernel(int64_t* __restrict__ part, int nt) {
  int64_t* q = part + (int64_t)blockIdx.x * nt * 2;
  const int lane = threadIdx.x;
  const int per = (nt + 63) / 64;
  const int lo = lane * per < nt ? lane * per : nt, hi = lo + per < nt ? lo + per : nt;
  int64_t a = 0, b = 0;
  for (int i = lo; i < hi; ++i) a += q[2 * i], b += q[2 * i + 1];
  int64_t ia = a, ib = b;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t va = __shfl_up(ia, off), vb = __shfl_up(ib, off);
    if (lane >= off) ia += va, ib += vb;
  }
  int64_t ra = ia - a, rb = ib - b;
  for (int i = lo; i < hi; ++i) {
    const int64_t va = q[2 * i], vb = q[2 * i + 1];
    q[2 * i] = ra, q[2 * i + 1] = rb;
    ra += va, rb += vb;
  }
}

__global__ __launch_bounds__(kDetThreads) void det_apply_kernel(const uint8_t* __restrict__ outcome, const int* __restrict__ pos, int m, int nt,
                                                                const int64_t* __restrict__ part, const int64_t* __restrict__ n_truth,
                                                                int64_t* __restrict__ tp_cum, int64_t* __restrict__ fp_cum,
                                                                double* __restrict__ recall, double* __restrict__ precision) {
  __shared__ int wtp[kDetWaves], wfp[kDetWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * kDetScanTile + tid * kDetScanItems;
  int tp[kDetScanItems], fp[kDetScanItems];
  det_flags(outcome + (int64_t)j * m, pos, i0, m, tp, fp);
  const int a = tp[0] + tp[1] + tp[2] + tp[3], b = fp[0] + fp[1] + fp[2] + fp[3];
  int ia = a, ib = b;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int va = __shfl_up(ia, off), vb = __shfl_up(ib, off);
    if (lane >= off) ia += va, ib += vb;
  }
  if (lane == 63) wtp[wave] = ia, wfp[wave] = ib;
  __syncthreads();
  const int64_t* q = part + ((int64_t)j * nt + blockIdx.x) * 2;
  int64_t ra = q[0] + (ia - a), rb = q[1] + (ib - b);
  for (int w = 0; w < wave; ++w) ra += wtp[w], rb += wfp[w];
  const int64_t nt_all = n_truth[0];
  const double den = (double)nt_all;
#pragma unroll
  for (int r = 0; r < kDetScanItems; ++r) {
    const int64_t i = i0 + r;
    if (i >= m) break;
    ra += tp[r], rb += fp[r];
    const int64_t o = (int64_t)j * m + i;
    tp_cum[o] = ra;
    fp_cum[o] = rb;
    recall[o] = nt_all > 0 ? (double)ra / den : 0.0;
    precision[o] = (double)ra / det_max((double)(ra + rb), kDetEps);
  }
}

// ---- compute_ap.  mrec = [0, recall, 1], mpre = [0, precision, 0]; the envelope at i is the maximum of precision[i ..] and
// the sentinel 0; the sum takes (recall[i] - recall[i - 1]) * envelope[i] where the two differ (recall[-1] = 0), and the step
// to the sentinel 1, whose envelope is the sentinel 0.
// One tile: `carry` = the envelope behind the tile.  Returns the sum of the tile's terms -- a thread's four in order, the
// lanes of a wave by the butterfly, the four waves in order: a fixed order -- and the tile's own maximum, to every thread.
__device__ __forceinline__ void det_ap_tile(const double* __restrict__ rec, const double* __restrict__ pre, int64_t m, int64_t tile, double carry,
                                            bool want_sum, double* sum_out, double* max_out) {
  __shared__ double wmax[kDetWaves], wsum[kDetWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = tile * kDetScanTile + tid * kDetScanItems;
  const double ninf = -__builtin_inf();
  double p[kDetScanItems];
#pragma unroll
  for (int r = 0; r < kDetScanItems; ++r) p[r] = i0 + r < m ? pre[i0 + r] : ninf;
  // the maximum of the thread's items, then of the threads behind it: inclusive over the lanes from the right
  double mine = det_npmax(det_npmax(p[0], p[1]), det_npmax(p[2], p[3]));
  double inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double v = __shfl_down(inc, off);
    if (lane + off < 64) inc = det_npmax(inc, v);
  }
  __syncthreads();                              // (a block that walks several tiles: the tile before has been read)
  if (lane == 0) wmax[wave] = inc;
  __syncthreads();
  double behind = __shfl_down(inc, 1);          // the lanes behind this one ...
  if (lane == 63) behind = ninf;
  for (int w = kDetWaves - 1; w > wave; --w) behind = det_npmax(behind, wmax[w]);   // ... and the waves
  *max_out = det_npmax(det_npmax(wmax[0], wmax[1]), det_npmax(wmax[2], wmax[3]));
  if (!want_sum) return;
  double env = det_npmax(behind, carry), s = 0.0, term[kDetScanItems];
#pragma unroll
  for (int r = kDetScanItems - 1; r >= 0; --r) {
    term[r] = 0.0;
    const int64_t i = i0 + r;
    if (i < m) {
      env = det_npmax(p[r], env);
      const double cur = rec[i], prev = i > 0 ? rec[i - 1] : 0.0;
      if (cur != prev) term[r] = (cur - prev) * env;
    }
  }
#pragma unroll
  for (int r = 0; r < kDetScanItems; ++r) s += term[r];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) wsum[wave] = s;
  __syncthreads();
  *sum_out = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// the step to the sentinel: (1 - recall[m - 1]) * 0 where the two differ; an empty curve steps from 0 to 1
__device__ __forceinline__ double det_ap_last(const double* __restrict__ rec, int64_t m) {
  const double last = m > 0 ? rec[m - 1] : 0.0;
  return 1.0 != last ? (1.0 - last) * 0.0 : 0.0;
}

__global__ __launch_bounds__(kDetThreads) void det_tile_max_kernel(const double* __restrict__ precision, int64_t m, int nt, double* __restrict__ tmax) {
  double s, mx;
  det_ap_tile(nullptr, precision + (int64_t)blockIdx.y * m, m, blockIdx.x, 0.0, false, &s, &mx);
  if (threadIdx.x == 0) tmax[(int64_t)blockIdx.y * nt + blockIdx.x] = mx;
}

// One wave per threshold: tmax[j][tile] <- the envelope behind the tile (the maximum of the tiles behind it and the sentinel)
__global__ __launch_bounds__(64) void det_carry_kernel(double* __restrict__ tmax, int nt) {
  double* q = tmax + (int64_t)blockIdx.x * nt;
  const int lane = threadIdx.x;
  const int per = (nt + 63) / 64;
  const int lo = lane * per < nt ? lane * per : nt, hi = lo + per < nt ? lo + per : nt;
  const double ninf = -__builtin_inf();
  double mine = ninf;
  for (int i = lo; i < hi; ++i) mine = det_npmax(mine, q[i]);
  double inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double v = __shfl_down(inc, off);
    if (lane + off < 64) inc = det_npmax(inc, v);
  }
  double run = __shfl_down(inc, 1);
  if (lane == 63) run = ninf;
  run = det_npmax(run, 0.0);
  for (int i = hi - 1; i >= lo; --i) {
    const double v = q[i];
    q[i] = run;
    run = det_npmax(v, run);
  }
}

__global__ __launch_bounds__(kDetThreads) void det_tile_ap_kernel(const double* __restrict__ recall, const double* __restrict__ precision, int64_t m,
                                                                  int nt, const double* __restrict__ carry, double* __restrict__ tsum) {
  const int64_t o = (int64_t)blockIdx.y * nt + blockIdx.x;
  double s, mx;
  det_ap_tile(recall + (int64_t)blockIdx.y * m, precision + (int64_t)blockIdx.y * m, m, blockIdx.x, carry[o], true, &s, &mx);
  if (threadIdx.x == 0) tsum[o] = s;
}

// One wave per threshold: the step to the sentinel, then the tiles' sums, last tile first -- the order of det_ap_kernel.
__global__ __launch_bounds__(64) void det_ap_sum_kernel(const double* __restrict__ recall, int64_t m, int nt, const double* __restrict__ tsum,
                                                        double* __restrict__ ap) {
  const double* q = tsum + (int64_t)blockIdx.x * nt;
  const int lane = threadIdx.x;
  double acc = det_ap_last(recall + (int64_t)blockIdx.x * m, m);
  for (int hi = nt; hi > 0; hi -= 64) {         // tiles [hi - 64, hi): lane l holds tile hi - 64 + l
    const int i = hi - 64 + lane;
    const double v = i >= 0 ? q[i] : 0.0;
    const int first = hi < 64 ? 64 - hi : 0;
    for (int l = 63; l >= first; --l) acc += __shfl(v, l);
  }
  if (lane == 0) ap[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kDetThreads) void det_ap_kernel(const double* __restrict__ recall, const double* __restrict__ precision, int64_t m,
                                                             double* __restrict__ ap) {
  double acc = det_ap_last(recall, m), carry = 0.0;
  for (int64_t tile = (m + kDetScanTile - 1) / kDetScanTile - 1; tile >= 0; --tile) {
    double s, mx;
    det_ap_tile(recall, precision, m, tile, carry, true, &s, &mx);
    acc += s;
    carry = det_npmax(mx, carry);
  }
  if (threadIdx.x == 0) ap[0] = acc;
}

}  // namespace dif

using namespace dif;

struct DetWork {
  unsigned *k0, *k1, *hist;
  int *p0, *p1, *rank, *claim;
  int64_t* part;
  double *tmax, *tsum;
};

static int64_t det_blocks(int64_t items, int per) { return (items + per - 1) / per; }

static size_t det_carve(void* base, int64_t m, int64_t t, int J, DetWork* w) {
  Carver c(base);
  const size_t nt = (size_t)det_blocks(m, kDetScanTile);
  w->k0 = (unsigned*)c.take((size_t)m * 4);
  w->k1 = (unsigned*)c.take((size_t)m * 4);
  w->p0 = (int*)c.take((size_t)m * 4);
  w->p1 = (int*)c.take((size_t)m * 4);
  w->hist = (unsigned*)c.take(radix_sort_hist_bytes(m));
  w->rank = (int*)c.take((size_t)m * 4);
  w->claim = (int*)c.take((size_t)J * (size_t)t * 4);
  w->part = (int64_t*)c.take((size_t)J * nt * 16);
  w->tmax = (double*)c.take((size_t)J * nt * 8);
  w->tsum = (double*)c.take((size_t)J * nt * 8);
  return c.at;
}

static int det_check_sizes(const char* fn, int64_t m, int64_t t, int J) {
  if (m < 0 || m > DIF_DET_MAX_ROWS || t < 0 || t > DIF_DET_MAX_ROWS)
    return set_error("%s: sizes out of range (%lld detections, %lld truths; at most %d each)", fn, (long long)m, (long long)t, DIF_DET_MAX_ROWS);
  if (J < 1 || J > DIF_DET_MAX_THRESHOLDS) return set_error("%s: %d thresholds outside [1, %d]", fn, J, DIF_DET_MAX_THRESHOLDS);
  return 0;
}

// the rows of scores[0 .. m) in order -> w.p0 (m > 0)
static int det_sort(const float* scores_dev, int64_t m, const DetWork& w, hipStream_t st) {
  hipLaunchKernelGGL(det_keys_kernel, dim3((unsigned)det_blocks(m, kDetThreads)), dim3(kDetThreads), 0, st, scores_dev, (int)m, w.k0, w.p0);
  return radix_sort_run<unsigned>(nullptr, 4, w.k0, w.k1, w.p0, w.p1, m, w.hist, st);   // (four passes: the sorted pairs are back in k0 / p0)
}

extern "C" {

int dif_box_overlap(const float* a_dev, int64_t n, const float* b_dev, int64_t k, double* out_dev, void* stream) {
  const char* fn = "dif_box_overlap";
  if (n < 0 || k < 0 || n > DIF_DET_MAX_ROWS || k > DIF_DET_MAX_ROWS || (n > 0 && k > 0x7fffffffffll / n))
    return set_error("%s: sizes out of range (%lld x %lld)", fn, (long long)n, (long long)k);
  if (n == 0 || k == 0) return 0;
  if (!a_dev || !b_dev || !out_dev) return set_error("%s: null pointer", fn);
  hipLaunchKernelGGL(det_overlap_kernel, dim3((unsigned)det_blocks(n * k, kDetThreads)), dim3(kDetThreads), 0, (hipStream_t)stream, a_dev, n,
                     b_dev, k, out_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

int64_t dif_det_workspace_size(int64_t m, int64_t t, int j) {
  if (det_check_sizes("dif_det_workspace_size", m, t, j)) return -1;
  DetWork w;
  return (int64_t)det_carve(nullptr, m, t, j, &w);
}

int dif_det_match(const int64_t* det_offsets_dev, const float* det_boxes_dev, const float* det_scores_dev, int64_t m,
                  const int64_t* gt_offsets_dev, const float* gt_boxes_dev, const uint8_t* gt_ignore_dev, int64_t t, int64_t n_frames,
                  const double* thr_host, int j, int32_t* assigned_out_dev, double* iou_out_dev, uint8_t* outcome_out_dev,
                  int64_t* n_truth_out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  const char* fn = "dif_det_match";
  if (det_check_sizes(fn, m, t, j)) return -1;
  if (n_frames < 0 || n_frames > DIF_DET_MAX_ROWS) return set_error("%s: %lld frames out of range", fn, (long long)n_frames);
  if ((m > 0 || t > 0) && n_frames == 0) return set_error("%s: %lld detections and %lld truths in no frame", fn, (long long)m, (long long)t);
  if (!thr_host) return set_error("%s: null pointer", fn);
  DetThr thr = {};
  for (int i = 0; i < j; ++i) {
    if (!(thr_host[i] > 0.0 && thr_host[i] <= 1.0)) return set_error("%s: IoU threshold %d (%g) outside (0, 1]", fn, i, thr_host[i]);
    thr.v[i] = thr_host[i];
  }
  if (!n_truth_out_dev || (n_frames > 0 && (!det_offsets_dev || !gt_offsets_dev))) return set_error("%s: null pointer", fn);
  if (m > 0 && (!det_boxes_dev || !det_scores_dev || !assigned_out_dev || !iou_out_dev || !outcome_out_dev)) return set_error("%s: null pointer", fn);
  if (t > 0 && !gt_boxes_dev) return set_error("%s: null pointer", fn);
  const int64_t need = dif_det_workspace_size(m, t, j);
  if (need > 0 && (!workspace_dev || workspace_bytes < need))
    return set_error("%s: workspace of %lld bytes, %lld needed (dif_det_workspace_size)", fn, (long long)workspace_bytes, (long long)need);
  if ((uintptr_t)workspace_dev & 7) return set_error("%s: the workspace must be aligned to 8 bytes", fn);
  hipStream_t st = (hipStream_t)stream;
  DetWork w;
  det_carve(workspace_dev, m, t, j, &w);
  DIF_HIP(hipMemsetAsync(n_truth_out_dev, 0, 8, st));
  if (t > 0)
    hipLaunchKernelGGL(det_truth_kernel, dim3((unsigned)det_blocks(t, kDetThreads)), dim3(kDetThreads), 0, st, gt_ignore_dev, t, j, w.claim,
                       (unsigned long long*)n_truth_out_dev);
  if (m > 0) {
    const dim3 grid((unsigned)det_blocks(m, kDetThreads));
    hipLaunchKernelGGL(det_best_kernel, grid, dim3(kDetThreads), 0, st, det_offsets_dev, gt_offsets_dev, n_frames, det_boxes_dev, m, gt_boxes_dev,
                       t, assigned_out_dev, iou_out_dev);
    if (det_sort(det_scores_dev, m, w, st)) return -1;
    hipLaunchKernelGGL(det_rank_kernel, grid, dim3(kDetThreads), 0, st, w.p0, (int)m, w.rank, (int64_t*)nullptr);
    hipLaunchKernelGGL(det_claim_kernel, grid, dim3(kDetThreads), 0, st, assigned_out_dev, iou_out_dev, w.rank, gt_ignore_dev, (int)m, t, thr, j,
                       w.claim);
    hipLaunchKernelGGL(det_classify_kernel, grid, dim3(kDetThreads), 0, st, assigned_out_dev, iou_out_dev, w.rank, gt_ignore_dev, (int)m, t, thr,
                       j, w.claim, outcome_out_dev);
  }
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_det_curve(const float* scores_dev, const uint8_t* outcome_dev, const int64_t* n_truth_dev, int64_t m, int j, int64_t* order_out_dev,
                  int64_t* tp_cum_out_dev, int64_t* fp_cum_out_dev, double* recall_out_dev, double* precision_out_dev, double* ap_out_dev,
                  void* workspace_dev, int64_t workspace_bytes, void* stream) {
  const char* fn = "dif_det_curve";
  if (det_check_sizes(fn, m, 0, j)) return -1;
  if (!n_truth_dev || !ap_out_dev) return set_error("%s: null pointer", fn);
  if (m > 0 && (!scores_dev || !outcome_dev || !order_out_dev || !tp_cum_out_dev || !fp_cum_out_dev || !recall_out_dev || !precision_out_dev))
    return set_error("%s: null pointer", fn);
  const int64_t need = dif_det_workspace_size(m, 0, j);
  if (need > 0 && (!workspace_dev || workspace_bytes < need))
    return set_error("%s: workspace of %lld bytes, %lld needed (dif_det_workspace_size)", fn, (long long)workspace_bytes, (long long)need);
  if ((uintptr_t)workspace_dev & 7) return set_error("%s: the workspace must be aligned to 8 bytes", fn);
  hipStream_t st = (hipStream_t)stream;
  DetWork w;
  det_carve(workspace_dev, m, 0, j, &w);
  const int nt = (int)det_blocks(m, kDetScanTile);
  if (m > 0) {
    if (det_sort(scores_dev, m, w, st)) return -1;
    hipLaunchKernelGGL(det_rank_kernel, dim3((unsigned)det_blocks(m, kDetThreads)), dim3(kDetThreads), 0, st, w.p0, (int)m, (int*)nullptr,
                       order_out_dev);
    const dim3 tiles(nt, j);
    hipLaunchKernelGGL(det_count_kernel, tiles, dim3(kDetThreads), 0, st, outcome_dev, w.p0, (int)m, nt, w.part);
    hipLaunchKernelGGL(det_count_scan_kernel, dim3(j), dim3(64), 0, st, w.part, nt);
    hipLaunchKernelGGL(det_apply_kernel, tiles, dim3(kDetThreads), 0, st, outcome_dev, w.p0, (int)m, nt, w.part, n_truth_dev, tp_cum_out_dev,
                       fp_cum_out_dev, recall_out_dev, precision_out_dev);
    hipLaunchKernelGGL(det_tile_max_kernel, tiles, dim3(kDetThreads), 0, st, precision_out_dev, m, nt, w.tmax);
    hipLaunchKernelGGL(det_carry_kernel, dim3(j), dim3(64), 0, st, w.tmax, nt);
    hipLaunchKernelGGL(det_tile_ap_kernel, tiles, dim3(kDetThreads), 0, st, recall_out_dev, precision_out_dev, m, nt, w.tmax, w.tsum);
  }
  hipLaunchKernelGGL(det_ap_sum_kernel, dim3(j), dim3(64), 0, st, recall_out_dev, m, nt, w.tsum, ap_out_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_det_ap(const double* recall_dev, const double* precision_dev, int64_t m, double* out_dev, void* stream) {
  const char* fn = "dif_det_ap";
  if (m < 0 || m > DIF_DET_MAX_ROWS) return set_error("%s: %lld points out of range", fn, (long long)m);
  if (!out_dev || (m > 0 && (!recall_dev || !precision_dev))) return set_error("%s: null pointer", fn);
  hipLaunchKernelGGL(det_ap_kernel, dim3(1), dim3(kDetThreads), 0, (hipStream_t)stream, recall_dev, precision_dev, m, out_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
