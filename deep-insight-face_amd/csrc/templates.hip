// hipcc-flags: -ffp-contract=off
// (the reduction and the finish restate NumPy's float32 arithmetic operation by operation: a product is rounded before
// it is added, and match_ref.hpp asks for this flag of every translation unit that includes it)
// Template pooling: one exact mean embedding per identity (include/dif.h, "template pooling").
//   group   pool_stats_kernel      OR of the non-negative labels and of their complements: a bit that is set in both
//                                  varies, a byte without such a bit is constant and its sort pass is skipped
//           pool_init_kernel       (key, position) pairs -- the t0 state labels in front of the n new ones, every negative
//                                  label mapped to ONE key above all others -- and the plan of the eight passes
//           radix_sort_run         the stable LSD radix sort of csrc/radix_sort.hip under that plan.  All eight passes are
//                                  enqueued; a skipped one returns at once, and which of the two buffers a pass reads is
//                                  part of the plan in device memory
//           pool_heads_kernel      segment heads per block of kHeadBlock sorted keys (block_scan_run scans them)
//           pool_index_kernel      template number of every key -> index_out, the start of every segment, T
//   reduce  pool_reduce_kernel     one thread per (segment, float4 column): the segment's rows in sorted -- that is, row --
//                                  order into ONE accumulator, the loads of kLookAhead rows issued in front of their
//                                  adds and their positions a chunk earlier
//   best    pool_best_kernel       one thread per segment: the row with the greatest key, in the segment's order (best shot)
//   finish  pool_finish_kernel     one wave per template: sums / divisor, and the row's norm in NumPy's order (np_sum)
// The only atomics are the ORs of pool_stats_kernel and the sort's LDS counters, whose totals do not depend on the order; every
// output is a function of the input alone.
#include "../../include/dif.h"
#include "match_ref.hpp"
#include <new>

namespace dif {

// The tile of the sort's passes, restated from csrc/radix_sort.hip where the tests of this file's sizes read it
// (tests/test_templates_gpu.py); the assertion keeps the two from drifting apart.
constexpr int kSortThreads = 256;
constexpr int kSortItems = 8;
static_assert(kSortThreads * kSortItems == kRadixSortTile, "the sort's tile: csrc/radix_sort.hip");
constexpr int kHeadBlock = 256;                             // sorted keys per block of pool_heads_kernel / pool_index_kernel
constexpr int kLookAhead = 16;                              // rows of a segment in flight in pool_reduce_kernel
constexpr unsigned long long kNegBit = 1ull << 63;

struct PoolMeta {
  unsigned long long or_all, nor_all;   // OR of the non-negative labels, OR of their complements
  int any_neg, any_nonneg;
  RadixPlan sort;                       // the eight passes: pool_init_kernel writes it, radix_sort_run follows it
  long long T;                          // templates after the group
};

__device__ __forceinline__ int64_t pool_label(const int64_t* __restrict__ state, int t0, const int64_t* __restrict__ labels, int i) {
  return i < t0 ? state[i] : labels[i - t0];
}

__global__ __launch_bounds__(256) void pool_stats_kernel(const int64_t* __restrict__ state, int t0, const int64_t* __restrict__ labels, int m,
                                                         PoolMeta* __restrict__ meta) {
  unsigned long long o = 0, no = 0;
  int neg = 0, nonneg = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    const int64_t l = pool_label(state, t0, labels, (int)i);
    if (l < 0) {
      neg = 1;
    } else {
      o |= (unsigned long long)l;
      no |= ~(unsigned long long)l;
      nonneg = 1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    o |= __shfl_xor(o, off);
    no |= __shfl_xor(no, off);
    neg |= __shfl_xor(neg, off);
    nonneg |= __shfl_xor(nonneg, off);
  }
  if ((threadIdx.x & 63) == 0) {
    if (o) atomicOr(&meta->or_all, o);
    if (no) atomicOr(&meta->nor_all, no);
    if (neg) atomicOr(&meta->any_neg, 1);
    if (nonneg) atomicOr(&meta->any_nonneg, 1);
  }
}

__global__ __launch_bounds__(256) void pool_init_kernel(const int64_t* __restrict__ state, int t0, const int64_t* __restrict__ labels, int m,
                                                        PoolMeta* __restrict__ meta, unsigned long long* __restrict__ keys,
                                                        int* __restrict__ pos) {
  const unsigned long long or_all = meta->or_all, nor_all = meta->nor_all;
  // every negative label becomes one key: above every label by its top bit, equal to the labels in each byte that is
  // constant over them, so that it adds no pass but the last
  const unsigned long long negkey = kNegBit | ~nor_all;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    const int64_t l = pool_label(state, t0, labels, (int)i);
    keys[i] = l < 0 ? negkey : (unsigned long long)l;
    pos[i] = (int)i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    unsigned long long varies = or_all & nor_all;
    if (meta->any_neg && meta->any_nonneg) varies |= 0xffull << 56;
    int buf = 0;
    for (int b = 0; b < 8; ++b) {
      const int on = ((varies >> (8 * b)) & 0xff) != 0;
      meta->sort.active[b] = on;
      meta->sort.src[b] = buf;
      buf ^= on;
    }
    meta->sort.final_buf = buf;
  }
}

// sorted key i opens a segment: a label (not the key of the negatives) that differs from the key in front of it
__device__ __forceinline__ bool pool_is_head(const unsigned long long* __restrict__ keys, int64_t i, int m) {
  if (i >= m) return false;
  const unsigned long long k = keys[i];
  return !(k & kNegBit) && (i == 0 || keys[i - 1] != k);
}

__global__ __launch_bounds__(kHeadBlock) void pool_heads_kernel(const PoolMeta* __restrict__ meta, const unsigned long long* __restrict__ k0,
                                                                const unsigned long long* __restrict__ k1, int m,
                                                                unsigned* __restrict__ block_heads) {
  const unsigned long long* __restrict__ keys = meta->sort.final_buf ? k1 : k0;
  __shared__ int wave_total[kHeadBlock / 64];
  const int tid = threadIdx.x;
  const unsigned long long mask = __ballot(pool_is_head(keys, (int64_t)blockIdx.x * kHeadBlock + tid, m));
  if ((tid & 63) == 0) wave_total[tid >> 6] = __popcll(mask);
  __syncthreads();
  if (tid == 0) {
    int all = 0;
#pragma unroll
    for (int w = 0; w < kHeadBlock / 64; ++w) all += wave_total[w];
    block_heads[blockIdx.x] = (unsigned)all;
  }
}

// i runs over [0, m]: the sorted keys and one slot behind them.  The labels end at the first key of the negatives, or at
// m: that slot closes the last segment and knows T.
__global__ __launch_bounds__(kHeadBlock) void pool_index_kernel(PoolMeta* __restrict__ meta, const unsigned long long* __restrict__ k0,
                                                                const unsigned long long* __restrict__ k1, const int* __restrict__ p0,
                                                                const int* __restrict__ p1, int m, int t0,
                                                                const unsigned* __restrict__ block_heads, int* __restrict__ seg_start,
                                                                int64_t* __restrict__ index_out, int64_t* __restrict__ t_out) {
  const int fin = meta->sort.final_buf;
  const unsigned long long* __restrict__ keys = fin ? k1 : k0;
  const int* __restrict__ pos = fin ? p1 : p0;
  __shared__ int wave_total[kHeadBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * kHeadBlock + tid;
  const bool head = pool_is_head(keys, i, m);
  const unsigned long long mask = __ballot(head);
  if (lane == 0) wave_total[wave] = __popcll(mask);
  __syncthreads();
  int before = (int)block_heads[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));   // heads in front of i
  for (int w = 0; w < wave; ++w) before += wave_total[w];
  if (i > m) return;
  const bool neg = i < m && (keys[i] & kNegBit);
  if (head) seg_start[before] = (int)i;
  if ((i == m || neg) && (i == 0 || !(keys[i - 1] & kNegBit))) {
    seg_start[before] = (int)i;
    meta->T = before;
    t_out[0] = before;
  }
  if (i < m) {
    const int p = pos[i];
    if (p >= t0) index_out[p - t0] = neg ? -1 : (int64_t)(before + (head ? 1 : 0) - 1);
  }
}

template <bool W>
__global__ __launch_bounds__(256) void pool_reduce_kernel(const PoolMeta* __restrict__ meta, const unsigned long long* __restrict__ k0,
                                                          const unsigned long long* __restrict__ k1, const int* __restrict__ p0,
                                                          const int* __restrict__ p1, const int* __restrict__ seg_start, int t0,
                                                          const float4* __restrict__ state_sums, const float* __restrict__ state_wsum,
                                                          const int64_t* __restrict__ state_counts, const float4* __restrict__ rows,
                                                          const float* __restrict__ weights, int64_t t, int q,
                                                          int64_t* __restrict__ labels_out, float4* __restrict__ sums_out,
                                                          float* __restrict__ wsum_out, int64_t* __restrict__ counts_out) {
#pragma clang fp contract(off)
  if (meta->T != t) return;                     // the caller's buffers hold t templates: write nothing into a wrong size
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t seg = gid / q;
  const int c = (int)(gid - seg * q);
  if (seg >= t) return;
  const int fin = meta->sort.final_buf;
  const int* __restrict__ order = fin ? p1 : p0;
  const int b = seg_start[seg], e = seg_start[seg + 1];
  const int first = order[b];
  float4 acc;
  float ws = 0.f;
  int64_t cnt;
  if (first < t0) {                             // a stored template: its sum goes on
    acc = state_sums[(int64_t)first * q + c];
    if (W) ws = state_wsum[first];
    cnt = state_counts[first] + (e - b - 1);
  } else {                                      // the sum starts AT the first row, not at zero: -0 stays -0
    const float4 x = rows[(int64_t)(first - t0) * q + c];
    if (W) {
      const float w = weights[first - t0];
      acc = make_float4(w * x.x, w * x.y, w * x.z, w * x.w);
      ws = w;
    } else {
      acc = x;
    }
    cnt = e - b;
  }
  // The rest of the segment in chunks of kLookAhead rows: the loads of a chunk are issued together, in front of its adds,
  // and its positions were loaded a chunk earlier, so that a row's load never waits on the load of its position.
  int next[kLookAhead];
  int64_t i = b + 1;
#pragma unroll
  for (int k = 0; k < kLookAhead; ++k) next[k] = k < e - i ? order[i + k] : -1;
  for (; i < e; i += kLookAhead) {
    float4 x[kLookAhead];
    float w[kLookAhead];
#pragma unroll
    for (int k = 0; k < kLookAhead; ++k) {
      const int p = next[k];
      next[k] = k + kLookAhead < e - i ? order[i + kLookAhead + k] : -1;
      x[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      w[k] = 0.f;
      if (p >= 0) {
        x[k] = rows[(int64_t)(p - t0) * q + c];
        if (W) w[k] = weights[p - t0];
      }
    }
#pragma unroll
    for (int k = 0; k < kLookAhead; ++k)
      if (k < e - i) {                          // in row order, one add after the other
        if (W) {
          acc.x = acc.x + w[k] * x[k].x;
          acc.y = acc.y + w[k] * x[k].y;
          acc.z = acc.z + w[k] * x[k].z;
          acc.w = acc.w + w[k] * x[k].w;
          ws = ws + w[k];
        } else {
          acc.x = acc.x + x[k].x;
          acc.y = acc.y + x[k].y;
          acc.z = acc.z + x[k].z;
          acc.w = acc.w + x[k].w;
        }
      }
  }
  sums_out[seg * q + c] = acc;
  if (c == 0) {
    labels_out[seg] = (int64_t)(fin ? k1 : k0)[b];
    counts_out[seg] = cnt;
    if (W) wsum_out[seg] = ws;
  }
}

// One thread per segment: the stored entry, if the segment has one, then the new rows in ascending row; a row is taken
// when nothing was taken yet or its key is strictly greater, so a tie keeps the lower row and a NaN never wins.
__global__ __launch_bounds__(256) void pool_best_kernel(const PoolMeta* __restrict__ meta, const unsigned long long* __restrict__ k0,
                                                        const unsigned long long* __restrict__ k1, const int* __restrict__ p0,
                                                        const int* __restrict__ p1, const int* __restrict__ seg_start, int t0,
                                                        const float* __restrict__ state_key, const int64_t* __restrict__ state_row,
                                                        const int64_t* __restrict__ state_counts, const float* __restrict__ key, int64_t row_base,
                                                        int64_t t, int64_t* __restrict__ labels_out, float* __restrict__ key_out,
                                                        int64_t* __restrict__ row_out, int64_t* __restrict__ counts_out) {
  if (meta->T != t) return;                     // as pool_reduce_kernel: nothing into buffers of a wrong size
  const int64_t seg = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (seg >= t) return;
  const int fin = meta->sort.final_buf;
  const int* __restrict__ order = fin ? p1 : p0;
  const int b = seg_start[seg], e = seg_start[seg + 1];
  float best = __builtin_nanf("");
  int64_t row = -1, cnt = e - b;
  int i = b;
  const int first = order[b];
  if (first < t0) {
    best = state_key[first];
    row = state_row[first];
    if (row < 0 || best != best) {              // a label that has shown NaN keys only
      best = __builtin_nanf("");
      row = -1;
    }
    cnt = state_counts[first] + (e - b - 1);
    i = b + 1;
  }
  for (; i < e; ++i) {
    const int p = order[i] - t0;
    const float k = key[p];
    if (k == k && (row < 0 || k > best)) {
      best = k;
      row = row_base + p;
    }
  }
  labels_out[seg] = (int64_t)(fin ? k1 : k0)[b];
  key_out[seg] = best;
  row_out[seg] = row;
  counts_out[seg] = cnt;
}

__global__ __launch_bounds__(256) void pool_finish_kernel(const float* __restrict__ sums, const float* __restrict__ wsum,
                                                          const int64_t* __restrict__ counts, int64_t t, int d, int normalize,
                                                          const SumPlan plan, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float scratch[4][NP_PLANE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= t) return;                         // (np_sum synchronises the wave alone)
  const float div = wsum ? wsum[row] : (float)counts[row];
  const float* __restrict__ s = sums + row * d;
  float* __restrict__ o = out + row * d;
  float norm = 1.f;
  if (normalize) {
    const float ss = np_sum(plan, scratch[wave], lane, [&](int k) {
      const float mean = s[k] / div;
      return mean * mean;
    });
    norm = __builtin_sqrtf(ss);
  }
  for (int k = lane; k < d; k += 64) {
    const float mean = s[k] / div;
    o[k] = normalize ? mean / norm : mean;
  }
}

}  // namespace dif

using namespace dif;

struct dif_pool {
  int d = 0;
  char* ws = nullptr;            // one allocation, carved by pool_carve for the sizes of the last group
  size_t ws_cap = 0;
  PoolMeta* meta = nullptr;
  unsigned long long* keys[2] = {nullptr, nullptr};
  int* pos[2] = {nullptr, nullptr};
  unsigned* hist = nullptr;      // the sort's histogram
  unsigned* block_heads = nullptr;
  int* seg_start = nullptr;      // [T + 1]
  bool grouped = false;          // the workspace holds the order of a group ...
  int64_t t0 = 0, n = 0;         // ... of these sizes
  int64_t* t_host = nullptr;     // pinned: T of the last group, copied asynchronously behind it; valid once t_event has passed
  hipEvent_t t_event = nullptr;
};

static size_t pool_carve(dif_pool* p, int64_t m, int64_t nhb) {
  Carver c(p->ws);
  p->meta = (PoolMeta*)c.take(sizeof(PoolMeta));
  for (int i = 0; i < 2; ++i) p->keys[i] = (unsigned long long*)c.take((size_t)m * 8);
  for (int i = 0; i < 2; ++i) p->pos[i] = (int*)c.take((size_t)m * 4);
  p->hist = (unsigned*)c.take(radix_sort_hist_bytes(m > 0 ? m : 1));
  p->block_heads = (unsigned*)c.take((size_t)nhb * 4);
  p->seg_start = (int*)c.take((size_t)(m + 1) * 4);
  return c.at;
}

static bool misaligned16(const void* q) { return ((uintptr_t)q & 15) != 0; }

extern "C" {

int dif_pool_create(dif_pool** out, int d) {
  if (!out) return set_error("dif_pool_create: null out");
  if (d <= 0 || d % 32 != 0) return set_error("dif_pool_create: embedding size must be a positive multiple of 32 (got %d)", d);
  dif_pool* p = new (std::nothrow) dif_pool();
  if (!p) return set_error("dif_pool_create: out of host memory");
  p->d = d;
  hipError_t e = hipHostMalloc((void**)&p->t_host, sizeof(int64_t), hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p->t_event, hipEventDisableTiming);
  if (e != hipSuccess) {
    if (p->t_host) (void)hipHostFree(p->t_host);
    delete p;
    return set_error("dif_pool_create: %s", hipGetErrorString(e));
  }
  *out = p;
  return 0;
}

int dif_pool_destroy(dif_pool* p) {
  if (!p) return 0;
  if (p->ws) (void)hipFree(p->ws);
  if (p->t_event) (void)hipEventDestroy(p->t_event);
  if (p->t_host) (void)hipHostFree(p->t_host);
  delete p;
  return 0;
}

int dif_pool_group(dif_pool* p, const int64_t* state_labels_dev, int64_t t0, const int64_t* labels_dev, int64_t n, int64_t* index_out_dev,
                   int64_t* t_out_dev, void* stream) {
  if (!p) return set_error("dif_pool_group: null handle");
  if (t0 < 0 || n < 0 || t0 > 0x7fffffff || n > 0x7fffffff || t0 + n > 0x7fffffffll)
    return set_error("dif_pool_group: sizes out of range (t0 %lld, n %lld; t0 + n must stay below 2^31)", (long long)t0, (long long)n);
  if (!t_out_dev || (t0 > 0 && !state_labels_dev) || (n > 0 && (!labels_dev || !index_out_dev)))
    return set_error("dif_pool_group: null pointer");
  hipStream_t st = (hipStream_t)stream;
  p->grouped = false;
  const int64_t m = t0 + n;
  const int64_t nb = m > 0 ? (m + radix_sort_tile() - 1) / radix_sort_tile() : 1;   // blocks of a sort pass
  const int64_t nhb = (m + 1 + kHeadBlock - 1) / kHeadBlock;
  if (nb * 256 > 0x7fffffff) return set_error("dif_pool_group: sizes out of range");
  dif_pool probe;
  const size_t need = pool_carve(&probe, m, nhb);
  if (grow(&p->ws, &p->ws_cap, need, 1)) return -1;
  pool_carve(p, m, nhb);
  DIF_HIP(hipMemsetAsync(p->meta, 0, sizeof(PoolMeta), st));
  const unsigned flat = (unsigned)(m > 0 ? (nb < 2048 ? nb : 2048) : 1);
  hipLaunchKernelGGL(pool_stats_kernel, dim3(flat), dim3(256), 0, st, state_labels_dev, (int)t0, labels_dev, (int)m, p->meta);
  hipLaunchKernelGGL(pool_init_kernel, dim3(flat), dim3(256), 0, st, state_labels_dev, (int)t0, labels_dev, (int)m, p->meta, p->keys[0],
                     p->pos[0]);
  if (m > 1 && radix_sort_run(&p->meta->sort, 8, p->keys[0], p->keys[1], p->pos[0], p->pos[1], m, p->hist, st)) return -1;
  hipLaunchKernelGGL(pool_heads_kernel, dim3((unsigned)nhb), dim3(kHeadBlock), 0, st, p->meta, p->keys[0], p->keys[1], (int)m, p->block_heads);
  if (block_scan_run(p->block_heads, nhb, st)) return -1;
  hipLaunchKernelGGL(pool_index_kernel, dim3((unsigned)nhb), dim3(kHeadBlock), 0, st, p->meta, p->keys[0], p->keys[1], p->pos[0], p->pos[1],
                     (int)m, (int)t0, p->block_heads, p->seg_start, index_out_dev, t_out_dev);
  DIF_HIP(hipGetLastError());
  // T follows the kernels into pinned memory without a wait: dif_pool_reduce compares it once the event has passed
  DIF_HIP(hipMemcpyAsync(p->t_host, &p->meta->T, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  DIF_HIP(hipEventRecord(p->t_event, st));
  p->grouped = true;
  p->t0 = t0;
  p->n = n;
  return 0;
}

int dif_pool_reduce(dif_pool* p, const float* state_sums_dev, const float* state_wsum_dev, const int64_t* state_counts_dev,
                    const float* rows_dev, const float* weights_dev, int64_t t, int64_t* labels_out_dev, float* sums_out_dev,
                    float* wsum_out_dev, int64_t* counts_out_dev, void* stream) {
  if (!p) return set_error("dif_pool_reduce: null handle");
  if (!p->grouped) return set_error("dif_pool_reduce: no dif_pool_group on this handle left an order behind");
  if (t < p->t0 || t > p->t0 + p->n)
    return set_error("dif_pool_reduce: t %lld disagrees with the group (%lld stored templates, %lld rows)", (long long)t, (long long)p->t0,
                     (long long)p->n);
  const hipError_t seen = hipEventQuery(p->t_event);
  (void)hipGetLastError();                      // (not ready is no error)
  if (seen == hipSuccess && *p->t_host != t)
    return set_error("dif_pool_reduce: t %lld disagrees with the %lld templates the group found", (long long)t, (long long)*p->t_host);
  const bool weighted = weights_dev != nullptr;
  if ((p->t0 > 0 && (!state_sums_dev || !state_counts_dev || (weighted && !state_wsum_dev))) || (p->n > 0 && !rows_dev) ||
      (t > 0 && (!labels_out_dev || !sums_out_dev || !counts_out_dev || (weighted && !wsum_out_dev))))
    return set_error("dif_pool_reduce: null pointer");
  if (misaligned16(state_sums_dev) || misaligned16(rows_dev) || misaligned16(sums_out_dev))
    return set_error("dif_pool_reduce: rows and sums must be aligned to 16 bytes");
  if (t == 0) return 0;
  const int q = p->d / 4;
  const int64_t blocks = (t * q + 255) / 256;
  if (blocks > 0x7fffffff) return set_error("dif_pool_reduce: sizes out of range");
  hipStream_t st = (hipStream_t)stream;
  auto kernel = weighted ? pool_reduce_kernel<true> : pool_reduce_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, p->meta, p->keys[0], p->keys[1], p->pos[0], p->pos[1], p->seg_start,
                     (int)p->t0, (const float4*)state_sums_dev, state_wsum_dev, state_counts_dev, (const float4*)rows_dev, weights_dev, t, q,
                     labels_out_dev, (float4*)sums_out_dev, wsum_out_dev, counts_out_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_pool_best(dif_pool* p, const float* state_key_dev, const int64_t* state_row_dev, const int64_t* state_counts_dev, const float* key_dev,
                  int64_t row_base, int64_t t, int64_t* labels_out_dev, float* key_out_dev, int64_t* row_out_dev, int64_t* counts_out_dev,
                  void* stream) {
  if (!p) return set_error("dif_pool_best: null handle");
  if (!p->grouped) return set_error("dif_pool_best: no dif_pool_group on this handle left an order behind");
  if (t < p->t0 || t > p->t0 + p->n)
    return set_error("dif_pool_best: t %lld disagrees with the group (%lld stored templates, %lld rows)", (long long)t, (long long)p->t0,
                     (long long)p->n);
  const hipError_t seen = hipEventQuery(p->t_event);
  (void)hipGetLastError();                      // (not ready is no error)
  if (seen == hipSuccess && *p->t_host != t)
    return set_error("dif_pool_best: t %lld disagrees with the %lld templates the group found", (long long)t, (long long)*p->t_host);
  if ((p->t0 > 0 && (!state_key_dev || !state_row_dev || !state_counts_dev)) || (p->n > 0 && !key_dev) ||
      (t > 0 && (!labels_out_dev || !key_out_dev || !row_out_dev || !counts_out_dev)))
    return set_error("dif_pool_best: null pointer");
  if (t == 0) return 0;
  hipLaunchKernelGGL(pool_best_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->meta, p->keys[0], p->keys[1],
                     p->pos[0], p->pos[1], p->seg_start, (int)p->t0, state_key_dev, state_row_dev, state_counts_dev, key_dev, row_base, t,
                     labels_out_dev, key_out_dev, row_out_dev, counts_out_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

int dif_pool_finish(const float* sums_dev, const float* wsum_dev, const int64_t* counts_dev, int64_t t, int d, int normalize, float* out_dev,
                    void* stream) {
  if (d <= 0 || d % 32 != 0) return set_error("dif_pool_finish: embedding size must be a positive multiple of 32 (got %d)", d);
  if (t < 0 || t > 0x7fffffff) return set_error("dif_pool_finish: t %lld out of range", (long long)t);
  if (t == 0) return 0;
  if (!sums_dev || !out_dev || (!wsum_dev && !counts_dev)) return set_error("dif_pool_finish: null pointer");
  SumPlan plan;
  if (make_sum_plan(d, &plan)) return -1;
  hipLaunchKernelGGL(pool_finish_kernel, dim3((unsigned)((t + 3) / 4)), dim3(256), 0, (hipStream_t)stream, sums_dev, wsum_dev, counts_dev, t, d,
                     normalize != 0, plan, out_dev);
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
