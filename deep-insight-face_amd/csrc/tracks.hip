// hipcc-flags: -ffp-contract=off
// (box_iou of box_iou.hpp and ref_distance restate float32 arithmetic operation by operation: a product is rounded before it is
// added, and match_ref.hpp asks for this flag of every translation unit that includes it)
// Tracks: the faces of a sequence of frames linked into tracks (include/dif.h, "tracks").
//   tracks_cand_kernel    one block per (face j, gap g): the faces of frame f - g are the tails j may continue.  Lane p
//                         takes the tail at position p and gates it by the IoU; the ballot of the gate is split among the
//                         block's four waves, and a wave evaluates ref_distance for one gated pair at a time (the idiom
//                         of pairwise_kernel, the same SumPlan).  cand[j][(G - g) * K + p] = the distance where it is
//                         <= tolerance, else NaN: ascending slot = ascending tail row.  A pair the gate rejects costs no
//                         distance.
//   tracks_walk_kernel    ONE block, frame by frame, over an LDS ring of the last G frames' faces: every face keeps its
//                         nearest open tail (a wave per face over its G * K slots), the block picks the least (dist, tail,
//                         face) among them, closes the tail, and only the faces whose nearest tail that was look again.
//                         Loops are bounded by N, kmax and G * K, the control flow around every barrier is uniform over
//                         the block, nothing waits on another block, and every output element is written by one thread:
//                         no atomics.
//   tracks_state_kernel   the last G frames -- old state, padding or new faces -- into the fixed slots of the next state.
// Frames are numbered over the state and the call together: state slot s holds frame s (0 .. G - 1), `pad` empty frames
// follow (batches without a face that the caller skipped), and frame n of the call is frame G + pad + n.
#include "../../include/dif.h"
#include "box_iou.hpp"
#include "frame_rows.hpp"
#include "gemm_core.hpp"
#include "match_ref.hpp"

namespace dif {

constexpr int kTrackKmax = DIF_TRACKS_MAX_FACES;   // positions of a frame that take part: one lane each
constexpr int kTrackGap = DIF_TRACKS_MAX_GAP;
constexpr int kTrackSlots = kTrackKmax * kTrackGap;   // tails a face can see
constexpr int kWalkThreads = 256;
constexpr int kWalkWaves = kWalkThreads / 64;

// A state of G frames with K slots each and embeddings of d floats, as one buffer (S = G * K):
//   int64 labels[S], age[S], rows[S]; float boxes[S][4], emb[S][d]; int32 closed[S], count[G]; rounded up to 8 bytes
struct TrackState {
  int64_t* labels;
  int64_t* age;
  int64_t* rows;
  float* boxes;
  float* emb;
  int* closed;
  int* count;
  int* tail;                // the word that rounds the buffer up to 8 bytes, or nullptr
};

__host__ __device__ inline size_t track_state_carve(void* base, int G, int K, int d, TrackState* s) {
  char* q = (char*)base;
  const size_t S = (size_t)G * K;
  size_t at = 0;
  s->labels = (int64_t*)(q + at), at += S * 8;
  s->age = (int64_t*)(q + at), at += S * 8;
  s->rows = (int64_t*)(q + at), at += S * 8;
  s->boxes = (float*)(q + at), at += S * 16;
  s->emb = (float*)(q + at), at += S * (size_t)d * 4;
  s->closed = (int*)(q + at), at += S * 4;
  s->count = (int*)(q + at), at += (size_t)G * 4;
  s->tail = (at & 7) ? (int*)(q + at) : nullptr;
  return (at + 7) & ~(size_t)7;
}

struct TrackSeq {
  const int64_t* offsets;   // [N + 1] of the call
  int64_t n_frames, m;
  int G, kmax;              // max_gap; positions of a frame of the call that take part
  const void* state;        // the state handed in, or nullptr
  int Ks, d;                // ... its slots per frame; floats per embedding
  int pad;                  // empty frames between the state and the call, at most G
  int K;                    // slots per gap of the candidate table: max(kmax, Ks)
};

// the arrays of the state handed in (carved where they are used: seven pointers held across the walk's loops cost SGPRs)
__device__ __forceinline__ TrackState track_state_in(const TrackSeq& q) {
  TrackState s;
  track_state_carve(const_cast<void*>(q.state), q.G, q.Ks, q.d, &s);
  return s;
}

// The face at position p of frame cf as an index over [the state's G * Ks slots][the call's m rows], or -1: no such
// frame, no such face, or a clipped one.
__device__ __forceinline__ int64_t track_tail(const TrackSeq& q, int64_t cf, int p) {
  if (cf < 0) return -1;
  if (cf < q.G) return (q.state && p < q.Ks && p < track_state_in(q).count[cf]) ? cf * q.Ks + p : -1;
  const int64_t n = cf - q.G - q.pad;
  if (n < 0 || n >= q.n_frames || p >= q.kmax) return -1;
  int64_t b, e;
  frame_rows(q.offsets, n, q.m, &b, &e);
  return p < e - b ? (int64_t)q.G * q.Ks + b + p : -1;
}

__global__ __launch_bounds__(256) void tracks_cand_kernel(const TrackSeq q, const float* __restrict__ boxes, const float* __restrict__ emb,
                                                          int d, float tolerance, float min_iou, int metric, const SumPlan plan,
                                                          float* __restrict__ cand) {
#pragma clang fp contract(off)
  __shared__ float scratch[4][NP_SCRATCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = blockIdx.x / q.G;
  const int g = (int)(blockIdx.x - j * q.G) + 1;
  const int64_t lo = frame_bisect(q.offsets, q.n_frames, j);   // the frame of row j (offsets[0] = 0, offsets[N] = m)
  int64_t b, e;
  frame_rows(q.offsets, lo, q.m, &b, &e);
  if (j < b || j >= e || j - b >= q.kmax) return;           // (uniform over the block) a clipped face: its slots are never read
  const int64_t cf = q.G + q.pad + lo;
  const int64_t c = lane < q.K ? track_tail(q, cf - g, lane) : -1;
  const int64_t Sn = (int64_t)q.G * q.Ks;
  bool pass = false;
  if (c >= 0) {
    const float* tb = c < Sn ? track_state_in(q).boxes + c * 4 : boxes + (c - Sn) * 4;
    pass = box_iou(tb, boxes + j * 4) >= min_iou;           // (a NaN IoU compares false)
  }
  const unsigned long long mask = __ballot(pass);
  float* __restrict__ row = cand + (j * q.G + (q.G - g)) * q.K;
  if (wave == 0 && lane < q.K && !pass) row[lane] = __builtin_nanf("");
  unsigned long long rest = mask;
  for (int k = 0; rest; ++k) {
    const int p = __builtin_ctzll(rest);
    rest &= rest - 1;
    if ((k & 3) != wave) continue;              // (uniform over the wave)
    const int64_t ci = __shfl(c, p);
    const float* ei = ci < Sn ? track_state_in(q).emb + ci * d : emb + (ci - Sn) * d;
    float dist;
    (void)ref_distance(plan, scratch[wave], emb + j * d, ei, metric, lane, &dist, false);
    if (lane == 0) row[p] = dist <= tolerance ? dist : __builtin_nanf("");
  }
}

// the lesser of two (dist, slot) pairs: dist as a number, ties to the lower slot
__device__ __forceinline__ void track_min2(float& d, int& t, float od, int ot) {
  if (od < d || (od == d && ot < t)) d = od, t = ot;
}

constexpr int kNoSlot = 0x7fffffff;

// the nearest open tail of the face whose candidate row is `row`: one wave, every lane returns it.  tail_ring: the ring
// slot of every table slot (-1: no face there), open: the ring's flags
__device__ __forceinline__ void track_nearest(const float* __restrict__ row, const short* tail_ring, const int* open, int T, int lane, float* bd,
                                              int* bt) {
  float d = __builtin_inff();
  int t = kNoSlot;
  for (int s = lane; s < T; s += 64) {
    const float v = row[s];
    const int rs = tail_ring[s];
    if (rs >= 0 && open[rs] && v == v && (t == kNoSlot || v < d)) d = v, t = s;   // (s ascends: a tie keeps the lower slot)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float od = __shfl_xor(d, off);
    const int ot = __shfl_xor(t, off);
    track_min2(d, t, od, ot);
  }
  *bd = d;
  *bt = t;
}

// The walk shares nothing between its threads but LDS: the last G frames -- the only ones a face can continue -- live in
// a ring of G x K slots (label, age, open flag; per frame its number of unclipped faces, the global row and the `closed`
// index of its position 0), frame cf in ring frame cf % G.  Global memory is read for `offsets` and the candidate table
// and written for the outputs, so the barriers are LDS-only (lds_barrier): __syncthreads() would wait at every pick for the
// stores of the pick before, and a link costs three barriers.
__global__ __launch_bounds__(kWalkThreads) void tracks_walk_kernel(const TrackSeq q, const float* __restrict__ cand, int* __restrict__ closed,
                                                                   int64_t row_base, int64_t* __restrict__ prev, float* __restrict__ link_dist,
                                                                   int64_t* __restrict__ labels, int64_t* __restrict__ age,
                                                                   int64_t* __restrict__ n_new, int64_t* __restrict__ clipped_out) {
  __shared__ int64_t ring_label[kTrackSlots], ring_age[kTrackSlots];
  __shared__ int ring_open[kTrackSlots];
  __shared__ int64_t ring_row0[kTrackGap], ring_c0[kTrackGap];
  __shared__ int ring_cnt[kTrackGap];
  __shared__ short tail_ring[kTrackSlots];      // per slot of the frame's table: the tail's ring slot, or -1 (closed tails too)
  __shared__ float best_d[kTrackKmax];
  __shared__ int best_t[kTrackKmax], taken[kTrackKmax];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = q.G, K = q.K, T = G * K;
  const int Sn = G * q.Ks;                      // (rows, frames and counts fit an int: dif_tracks_link checks m and n_frames)
  // the state's frames are frames 0 .. G - 1; its closed flags also go to `closed` ([state slots][rows of the call], the
  // rows zeroed in front of this kernel), where tracks_state_kernel finds them
  {
    const TrackState st = track_state_in(q);
    for (int s = tid; s < T; s += kWalkThreads) {
      const int f = s / K, p = s - f * K;
      const bool have = q.state && p < q.Ks && p < st.count[f];
      const int c = f * q.Ks + p;
      ring_label[s] = have ? st.labels[c] : -1;
      ring_age[s] = have ? st.age[c] : 0;
      ring_open[s] = have && !st.closed[c];
    }
    for (int s = tid; s < Sn; s += kWalkThreads) closed[s] = st.closed[s];
    if (tid < G) {
      const int have = q.state ? st.count[tid] : 0;
      ring_cnt[tid] = have < q.Ks ? have : q.Ks;
      ring_row0[tid] = have > 0 ? st.rows[tid * q.Ks] : 0;
      ring_c0[tid] = (int64_t)tid * q.Ks;
    }
  }
  __syncthreads();                              // global too: thread 0 later stores 1 into words of `closed` that other threads copied above
  if (tid < q.pad) ring_cnt[(G + tid) % G] = 0;   // the frames the caller skipped (pad <= G)
  int links = 0, clipped = 0, faces = 0;        // (faces: the rows the frames cover -- m when offsets is what dif.h asks for)
  const int N = (int)q.n_frames, M = (int)q.m;
  // frame_rows' clamps, in ints: offsets[n + 1] closes frame n and opens the next, offsets[n + 2] is requested a frame ahead
  auto clamped = [&](int64_t v) { return (int)(v < 0 ? 0 : (v > M ? M : v)); };
  int off_e = N > 0 ? clamped(q.offsets[0]) : 0, off_next = N > 0 ? clamped(q.offsets[1]) : 0;
  for (int n = 0; n < N; ++n) {
    const int b = off_e;
    off_e = off_next;
    const int e = off_e < b ? b : off_e;
    off_next = n + 2 <= N ? clamped(q.offsets[n + 2]) : 0;
    const int cnt = e - b;
    faces += cnt;
    const int cf = G + q.pad + n;               // (n_frames <= 2^30)
    const int slot = cf % G;                    // the ring frame this frame takes over: frame cf - G's, a tail of it until then
    if (cnt == 0) {                             // (uniform: every thread reads the same offsets)
      if (tid == 0) ring_cnt[slot] = 0;
      continue;
    }
    const int nj = cnt < q.kmax ? cnt : q.kmax;
    clipped += cnt - nj;
    lds_barrier();                              // the ring as the frames before left it
    for (int s = tid; s < T; s += kWalkThreads) {
      const int gi = s / K, p = s - gi * K;       // table slot = (G - g) * K + p: the tail at position p of frame cf - G + gi
      const int rf = (cf - G + gi) % G;
      tail_ring[s] = p < ring_cnt[rf] ? (short)(rf * K + p) : (short)-1;
    }
    if (tid < kTrackKmax) taken[tid] = 0;
    lds_barrier();
    for (int j = wave; j < nj; j += kWalkWaves) {
      float d;
      int t;
      track_nearest(cand + (int64_t)(b + j) * T, tail_ring, ring_open, T, lane, &d, &t);
      if (lane == 0) best_d[j] = d, best_t[j] = t;
    }
    lds_barrier();
    for (int pick = 0; pick < nj; ++pick) {
      // every wave finds the same least (dist, tail, face) from the same LDS words
      float d = __builtin_inff();
      int t = kNoSlot, jj = lane;
      if (lane < nj && !taken[lane]) d = best_d[lane], t = best_t[lane];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float od = __shfl_xor(d, off);
        const int ot = __shfl_xor(t, off), oj = __shfl_xor(jj, off);
        if (od < d || (od == d && (ot < t || (ot == t && oj < jj)))) d = od, t = ot, jj = oj;
      }
      if (t == kNoSlot) break;                  // (uniform) no face of the frame has an open tail left
      ++links;
      lds_barrier();                            // every wave has read taken / best_* of this pick
      if (tid == 0) {
        const int rs = tail_ring[t], rf = rs / K, p = rs - rf * K, r = b + jj;
        prev[r] = ring_row0[rf] + p;
        link_dist[r] = d;
        labels[r] = ring_label[rs];
        age[r] = ring_age[rs] + 1;
        closed[ring_c0[rf] + p] = 1;
        ring_open[rs] = 0;
        taken[jj] = 1 + rs;                     // (the tail it continues: its label and age move to the face's ring slot below)
      }
      lds_barrier();
      for (int j = wave; j < nj; j += kWalkWaves) {
        if (taken[j] || best_t[j] != t) continue;   // (uniform over the wave)
        float nd;
        int nt;
        track_nearest(cand + (int64_t)(b + j) * T, tail_ring, ring_open, T, lane, &nd, &nt);
        if (lane == 0) best_d[j] = nd, best_t[j] = nt;
      }
      lds_barrier();
    }
    lds_barrier();                              // (the break leaves in front of the pick's barriers)
    // the frame's faces: the outputs of the starts, and -- first read, then written, a tail may sit in the ring frame that
    // this frame takes over -- the ring's new frame
    int64_t lab = 0, ag = 0;                    // (nj <= 64: a thread holds one face)
    if (tid < nj) {
      const int rs = taken[tid] - 1;
      lab = rs >= 0 ? ring_label[rs] : row_base + b + tid;
      ag = rs >= 0 ? ring_age[rs] + 1 : 1;
    }
    for (int j = tid; j < cnt; j += kWalkThreads) {
      if (j < nj && taken[j]) continue;
      const int64_t r = b + j;
      prev[r] = -1;
      link_dist[r] = __builtin_nanf("");
      labels[r] = row_base + r;
      age[r] = 1;
    }
    lds_barrier();
    if (tid < nj) {
      ring_label[slot * K + tid] = lab;
      ring_age[slot * K + tid] = ag;
      ring_open[slot * K + tid] = 1;
    }
    if (tid == 0) {
      ring_cnt[slot] = nj;
      ring_row0[slot] = row_base + b;
      ring_c0[slot] = (int64_t)Sn + b;
    }
  }
  if (tid == 0) {
    n_new[0] = faces - links;
    clipped_out[0] = clipped;
  }
}

// Block (t, p): slot p of frame pad + N + t -- the last G frames -- of the next state.
__global__ __launch_bounds__(256) void tracks_state_kernel(const TrackSeq q, const float* __restrict__ boxes, const float* __restrict__ emb, int d,
                                                           const int* __restrict__ closed, int64_t row_base,
                                                           const int64_t* __restrict__ labels, const int64_t* __restrict__ age,
                                                           const TrackState out, int Ko) {
  const int t = blockIdx.x / Ko, p = blockIdx.x - t * Ko;
  const int64_t cf = (int64_t)q.pad + q.n_frames + t;
  const int64_t c = track_tail(q, cf, p);
  const int64_t Sn = (int64_t)q.G * q.Ks;
  const int64_t o = (int64_t)t * Ko + p;
  const bool old = c >= 0 && c < Sn;
  const TrackState st = track_state_in(q);
  const float* __restrict__ src = c < 0 ? nullptr : (old ? st.emb + c * d : emb + (c - Sn) * d);
  float* __restrict__ dst = out.emb + o * d;
  for (int k = threadIdx.x; k < d; k += 256) dst[k] = src ? src[k] : 0.f;
  if (threadIdx.x < 4) {
    const float* sb = c < 0 ? nullptr : (old ? st.boxes + c * 4 : boxes + (c - Sn) * 4);
    out.boxes[o * 4 + threadIdx.x] = sb ? sb[threadIdx.x] : 0.f;
  }
  if (threadIdx.x == 0) {
    out.labels[o] = c < 0 ? -1 : (old ? st.labels[c] : labels[c - Sn]);
    out.age[o] = c < 0 ? 0 : (old ? st.age[c] : age[c - Sn]);
    out.rows[o] = c < 0 ? -1 : (old ? st.rows[c] : row_base + (c - Sn));
    out.closed[o] = c < 0 ? 1 : closed[c];
    if (blockIdx.x == 0 && out.tail) *out.tail = 0;           // every byte of the buffer is written: equal calls, equal states
    if (p == 0) {
      int have = 0;                             // the faces of the frame that take part: they fill slots 0 .. have - 1
      while (have < Ko && track_tail(q, cf, have) >= 0) ++have;
      out.count[t] = have;
    }
  }
}

}  // namespace dif

using namespace dif;

// the workspace: the candidate table [m][G * K] and the closed flags [state slots][rows of the call]
static size_t track_carve(void* base, int64_t m, int G, int K, int Ks, float** cand, int** closed) {
  Carver c(base);
  *cand = (float*)c.take((size_t)m * G * K * 4);
  *closed = (int*)c.take(((size_t)G * Ks + (size_t)m) * 4);
  return c.at;
}

static int track_check_shape(const char* fn, int max_gap, int k, int d) {
  if (max_gap < 1 || max_gap > kTrackGap) return set_error("%s: max_gap %d outside [1, %d]", fn, max_gap, kTrackGap);
  if (k < 1 || k > kTrackKmax) return set_error("%s: %d faces per frame outside [1, %d]", fn, k, kTrackKmax);
  if (d <= 0 || d > 8192) return set_error("%s: embedding size %d outside [1, 8192]", fn, d);
  return 0;
}

extern "C" {

int64_t dif_tracks_state_size(int max_gap, int k, int d) {
  if (track_check_shape("dif_tracks_state_size", max_gap, k, d)) return -1;
  TrackState s;
  return (int64_t)track_state_carve(nullptr, max_gap, k, d, &s);
}

int64_t dif_tracks_workspace_size(int64_t m, int max_gap, int kmax, int state_k) {
  if (m < 0 || m > 0x7fffffff) return set_error("dif_tracks_workspace_size: m %lld out of range", (long long)m);
  if (state_k != 0 && track_check_shape("dif_tracks_workspace_size", max_gap, state_k, 1)) return -1;
  if (track_check_shape("dif_tracks_workspace_size", max_gap, kmax, 1)) return -1;
  const int K = kmax > state_k ? kmax : state_k;
  float* cand;
  int* closed;
  return (int64_t)track_carve(nullptr, m, max_gap, K, state_k, &cand, &closed);
}

int dif_tracks_link(const int64_t* offsets_dev, const float* boxes_dev, const float* emb_dev, int64_t n_frames, int64_t m, int d,
                    float tolerance, float min_iou, int max_gap, int metric, int kmax, int64_t row_base, const void* state_in_dev,
                    int state_k_in, int64_t state_pad, int64_t* prev_out_dev, float* link_dist_out_dev, int64_t* labels_out_dev,
                    int64_t* age_out_dev, int64_t* n_new_out_dev, int64_t* clipped_out_dev, void* state_out_dev, int state_k_out,
                    void* workspace_dev, int64_t workspace_bytes, int passes, void* stream) {
  const char* fn = "dif_tracks_link";
  if (track_check_shape(fn, max_gap, kmax, d)) return -1;
  if (metric != 0 && metric != 1) return set_error("%s: unknown metric %d", fn, metric);
  if (passes < 0 || passes > 7) return set_error("%s: passes %d is no set of DIF_TRACKS_PASS_*", fn, passes);
  if (passes == 0) passes = DIF_TRACKS_PASS_CAND | DIF_TRACKS_PASS_WALK | DIF_TRACKS_PASS_STATE;
  if (n_frames < 0 || m < 0 || n_frames > 0x40000000 || m > 0x7fffffff)
    return set_error("%s: sizes out of range (%lld frames, %lld faces)", fn, (long long)n_frames, (long long)m);
  if (m > 0 && n_frames == 0) return set_error("%s: %lld faces in no frame", fn, (long long)m);
  if (row_base < 0 || state_pad < 0) return set_error("%s: negative row_base or state_pad", fn);
  if (!state_in_dev) state_k_in = 0;
  if (state_in_dev && track_check_shape(fn, max_gap, state_k_in, d)) return -1;
  if (!offsets_dev || !n_new_out_dev || !clipped_out_dev) return set_error("%s: null pointer", fn);
  if (m > 0 && (!boxes_dev || !emb_dev || !prev_out_dev || !link_dist_out_dev || !labels_out_dev || !age_out_dev || !workspace_dev))
    return set_error("%s: null pointer", fn);
  if (((uintptr_t)state_in_dev | (uintptr_t)state_out_dev | (uintptr_t)workspace_dev) & 7)
    return set_error("%s: state and workspace must be aligned to 8 bytes", fn);
  if (state_out_dev) {
    if (track_check_shape(fn, max_gap, state_k_out, d)) return -1;
    if (state_k_out < kmax || state_k_out < state_k_in)
      return set_error("%s: state_k_out %d below kmax %d or state_k_in %d", fn, state_k_out, kmax, state_k_in);
  }
  const int64_t need = dif_tracks_workspace_size(m, max_gap, kmax, state_k_in);
  if (need < 0) return -1;
  if (need > 0 && (!workspace_dev || workspace_bytes < need))
    return set_error("%s: workspace of %lld bytes, %lld needed (dif_tracks_workspace_size)", fn, (long long)workspace_bytes, (long long)need);
  if (m * max_gap > 0x7fffffffll) return set_error("%s: %lld faces x max_gap %d out of range", fn, (long long)m, max_gap);
  SumPlan plan;
  if (make_sum_plan(d, &plan)) return -1;
  hipStream_t st = (hipStream_t)stream;
  TrackSeq q;
  q.offsets = offsets_dev;
  q.n_frames = n_frames;
  q.m = m;
  q.G = max_gap;
  q.kmax = kmax;
  q.Ks = state_k_in;
  q.pad = (int)(state_pad < max_gap ? state_pad : max_gap);   // (max_gap empty frames put every stored face out of reach)
  q.K = kmax > state_k_in ? kmax : state_k_in;
  q.state = state_in_dev;
  q.d = d;
  float* cand;
  int* closed;
  track_carve(workspace_dev, m, max_gap, q.K, state_k_in, &cand, &closed);
  if (m > 0 && (passes & DIF_TRACKS_PASS_CAND))
    hipLaunchKernelGGL(tracks_cand_kernel, dim3((unsigned)(m * max_gap)), dim3(256), 0, st, q, boxes_dev, emb_dev, d, tolerance, min_iou, metric,
                       plan, cand);
  if (m > 0 && (passes & DIF_TRACKS_PASS_WALK)) DIF_HIP(hipMemsetAsync(closed + (size_t)max_gap * state_k_in, 0, (size_t)m * 4, st));
  if (passes & DIF_TRACKS_PASS_WALK)
    hipLaunchKernelGGL(tracks_walk_kernel, dim3(1), dim3(kWalkThreads), 0, st, q, cand, closed, row_base, prev_out_dev, link_dist_out_dev,
                       labels_out_dev, age_out_dev, n_new_out_dev, clipped_out_dev);
  if (state_out_dev && (passes & DIF_TRACKS_PASS_STATE)) {
    TrackState out;
    track_state_carve(state_out_dev, max_gap, state_k_out, d, &out);
    hipLaunchKernelGGL(tracks_state_kernel, dim3((unsigned)(max_gap * state_k_out)), dim3(256), 0, st, q, boxes_dev, emb_dev, d, closed,
                       row_base, labels_out_dev, age_out_dev, out, state_k_out);
  }
  DIF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
