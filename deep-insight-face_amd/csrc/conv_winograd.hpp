// conv_wino_kernel: Winograd F(2x2, 3x3) for the large-batch 3x3 / stride 1 / pad 1 layers -- one kernel template in three block
// shapes (WinoW, below) on even maps, and the half block in two more forms (WinoX) on odd maps and sub-sampled outputs.  Included by conv.hip (inside namespace dif, after the helpers it uses).
//
// A 3x3 convolution of a 4x4 input tile d is Y = A^T [ (G g G^T) .* (B^T d B) ] A: 2x2 outputs from 16 element-wise
// products, i.e. 16 GEMMs M_c[tile][co] = sum_ci V_c[tile][ci] U_c[ci][co] with K = Cin instead of one with K = 9 Cin --
// 2.25x fewer multiply-adds.  Every value stays f32 (v_mfma_f32_32x32x2_f32, f32 transforms); U = G g G^T is formed on
// the host in double and rounded once (net.hip: finalize, ConvArgs::w_wino).  The products differ from the direct fma
// chain: the per-layer error is about twice the direct path's (tools/winograd_error.py, profiles/r06_winograd_error.txt).
//
// Block: TT Winograd tiles (numbered linearly over image x tile grid, so a block may span images) x 64 output channels
// x all 16 components on 16 / CPW waves; wave w owns components CPW w .. CPW w + CPW - 1 in the eight-wave shapes and
// w, 4 + w, 8 + w, 12 + w -- a column of the 4 x 4 grid -- in the four-wave ones (TT / 32 row fragments x two
// 32-channel column fragments each: 128 accumulators per lane in every shape).  Per K-step of 16 input channels every
// thread fetches one 4x4 input tile of two channels (zero halo from out-of-range buffer loads), forms its 16 V values and
// writes them to LDS ([component][tile][16 ch], 16-byte chunks XOR-swizzled by tile); two such stages alternate, one
// barrier per K-step.  A operands come from LDS, B operands (U in fragment order: 1 KB per wave instruction) straight
// from L2; both sit in two register sets, component j in set j & 1, fetched two components ahead (B across the K-step
// boundary; in the four-wave shapes B comes in half sets, each re-filled behind the eight MFMAs that read it, 24 MFMAs
// ahead of its next use: WinoW::B_HALVES).  The K loop runs every step but the last with all its
// loads unconditional and the last step peeled; the
// next step's tile loads are issued half a step in, behind the B loads of the second half, and first waited on by the
// transform at the end of the step (vmcnt retires in order: what is issued behind them would wait for them).  The
// compiled order of issue, waits and registers of every instantiation: profiles/r11_wino_kloop_isa.txt, DESIGN 4b.
// The epilogue of the eight-wave shapes stages M in LDS one 32-channel half at a time, applies A^T M A and epilogue4
// (conv.hip).  In the four-wave shapes (WinoW::ONE_PASS) every wave first sums its grid column on its own accumulators
// -- s0 = (m0 + m1) + m2, s1 = (m1 - m2) - m3, the first stage of A^T M A in the order the two-pass form uses -- so eight
// planes instead of sixteen go through LDS, both halves in one pass with one barrier, and the shortcut tiles of both
// halves are requested inside the peeled last K-step, into the tile loader's registers.
// Every accumulator sums the same products in the same order in every shape, and every output the same terms in the same
// order in both epilogues: the block shape changes no bit.
namespace wino {
constexpr int BN = 64;                         // output channels per block
constexpr int KC = 16;                         // input channels per K-step
// fewest Winograd tiles per launch (a pure function of the layer shape and the batch): 64 images of 14 x 14.  Below it
// the layer stays on the direct kernels -- the split-K / one-image paths of the small batches among them
constexpr int64_t MIN_TILES = 64 * 49;
// the wide maps (level 2): map sides up to 112, and at least 128 images per launch
constexpr int WIDE_MAX_HW = 112;
constexpr int64_t WIDE_MIN_IMAGES = 128;
// the rest (level 2, class 3 of wino_applies): odd maps from 3 x 3 to 16 x 16 (a side of 1 or 2 is half padding: no fewer
// multiply-adds than direct, and more blocks than the 64-pixel tiles the trace buffer is sized by) with at least the tiles of
// 128 images of 7 x 7,
// and even maps whose first output is sub-sampled (ConvArgs::y_sub); both from WIDE_MIN_IMAGES images per launch up
constexpr int ODD_MAX_HW = 16;
constexpr int64_t ODD_MIN_TILES = 128 * 16;
}  // namespace wino

#ifndef DIF_WINO_RES_UNDER_K
#define DIF_WINO_RES_UNDER_K 1                 // (WinoW::RES_UNDER_K)
#endif
#ifndef DIF_WINO_B_HALVES
#define DIF_WINO_B_HALVES 1                    // (WinoW::B_HALVES)
#endif

// The block shapes.
// <64, 2, 1, false>: 64 tiles on eight waves, 128 KiB of LDS, one block per CU -- the narrow maps (at most 16 x 16: IResNet's
//   14 x 14 stage) at option "wino" = 1 [and at level 2 under dbg bit 16777216, A/B].  K = 256 .. 512 is 16 .. 32 K-steps,
//   which cover the fixed part of a block (set-up: first tile fetch, transform, barrier; epilogue: two LDS round trips of
//   M, output transform, stores).
// <32, 4, 2, true>: half the block, 32 tiles on four waves, 64 KiB -- two blocks per CU, so one block's epilogue and set-up
//   run under the other's MFMAs and a K-step barrier holds four waves instead of eight.  The price is U traffic from L2
//   per MFMA doubled (a B fragment feeds one row fragment, not two).  Level 2 runs everything in this shape.  The wide
//   maps (above 16 x 16 up to 112 x 112: IResNet's 28 x 28, 56 x 56 and 112 x 112 stages) have 128 or 64 input channels: a
//   K loop of 8 or 4 steps leaves set-up and epilogue uncovered for a third to a half of a full-size block's life.  On the
//   narrow maps the fixed part is a smaller share, but 784 blocks of 64 tiles on 256 CUs are 3.06 rounds paid as 4; half
//   blocks halve the quantum: a CU's share of 3.06 full-size blocks of work is paid as 3.5 (seven half blocks).
// <64, 2, 2, true>: the full-size block on the wide maps, kept for A/B runs [dbg bit 65536].
// EARLY_REQ: the epilogue requests each half's shortcut tile and BN / PReLU vectors before M goes to LDS (the operand
// registers of the K loop are dead by then), so their latency is not paid after the staging barrier; the level 1 shape
// requests them after the output transform, as it always has.  (Read by the two-pass epilogue only, i.e. by <64, 2, 2, true>
// and <64, 2, 1, false>: the four-wave shapes' one-pass epilogue requests the vectors behind the K loop and the shortcut
// tiles inside its last step: ONE_PASS, RES_UNDER_K.)
template <int TT_, int CPW_, int MIN_BLOCKS_, bool EARLY_REQ_>
struct WinoW {
  static constexpr int TT = TT_;                             // Winograd tiles per block
  static constexpr int CPW = CPW_;                           // components per wave
  static constexpr int MIN_BLOCKS = MIN_BLOCKS_;             // blocks per CU the launch bound asks for
  static constexpr bool EARLY_REQ = EARLY_REQ_;
  static constexpr bool ODD = false;                         // (WinoX, below)
  static constexpr bool YSUB = false;
  static constexpr int MF = TT / 32;                         // 32-tile row fragments per component
  static constexpr int NT = 16 / CPW * 64;                   // threads per block (NT / 8 == TT: one tile x two channels each)
  static constexpr int STAGE = 16 * TT * wino::KC;           // floats per V stage
  static constexpr int LDS_BYTES = 2 * STAGE * 4;            // the epilogue's M half (16 x TT x 32 floats) fits the same
  // The four-wave shapes: wave w owns the COLUMN w, 4 + w, 8 + w, 12 + w of the 4 x 4 component grid, so the first stage
  // of A^T M A (over the grid's rows) is the wave's own and eight planes, not sixteen, go through LDS: all 64 channels
  // in one pass (8 x 32 tiles x 64 channels = LDS_BYTES).  The eight-wave shapes own rows, CPW w .. CPW w + CPW - 1.
  static constexpr bool ONE_PASS = CPW_ == 4;
  static constexpr int COMP_W = ONE_PASS ? 1 : CPW_;          // component j of wave w is COMP_W w + COMP_J j
  static constexpr int COMP_J = ONE_PASS ? 4 : 1;
  // ONE_PASS: the shortcut tiles of both column fragments are requested inside the peeled last K-step, into the registers
  // the tile loader has left (-DDIF_WINO_RES_UNDER_K=0 requests them behind the K loop instead: the A/B build of round 12)
  static constexpr bool RES_UNDER_K = ONE_PASS && DIF_WINO_RES_UNDER_K;
  // The four-wave shapes: a component's B operands are fetched as two halves (k quads 0 and 1: the operands of its first
  // and of its last eight MFMAs), each right behind the eight MFMAs that read the registers it overwrites -- 24 MFMAs
  // (1 536 cycles) ahead of its first use, where a whole set behind the component's last MFMA is 16 ahead.  A wave alone
  // on its SIMD waited on B in front of every component (profiles/r13_wino_block_trace.txt).
  // -DDIF_WINO_B_HALVES=0 builds whole sets, the loop the eight-wave shapes keep: the A/B build of round 13
  static constexpr bool B_HALVES = CPW_ == 4 && DIF_WINO_B_HALVES;
  static_assert(NT / 8 == TT && CPW % 2 == 0, "one loader thread per (tile, channel pair)");
  static_assert(!ONE_PASS || (TT == 32 && 8 * TT * wino::BN * 4 <= LDS_BYTES), "one pass: eight planes of 32 tiles x 64 channels");
};

// The half block on the layers the even-map rule leaves out (wino_applies: 3), one form each:
// ODD: a map with an odd side.  The tile grid is (H + 1) / 2 x (W + 1) / 2, i.e. the map zero-padded to even sides: vmask
//   zeroes the input points beyond it as it does the halo, and the epilogue masks the output pixels of the row / column
//   beyond it (shortcut load and both stores).  IResNet's 7 x 7 stage: 16 tiles per image for 49 pixels, 49 / 64 of 2.25x.
// YSUB: an even map whose first output keeps the even pixels only (ConvArgs::y_sub): that pixel is output (0, 0) of its
//   tile and its dense index is the tile's, g.  The second output and the shortcut are whole.
template <bool ODD_, bool YSUB_>
struct WinoX : WinoW<32, 4, 2, true> {
  static constexpr bool ODD = ODD_;
  static constexpr bool YSUB = YSUB_;
  static_assert(!(ODD_ && YSUB_), "y_sub is admitted on even maps only");
};

// B^T x for one 4-vector: (x0 - x2, x1 + x2, x2 - x1, x1 - x3)
__device__ __forceinline__ void wino_bt4(float x0, float x1, float x2, float x3, float& o0, float& o1, float& o2, float& o3) {
  o0 = x0 - x2;
  o1 = x1 + x2;
  o2 = x2 - x1;
  o3 = x1 - x3;
}

// V = B^T d B of one 4x4 tile (d[4 r + c]), component c of V at v[c]
__device__ __forceinline__ void wino_input_transform(const float (&d)[16], float (&v)[16]) {
  float t[16];
#pragma unroll
  for (int c = 0; c < 4; ++c) wino_bt4(d[c], d[4 + c], d[8 + c], d[12 + c], t[c], t[4 + c], t[8 + c], t[12 + c]);
#pragma unroll
  for (int r = 0; r < 4; ++r) wino_bt4(t[4 * r], t[4 * r + 1], t[4 * r + 2], t[4 * r + 3], v[4 * r], v[4 * r + 1], v[4 * r + 2], v[4 * r + 3]);
}

// Block trace (ConvArgs::trace, net.hip: option dbg = 256): the TRACE instantiations stamp the block's start, the first
// barrier, the end of the K loop and the end of each epilogue half in 100 MHz ticks; thread 0 writes the eight-word record
// of the direct kernels with low byte 3: [K loop, set-up, epilogue half 0, epilogue half 1, HW_ID | XCC_ID << 32, start,
// end, 3 | cycles << 8].  The one-pass shapes put "stage" (K-loop end to the staging barrier: requests, first stage, LDS
// writes) and "finish" (LDS reads, second stage, epilogue4, stores) in the two epilogue words.  The launcher picks TRACE = false whenever trace is null: that code holds no stamp and no branch
// on trace (a branch alone moved the register allocation of these kernels, which sit at the 256-VGPR limit).
template <bool TRACE>
__device__ __forceinline__ unsigned long long wino_stamp() {
  if constexpr (TRACE) return __builtin_amdgcn_s_memrealtime();
  return 0ull;
}
__device__ __forceinline__ void wino_trace_write(const ConvArgs& a, unsigned long long c0, const unsigned long long (&ts)[5]) {
  unsigned long long* t = a.trace + (size_t)blockIdx.x * 8;
  t[0] = ts[2] - ts[1];
  t[1] = ts[1] - ts[0];
  t[2] = ts[3] - ts[2];
  t[3] = ts[4] - ts[3];
  t[4] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
  t[5] = ts[0];
  t[6] = ts[4];
  t[7] = 3 | ((__builtin_amdgcn_s_memtime() - c0) << 8);
}

template <class S, bool TRACE>
__global__ __launch_bounds__(S::NT, S::MIN_BLOCKS) void conv_wino_kernel(const ConvArgs a, int blocks_m, int nblocks) {
  constexpr int TT = S::TT, CPW = S::CPW, MF = S::MF, KC = wino::KC;
  extern __shared__ __attribute__((aligned(16))) float wino_smem[];
  const int b = xcd_remap((int)blockIdx.x, nblocks);
  const int nt = b / blocks_m, mt = b - nt * blocks_m;   // column-slice-major: an XCD's blocks share one slice of U in its L2
  const int tid = threadIdx.x, lane = tid & 63;
  // (WinoX: the wave's number in a scalar register.  With it in a vector register the y_sub form, which carries one more
  // value across the K loop, spilled the wave's LDS base to scratch; in the WinoW shapes it stays where it always was)
  const int wave = (S::ODD || S::YSUB) ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  const int tw = S::ODD ? (a.W + 1) >> 1 : a.W >> 1, tpi = (S::ODD ? (a.H + 1) >> 1 : a.H >> 1) * tw, ntiles = a.N * tpi;
  const int KS = a.Cin / KC;
  unsigned long long ts[5];
  ts[0] = wino_stamp<TRACE>();
  const unsigned long long tr_c0 = TRACE ? __builtin_amdgcn_s_memtime() : 0ull;

  // ---- this thread's tile: the input loader's (two channels) and the epilogue's (four channels) alike
  const int ltile = tid >> 3, cp = tid & 7;
  const int g = mt * TT + ltile;
  const bool tile_ok = g < ntiles;
  int pix0 = 0;                                  // first output pixel (2 ty, 2 tx) of the tile, linear over N x H x W
  unsigned vmask = 0;                            // in-range points of the 4x4 input tile
  if (tile_ok) {
    const int img = g / tpi, rem = g - img * tpi, ty = rem / tw, tx = rem - ty * tw;
    pix0 = (img * a.H + 2 * ty) * a.W + 2 * tx;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int iy = 2 * ty - 1 + (p >> 2), ix = 2 * tx - 1 + (p & 3);
      if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) vmask |= 1u << p;
    }
  }
  const int row_b = a.W * a.Cin * 4, pix_b = a.Cin * 4;
  // byte offset of point (0, 0) of the tile (one row and column before pix0; only in-range points are ever added to it)
  const int lbase = (pix0 - a.W - 1) * pix_b + cp * 8;
  const __amdgpu_buffer_rsrc_t xrs = make_rsrc(a.x, (uint32_t)a.N * (uint32_t)(a.H * a.W) * (uint32_t)pix_b);
  auto dload = [&](int ks, f32x2 (&d)[16]) {
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const uint32_t off = ((vmask >> p) & 1u) ? (uint32_t)(lbase + (p >> 2) * row_b + (p & 3) * pix_b + ks * (KC * 4)) : OOB;
      d[p] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(xrs, off, 0, 0));
    }
  };
  const int vdst = ltile * KC + (((cp >> 1) ^ ((ltile >> 2) & 3)) << 2) + (cp & 1) * 2;
  auto vstore = [&](float* buf, const f32x2 (&d)[16]) {
    float d0[16], d1[16], v0[16], v1[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      d0[p] = d[p][0];
      d1[p] = d[p][1];
    }
    wino_input_transform(d0, v0);
    wino_input_transform(d1, v1);
#pragma unroll
    for (int c = 0; c < 16; ++c) *reinterpret_cast<f32x2*>(buf + c * (TT * KC) + vdst) = f32x2{v0[c], v1[c]};
  };

  // ---- operands of this wave's components: two register sets, component j in set j & 1
  const int h = lane >> 5, r32 = lane & 31, sw = (r32 >> 2) & 3;
  const int tiles_n = a.Cout / wino::BN;
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(a.w_wino, a.w_wino_bytes);
  const uint32_t boff0 = (uint32_t)((S::COMP_W * wave * tiles_n + nt) * KS) * 4096u + (uint32_t)lane * 16u;
  const uint32_t bstep = (uint32_t)(S::COMP_J * tiles_n * KS) * 4096u;     // the wave's next component
  f32x4 bw[2][2][2];                             // [set][column fragment][k quad]
  auto bload = [&](int j, int ks) {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int q = 0; q < 2; ++q)
        bw[j & 1][nf][q] = buf_load4(wrs, boff0 + (uint32_t)j * bstep + (uint32_t)ks * 4096u + (uint32_t)(nf * 2 + q) * 1024u);
  };
  // lane half h consumes channels 8 h + 4 q + t of the K-step in sub-step s = 4 q + t (U is stored in the same order)
  int aoff[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) aoff[q] = r32 * KC + (((2 * h + q) ^ sw) << 2);
  f32x4 av[2][MF][2];                            // [set][row fragment][k quad]
  auto aread = [&](const float* buf, int j) {
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int q = 0; q < 2; ++q)
        av[j & 1][mf][q] = *reinterpret_cast<const f32x4*>(buf + (S::COMP_W * wave + S::COMP_J * j) * (TT * KC) + mf * 32 * KC + aoff[q]);
  };
  f32x16 acc[CPW][MF][2];                        // [component][row fragment][column fragment]
#pragma unroll
  for (int j = 0; j < CPW; ++j)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][mf][nf][r] = 0.f;
  auto mfma = [&](int j) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf)
#pragma unroll
          for (int nf = 0; nf < 2; ++nf)
            acc[j][mf][nf] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j & 1][mf][q][t], bw[j & 1][nf][q][t], acc[j][mf][nf], 0, 0, 0);
  };

  // (B_HALVES) k quad q of component j alone: the B loads of its two column fragments, and the eight MFMAs that read them
  // (mfma(j) is mfma_half(j, 0) then mfma_half(j, 1): the same MFMAs in the same order)
  auto bload_half = [&](int j, int ks, int q) {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
      bw[j & 1][nf][q] = buf_load4(wrs, boff0 + (uint32_t)j * bstep + (uint32_t)ks * 4096u + (uint32_t)(nf * 2 + q) * 1024u);
  };
  auto mfma_half = [&](int j, int q) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
          acc[j][mf][nf] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j & 1][mf][q][t], bw[j & 1][nf][q][t], acc[j][mf][nf], 0, 0, 0);
  };

  // ---- (ONE_PASS) the byte offsets of the tile's four outputs in both column fragments, for the shortcut loads and the stores
  // alike, and the request of the shortcut tiles.  The request is unconditional: without a shortcut the descriptor has size
  // zero and the loads return 0 without touching memory (a run-time branch inside the peeled K-step would bring two paths
  // to one label and with them the wait counts of the path without the loads).
  uint32_t voff8[2][4];
  f32x4 rv8[2][4];
  auto res_request = [&]() {
    const __amdgpu_buffer_rsrc_t res_rsrc = make_rsrc(a.res, a.res ? (uint32_t)a.M * (uint32_t)a.Cout * 4u : 0u);
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int pix = pix0 + (p >> 1) * a.W + (p & 1), c = nt * wino::BN + nf * 32 + cp * 4;
        // Output p is input point (1 + p / 2, 1 + p % 2) of the tile: its vmask bit says whether it is on the map (ODD) and,
        // on an even map, whether the tile exists at all.  Off the map the offset becomes OOB by arithmetic (the offsets
        // are multiples of 16): written as a select, the compiler made divergent branches of it inside the K-step, a
        // load in each arm, and counted the waits of the MFMAs behind them for the shorter path.
        const uint32_t off_map = ((vmask >> (5 + 4 * (p >> 1) + (p & 1))) & 1u) - 1u;          // 0 on the map, ~0 off it
        voff8[nf][p] = (((uint32_t)pix * (uint32_t)a.Cout + (uint32_t)c) * 4u) | (off_map & OOB);
        rv8[nf][p] = buf_load4(res_rsrc, voff8[nf][p]);
      }
  };

  // ---- main loop
  {
    f32x2 d[16];
    dload(0, d);
    bload(0, 0);
    bload(1, 0);
    vstore(wino_smem, d);
    lds_barrier();
    ts[1] = wino_stamp<TRACE>();
    // One K-step; `last` is a compile-time flag (the final step fetches nothing for a next one).  Every step but the last runs
    // in the loop with all its loads unconditional, the last one is peeled: with the loads under a run-time `more` the
    // two paths met at one label and the waits in front of the first MFMAs were those of the path WITHOUT the tile loads
    // (vmcnt retires in order: a wait counted for the B loads alone drained the tile loads issued just before).
    // Order of issue: the tile loads of step ks + 1 go out after the B loads of this step's second half, so every B wait
    // in front of the second half's MFMAs counts loads issued before them, and they have that half's MFMAs as cover.
    // B_HALVES: the same step with every B set re-filled in two halves, the first in the middle of the component that
    // reads the set, the second where the whole set went; the tile loads keep their place behind the last B load of the
    // first half of the step, and every B wait in front of the second half still counts loads issued before them.
    auto step = [&](int ks, auto last) {
      const float* cur = wino_smem + (ks & 1) * S::STAGE;
      float* nxt = wino_smem + ((ks + 1) & 1) * S::STAGE;
      aread(cur, 0);
      aread(cur, 1);
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        if constexpr (S::B_HALVES) {
          mfma_half(j, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (j + 2 < CPW) bload_half(j + 2, ks, 0);
          else if (!last.value) bload_half(j + 2 - CPW, ks + 1, 0);
          __builtin_amdgcn_sched_barrier(0);
          mfma_half(j, 1);
          __builtin_amdgcn_sched_barrier(0);
          if (j + 2 < CPW) {
            aread(cur, j + 2);
            bload_half(j + 2, ks, 1);
          } else if (!last.value) {
            bload_half(j + 2 - CPW, ks + 1, 1);
          }
        } else {
          mfma(j);
          __builtin_amdgcn_sched_barrier(0);
          if (j + 2 < CPW) {
            aread(cur, j + 2);
            bload(j + 2, ks);
          } else if (!last.value) {
            bload(j + 2 - CPW, ks + 1);
          }
        }
        if (!last.value && j == CPW / 2 - 1) dload(ks + 1, d);
        // (the peeled step has no tile to fetch: d's registers take the shortcut tiles, whose latency then runs under
        // the second half's MFMAs and the epilogue's first stage)
        if (last.value && S::RES_UNDER_K && j == CPW / 2 - 1) res_request();
        __builtin_amdgcn_sched_barrier(0);
      }
      if (!last.value) vstore(nxt, d);
      lds_barrier();
    };
    for (int ks = 0; ks + 1 < KS; ++ks) step(ks, std::false_type{});
    step(KS - 1, std::true_type{});
  }
  ts[2] = wino_stamp<TRACE>();

  // ---- epilogue: per 32-channel half, M through LDS, Y = A^T M A, BN / activation / shortcut / second output
  const int c4 = cp * 4;
  const uint32_t bytes = (uint32_t)a.M * (uint32_t)a.Cout * 4u;
  // (YSUB: the first output is the dense [tile][Cout] tensor of the tiles' (0, 0) pixels)
  const __amdgpu_buffer_rsrc_t y_rsrc = make_rsrc(a.y, a.y ? (S::YSUB ? (uint32_t)ntiles * (uint32_t)a.Cout * 4u : bytes) : 0u);
  const __amdgpu_buffer_rsrc_t y2_rsrc = make_rsrc(a.y2, a.y2 ? bytes : 0u);
  const __amdgpu_buffer_rsrc_t res_rsrc = make_rsrc(a.res, a.res ? bytes : 0u);
  const bool has_res = a.res != nullptr;
  const int act = a.act, act2 = a.act2;
  if constexpr (S::ONE_PASS) {
    // ---- one pass.  Y = A^T M A sums the component grid's rows first: s0[w] = m[w] + m[4 + w] + m[8 + w] and
    // s1[w] = m[4 + w] - m[8 + w] - m[12 + w] have all their operands in wave w's accumulators, element for element.
    // The same adds in the same order as the two-pass form below, so the same bits.
    static_assert(MF == 1 && CPW == 4, "one row fragment, one grid column per wave");
    if constexpr (!S::RES_UNDER_K) res_request();
    // the per-channel vectors of both fragments, into the registers the K loop's operands have left (L2 hits)
    f32x4 sc[2], sh[2], al[2], sc2[2], sh2[2], al2[2];
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const int c = nt * wino::BN + nf * 32 + c4;
      sc[nf] = load4_or(a.scale, c, 1.f), sh[nf] = load4_or(a.shift, c, 0.f), al[nf] = load4_or(a.alpha, c, 0.f);
      sc2[nf] = load4_or(a.scale2, c, 1.f), sh2[nf] = load4_or(a.shift2, c, 0.f), al2[nf] = load4_or(a.alpha2, c, 0.f);
    }
    __builtin_amdgcn_sched_barrier(0);             // (the requests stay above the LDS traffic)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      acc[3][0][nf] = (acc[1][0][nf] - acc[2][0][nf]) - acc[3][0][nf];       // s1[w]
      acc[0][0][nf] = (acc[0][0][nf] + acc[1][0][nf]) + acc[2][0][nf];       // s0[w]
    }
    // plane (s, w) of fragment nf at [(4 s + w) * 2 + nf][tile][32 ch]: the rows of the two-pass layout, so the same
    // conflict-free ds_write_b32 / ds_read_b128 patterns
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        wino_smem[(wave * 2 + nf) * (TT * 32) + frag_row(lane, r) * 32 + r32] = acc[0][0][nf][r];
        wino_smem[((4 + wave) * 2 + nf) * (TT * 32) + frag_row(lane, r) * 32 + r32] = acc[3][0][nf][r];
      }
    lds_barrier();
    ts[3] = wino_stamp<TRACE>();
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      f32x4 s0[4], s1[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        s0[jj] = *reinterpret_cast<const f32x4*>(wino_smem + (jj * 2 + nf) * (TT * 32) + ltile * 32 + c4);
        s1[jj] = *reinterpret_cast<const f32x4*>(wino_smem + ((4 + jj) * 2 + nf) * (TT * 32) + ltile * 32 + c4);
      }
      f32x4 yv[4];                                  // outputs (0,0), (0,1), (1,0), (1,1) of the tile
      yv[0] = s0[0] + s0[1] + s0[2];
      yv[1] = s0[1] - s0[2] - s0[3];
      yv[2] = s1[0] + s1[1] + s1[2];
      yv[3] = s1[1] - s1[2] - s1[3];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f32x4 v, v2;
        epilogue4(yv[p], sc[nf], sh[nf], al[nf], act, has_res, rv8[nf][p], sc2[nf], sh2[nf], al2[nf], act2, v, v2);
        if constexpr (S::YSUB) {
          if (p == 0)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc,
                                                   tile_ok ? ((uint32_t)g * (uint32_t)a.Cout + (uint32_t)(nt * wino::BN + nf * 32 + c4)) * 4u : OOB, 0, 0);
        } else {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, voff8[nf][p], 0, 0);
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v2), y2_rsrc, voff8[nf][p], 0, 0);
      }
    }
    ts[4] = wino_stamp<TRACE>();                   // (no barrier: nothing writes LDS after the last read of a block)
  } else {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const int c = nt * wino::BN + nf * 32 + c4;
      // The half's per-channel vectors and shortcut tile are requested in one of two places (S::EARLY_REQ).  The requests are
      // written out at both: behind a lambda, a member or a free function the 32-tile shape spilled to scratch and the traced
      // 64-tile kernels went from 254 to 256 VGPRs (profiles/r09_wino_unified_isa.txt).
      f32x4 sc, sh, al, sc2, sh2, al2, rv[4];
      uint32_t voff[4];
      if constexpr (S::EARLY_REQ) {
        // into the registers the K loop's operands have left: the latency runs under the LDS round trip of M, not after it
        sc = load4_or(a.scale, c, 1.f), sh = load4_or(a.shift, c, 0.f), al = load4_or(a.alpha, c, 0.f);
        sc2 = load4_or(a.scale2, c, 1.f), sh2 = load4_or(a.shift2, c, 0.f), al2 = load4_or(a.alpha2, c, 0.f);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int pix = pix0 + (p >> 1) * a.W + (p & 1);
          if constexpr (S::ODD)                        // output p is input point (1 + p / 2, 1 + p % 2) of the tile: on the map or not
            voff[p] = ((vmask >> (5 + 4 * (p >> 1) + (p & 1))) & 1u) ? ((uint32_t)pix * (uint32_t)a.Cout + (uint32_t)c) * 4u : OOB;
          else
            voff[p] = tile_ok ? ((uint32_t)pix * (uint32_t)a.Cout + (uint32_t)c) * 4u : OOB;
          rv[p] = has_res ? buf_load4(res_rsrc, voff[p]) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_sched_barrier(0);           // (the requests stay above the LDS traffic)
      }
#pragma unroll
      for (int j = 0; j < CPW; ++j)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            wino_smem[(CPW * wave + j) * (TT * 32) + (mf * 32 + frag_row(lane, r)) * 32 + r32] = acc[j][mf][nf][r];
      lds_barrier();
      f32x4 m[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) m[k] = *reinterpret_cast<const f32x4*>(wino_smem + k * (TT * 32) + ltile * 32 + c4);
      f32x4 yv[4];                                  // outputs (0,0), (0,1), (1,0), (1,1) of the tile
      {
        f32x4 s0[4], s1[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          s0[jj] = m[jj] + m[4 + jj] + m[8 + jj];
          s1[jj] = m[4 + jj] - m[8 + jj] - m[12 + jj];
        }
        yv[0] = s0[0] + s0[1] + s0[2];
        yv[1] = s0[1] - s0[2] - s0[3];
        yv[2] = s1[0] + s1[1] + s1[2];
        yv[3] = s1[1] - s1[2] - s1[3];
      }
      if constexpr (!S::EARLY_REQ) {
        sc = load4_or(a.scale, c, 1.f), sh = load4_or(a.shift, c, 0.f), al = load4_or(a.alpha, c, 0.f);
        sc2 = load4_or(a.scale2, c, 1.f), sh2 = load4_or(a.shift2, c, 0.f), al2 = load4_or(a.alpha2, c, 0.f);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int pix = pix0 + (p >> 1) * a.W + (p & 1);
          if constexpr (S::ODD)                        // output p is input point (1 + p / 2, 1 + p % 2) of the tile: on the map or not
            voff[p] = ((vmask >> (5 + 4 * (p >> 1) + (p & 1))) & 1u) ? ((uint32_t)pix * (uint32_t)a.Cout + (uint32_t)c) * 4u : OOB;
          else
            voff[p] = tile_ok ? ((uint32_t)pix * (uint32_t)a.Cout + (uint32_t)c) * 4u : OOB;
          rv[p] = has_res ? buf_load4(res_rsrc, voff[p]) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f32x4 v, v2;
        epilogue4(yv[p], sc, sh, al, act, has_res, rv[p], sc2, sh2, al2, act2, v, v2);
        if constexpr (S::YSUB) {
          if (p == 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, tile_ok ? ((uint32_t)g * (uint32_t)a.Cout + (uint32_t)c) * 4u : OOB, 0, 0);
        } else {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, voff[p], 0, 0);
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v2), y2_rsrc, voff[p], 0, 0);
      }
      lds_barrier();
      ts[3 + nf] = wino_stamp<TRACE>();
    }
  }
  if constexpr (TRACE)
    if (tid == 0) wino_trace_write(a, tr_c0, ts);
}

// The layers the Winograd kernels take: 3x3 / stride 1 / pad 1 (no output shrink), whole 32-channel input slices, whole
// 64-channel column blocks, no pre-activation, the lean epilogue's plain geometry and unit-stride shortcut, 31-bit byte
// offsets.  On an even map with a whole first output it returns 1 for the narrow maps: at most 16 x 16 with at least wino::MIN_TILES Winograd tiles (level 1
// and up; launch_conv_wino runs them in 64-tile blocks at level 1 and in 32-tile blocks at level 2, the same bits); 2 for
// the wide maps (launch_conv_winow): up to 112 x 112 with the tiles of at least wino::WIDE_MIN_IMAGES images (level 2);
// 3 for the rest (launch_conv_winox; level 2, at least wino::WIDE_MIN_IMAGES images): a map from 3 x 3 to 16 x 16 with an odd
// side and at least wino::ODD_MIN_TILES tiles of the padded grid, or an even map up to 112 x 112 whose first output is
// sub-sampled (y_sub); 0 otherwise.  Depends on the shape, the batch of the launch, the level and whether the net carries the transformed
// weights (Net option "wino") -- on nothing else.
static int wino_applies(const ConvArgs& a) {
  if (!a.w_wino || a.wino_level < 1 || a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad_t != 1 || a.pad_l != 1) return 0;
  if (a.Ho != a.H || a.Wo != a.W) return 0;
  const bool odd = (a.H & 1) || (a.W & 1), rest = odd || a.y_sub;
  const bool wide = a.H > 16 || a.W > 16;
  if (rest && (a.wino_level < 2 || (odd && (a.y_sub || a.H > wino::ODD_MAX_HW || a.W > wino::ODD_MAX_HW || a.H < 3 || a.W < 3)))) return 0;
  if (wide && (a.wino_level < 2 || a.H > wino::WIDE_MAX_HW || a.W > wino::WIDE_MAX_HW)) return 0;
  if (a.Cin % 32 != 0 || a.Cout % wino::BN != 0 || a.pre_scale) return 0;
  if (!(a.y_H == a.Ho && a.y_W == a.Wo && a.y_oy == 0 && a.y_ox == 0 && a.y_ld == a.Cout && a.y_coff == 0)) return 0;
  if (a.res && (a.res_stride != 1 || a.res_H != a.Ho || a.res_W != a.Wo)) return 0;
  if ((int64_t)a.M * a.Cout * 4 >= 0x7fffffffLL || (int64_t)a.M * a.Cin * 4 >= 0x7fffffffLL) return 0;
  if ((int64_t)16 * a.Cin * a.Cout * 4 > (int64_t)a.w_wino_bytes) return 0;
  const int64_t tpi = (int64_t)((a.H + 1) / 2) * ((a.W + 1) / 2);
  if (rest) return a.N >= wino::WIDE_MIN_IMAGES && (!odd || a.N * tpi >= wino::ODD_MIN_TILES) ? 3 : 0;
  if (wide) return a.N * tpi >= wino::WIDE_MIN_IMAGES * tpi ? 2 : 0;
  return a.N * tpi >= wino::MIN_TILES ? 1 : 0;
}

template <class S>
static int launch_wino(const ConvArgs& a, hipStream_t st, const char* name) {
  const auto kern = a.trace ? conv_wino_kernel<S, true> : conv_wino_kernel<S, false>;
  if (allow_dynamic_lds(reinterpret_cast<const void*>(kern), S::LDS_BYTES)) return -1;
  // [dbg bit 67108864: the half-block shapes ask for 24 KiB of dynamic LDS they do not use, 88 KiB in all, so that one block
  // is resident per CU and every wave is alone on its SIMD -- with dbg 256 the stamps of a lone wave's K loop.  The limit
  // is raised per launch: allow_dynamic_lds remembers a kernel, not a size]
  int lds = S::LDS_BYTES;
  if (S::TT == 32 && (a.dbg & 67108864)) {
    lds += 24 * 1024;
    DIF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  const int64_t ntiles = S::ODD ? (int64_t)a.N * ((a.H + 1) / 2) * ((a.W + 1) / 2) : (int64_t)a.N * (a.H / 2) * (a.W / 2);
  const int blocks_m = (int)((ntiles + S::TT - 1) / S::TT), tiles_n = a.Cout / wino::BN;
  const int64_t nblocks = (int64_t)blocks_m * tiles_n;
  if (nblocks >= 0x7fffffffLL) return set_error("conv: too many tiles");
  hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(S::NT), lds, st, a, blocks_m, (int)nblocks);
  DIF_HIP(hipGetLastError());
  g_last_kernel = name;
  return 0;
}

// The reported names keep the map class in their beginning, whatever the shape: op_table()'s readers tell the narrow-map
// layers (level 1's list, conv_wino_kernel) from the wide ones (conv_winow_kernel) by it.
static int launch_conv_wino(const ConvArgs& a, hipStream_t st) {             // narrow maps (wino_applies: 1)
  if (a.wino_level >= 2 && !(a.dbg & 16777216)) return launch_wino<WinoW<32, 4, 2, true>>(a, st, "conv_wino_kernel<F(2x2,3x3),32 tiles x 64>");
  return launch_wino<WinoW<64, 2, 1, false>>(a, st, "conv_wino_kernel<F(2x2,3x3),64 tiles x 64>");
}

static int launch_conv_winow(const ConvArgs& a, hipStream_t st) {            // wide maps (wino_applies: 2)
  if (a.dbg & 65536) return launch_wino<WinoW<64, 2, 2, true>>(a, st, "conv_winow_kernel<F(2x2,3x3),64 tiles x 64>");
  return launch_wino<WinoW<32, 4, 2, true>>(a, st, "conv_winow_kernel<F(2x2,3x3),32 tiles x 64>");
}

// the rest (wino_applies: 3): names of their own, so that the readers of the two lists above see neither class grow
static int launch_conv_winox(const ConvArgs& a, hipStream_t st) {
  if (a.y_sub) return launch_wino<WinoX<false, true>>(a, st, "conv_winox_kernel<F(2x2,3x3),32 tiles x 64,ysub>");
  return launch_wino<WinoX<true, false>>(a, st, "conv_winox_kernel<F(2x2,3x3),32 tiles x 64,odd>");
}
