// gemm_wgrad_ws_kernel: the fp32 (PREC 0, split-product) weight-gradient GEMMs with the operand split done ONCE
// per block on dedicated waves: RC x RC, the Linear weight gradients (dW += dy^T x, bias gradient fused), and
// RC x I2C_RC (GB), the conv2 weight gradient dW2r = dz2^T im2col(z1) with B gathered from the NHWC conv1 map.
//
// The gathered B (GB, a compile-time parameter: the RC x RC instantiations are unchanged): a tile row is a column
// (kt, kf, c) of the im2col view and a k-row an output pixel, so a producer lane's 16-byte quad -- four channels
// of one tap, C % 4 == 0 -- sits at the same offset from every pixel's receptive-field origin.  That offset
// (i2c_col_off) goes into the lane's base pointer once per tile; each of the lane's four loads per slab decodes
// its own pixel's origin (i2c_pix_off24: two multiply-high divisions and 24-bit multiplies, no branch), the only
// VALU the gather adds.  One 256 x 128 tile covers all of M = D = 256, so every B slab is gathered once per column
// tile (the 128-row kernel fetched it once per row tile) and split once.  Everything after the load -- the plane
// image, the ring, the barrier schedule, the consumers -- is the RC x RC kernel's, so an unsplit launch gives the C of
// gemm_glds_kernel<RC, I2C_RC, ., ., EPI_PLAIN, 0> bit for bit.
//
// One 512-thread block per CU, tile BMT x 128, two roles:
//   producers (waves 4-7; VALU + memory only): fetch the A and B slabs (32 k-rows x tile rows) with 16-byte
//     global loads into registers one slab ahead, split every value once (split3_pair, the split of
//     split3_bf16) and write the three bf16 planes of both operands with ds_write_b64 into the RC plane
//     image of StageP<RC> / frag_pl_rc (k-row major, 16-byte chunks XOR-swizzled by bf16_rc_swz).  No fp32
//     lands in LDS.  The fused row sums of A (the bias gradient) are taken here from the fp32 values: a
//     producer wave owns BMT / 4 tile rows through every k, so a row's sum is one lane's fixed-order chain
//     plus a fixed-order cross-lane tail (no atomics).
//   consumers (waves 0-3, 2 x 2, one per SIMD, BMT / 2 x 64 each; no split VALU): fragments of both
//     operands by ds_read_b64_tr_b16 (frag_pl_rc), the six split products in mma6's order with its
//     k-grouping (k-step hs of half h: k = 16h + 8hs + 0..7), so every accumulator sees the MFMAs
//     gemm_glds_kernel<RC, RC, ., ., EPI_PLAIN, 0> issues, in its order: C is the same bit for bit.
//
// Ring and synchronisation: two plane stages (3 * (BMT + 128) * 64 bytes each).  In iteration s the
// consumers read stage s % 2 while the producers write slab s + 1 into the other stage and then fetch
// slab s + 2 into registers; ONE raw s_barrier per slab closes the iteration for both roles.  The schedule
// (run()) is written once, with the role as a compile-time parameter inside it: a prologue barrier, then per
// tile c.nk calls of slab(), whose last statement is the slab's barrier for either role.  The tile / slab
// sequence is computed from wave-uniform launch values alone, so every wave executes 1 + sum over the
// block's tiles of nk barriers: the K tail, a split's short last chunk and
// the hand-over to the block's next tile (whose first slab the producers write during the current tile's
// last slab) are iterations of the same loop.  A stage is rewritten only after
// the barrier that follows the consumers' lgkmcnt(0) on their reads of it; the producers' plane writes
// are retired (lgkmcnt(0)) before the barrier that publishes them.
// Epilogue: the EPI_PLAIN stores of gemm_glds_kernel (split-K partials / alpha, beta R), by the consumers.
#include "gemm_kernels.h"

namespace espg {

#if ESP_WGRAD_WS && ESP_F32_SPLIT

namespace {

constexpr int WS_BN = 128, WS_NT = 512;

// a producer wave's share of one operand slab (ROWS tile rows x 32 k): the wave owns the ROWS / 16 row quads
// [LQ pw, LQ pw + LQ) at every k-row; lane = (k-row krl = lane / LQ, quad lane % LQ); load i covers k-rows
// KP i + krl.  KP % 4 == 0, so a lane's chunk swizzle (a function of k-row % 4) is the same for every i.
template <int ROWS>
struct WsStage {
  static constexpr int LQ = ROWS / 16, KP = 64 / LQ, NI = GL_BK / KP;
  static constexpr int ROWB = ROWS * 2, PLB = ROWB * GL_BK;  // bytes: one k-row, one plane image
  const float* p;  // the lane's quad in k-row 0 of the operand (row clamped to the last whole quad)
  int krl;
  uint32_t lds;    // byte offset of the lane's 8 bytes in k-row krl of a plane image
  __device__ __forceinline__ void init_lane(int pw, int lane) {
    const int c = LQ * pw + (lane % LQ);
    krl = lane / LQ;
    lds = (uint32_t)(krl * ROWB + (((c >> 1) ^ bf16_rc_swz(ROWB, krl)) << 4) + 8 * (c & 1));
  }
  __device__ __forceinline__ void init_tile(const float* base, int rows, int row0, int pw, int lane) {
    const int c = LQ * pw + (lane % LQ);
    p = base + min(row0 + 4 * c, rows - 4);  // rows % 4 == 0, rows >= 4 (host)
  }
  // the gathered form (I2C_RC: a tile row is a column (kt, kf, c) of the im2col view of an NHWC map, a k-row an
  // output pixel): the quad's column offset from the receptive-field origin is the same at every k-row (C % 4 == 0
  // keeps a quad inside one tap), so it is folded into p once per tile
  __device__ __forceinline__ void init_tile_i2c(const Operand& op, const FastDiv& fc, int rows, int row0, int pw,
                                                int lane) {
    const int c = LQ * pw + (lane % LQ);
    p = op.p + i2c_col_off(op.ic, fc, min(row0 + 4 * c, rows - 4));
  }
  // load i of the slab at k0; k-rows past K read the last one (finite in-range values, as the LDS-DMA staging
  // clamps them)
  __device__ __forceinline__ float4 load(long ld, int K, int k0, int i) const {
    const int k = min(k0 + KP * i + krl, K - 1);
    return *reinterpret_cast<const float4*>(p + (long)k * ld);
  }
  // ... gathered: the pixel's receptive-field origin, decoded per load on 24-bit multiplies (host: Bn H W < 2^24,
  // the map < 2^32 elements) and added as an unsigned 32-bit element offset to the 64-bit pointer
  __device__ __forceinline__ float4 load_i2c(const Operand& op, const FastDiv& fhw, const FastDiv& fwo, int K, int k0,
                                             int i) const {
    const uint32_t k = (uint32_t)min(k0 + KP * i + krl, K - 1);
    return *reinterpret_cast<const float4*>(p + i2c_pix_off24(op.ic, fhw, fwo, k));
  }
  // split load i's values and write the planes; ZERO (operand A): k-rows >= kv are written as zeros; RS: rs += the
  // values
  template <bool ZERO, bool RS>
  __device__ __forceinline__ void store(float4 w, int i, char* planes, int kv, bool do_rs, float (&rs)[4]) const {
    if (ZERO && KP * i + krl >= kv) w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (RS && do_rs) {
      rs[0] += w.x;
      rs[1] += w.y;
      rs[2] += w.z;
      rs[3] += w.w;
    }
    uint32_t h0, m0, l0, h1, m1, l1;
    // (the v_sub form: a pair here is two ROWS at one k, and the dot form's residual of a finite element is NaN
    // beside a non-finite partner -- the neighbour row of an inf / NaN would turn non-finite too)
    esp::split3_pair<false>(w.x, w.y, h0, m0, l0);
    esp::split3_pair<false>(w.z, w.w, h1, m1, l1);
    char* d = planes + lds + i * KP * ROWB;
    *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(d + PLB) = make_uint2(m0, m1);
    *reinterpret_cast<uint2*>(d + 2 * PLB) = make_uint2(l0, l1);
  }
};

// GB: B gathered from an NHWC map (I2C_RC) instead of read as a row-major [K][N] matrix (RC)
template <int BMT, bool RS, bool GB>
__global__ __launch_bounds__(WS_NT, 1) void gemm_wgrad_ws_kernel(GemmArgs g, GldsArgs x) {
  static_assert(BMT == 256 || BMT == 128, "tile height");
  constexpr int TM = BMT / 64, TN = 2;                // a consumer wave: BMT / 2 x 64
  constexpr int PLA = BMT * 64, PLBN = WS_BN * 64;    // bytes of one A / B plane image
  constexpr int STB = 3 * (PLA + PLBN);               // bytes of one stage
  static_assert(2 * STB <= 163840, "LDS");
  __shared__ __attribute__((aligned(16))) float smem[2 * STB / 4];
  char* const sm = reinterpret_cast<char*>(smem);

  const int G = gridDim.x;
  int t = blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool producer = wave >= 4;
  const int pw = wave & 3;               // producer: its row share; consumer: (wm, wn)
  const int wm = pw >> 1, wn = pw & 1;

  TileCoord c = tile_coord<WS_BN, BMT>(g, x, t, G);

  // ---- producer state: the slab held in registers (fetched, not yet written) and the next one to fetch
  WsStage<BMT> sa;
  WsStage<WS_BN> sb;
  constexpr int NIA = WsStage<BMT>::NI, NIB = WsStage<WS_BN>::NI;
  float4 va[NIA], vb[NIB];
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
  bool held = false, held_rs = false;    // registers hold a slab; its tile takes the row sums
  int held_kv = GL_BK;                   // its valid k-rows
  int lt = t, lkt = 0;                   // fetch cursor: tile, slab
  TileCoord lc = c;
  bool lok = true;
  auto fetch = [&]() {  // registers <- slab (lc, lkt); advance the cursor
    held = lok;
    if (!lok) return;
    if (lkt == 0) {
      sa.init_tile(g.a.p, g.M, lc.m0, pw, lane);
      if constexpr (GB) sb.init_tile_i2c(g.b, x.c_b, g.N, lc.n0, pw, lane);
      else sb.init_tile(g.b.p, g.N, lc.n0, pw, lane);
    }
    const int k0 = lc.kbeg + lkt * GL_BK;
#pragma unroll
    for (int i = 0; i < NIA; ++i) va[i] = sa.load(g.a.ld, g.K, k0, i);
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      if constexpr (GB) vb[i] = sb.load_i2c(g.b, x.hw_b, x.wo_b, g.K, k0, i);
      else vb[i] = sb.load(g.b.ld, g.K, k0, i);
    }
    held_kv = lc.kend - k0;
    held_rs = RS && lc.tn == 0;
    if (++lkt == lc.nk) {
      lt += G;
      lkt = 0;
      lok = lt < x.ntiles;
      if (lok) lc = tile_coord<WS_BN, BMT>(g, x, lt, G);
    }
  };
  auto put = [&](int stage) {  // planes of the held slab -> stage
    char* st = sm + stage * STB;
    float none[4];
#pragma unroll
    for (int i = 0; i < NIA; ++i) sa.template store<true, RS>(va[i], i, st, held_kv, held_rs, rs);
#pragma unroll
    for (int i = 0; i < NIB; ++i) sb.template store<false, false>(vb[i], i, st + 3 * PLA, GL_BK, false, none);
  };
  // the row sums of tile cc's rows (this wave's BMT / 4 of them), in fixed order
  auto flush_rs = [&](const TileCoord& cc) {
    if constexpr (RS) {
      if (cc.tn != 0) return;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = rs[e];
#pragma unroll
        for (int o = WsStage<BMT>::LQ; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
        rs[e] = 0.f;
        const int m = cc.m0 + 4 * (WsStage<BMT>::LQ * pw + lane) + e;
        if (lane < WsStage<BMT>::LQ && m < g.M) {
          if (g.splits > 1) g.rs_work[(long)cc.split * g.M + m] = v;
          else g.rowsum[m] += v;
        }
      }
    }
  };

  int buf = 0;

  // One iteration per slab for both roles: the role's work, then ONE raw s_barrier.
  f32x16 acc[TM][TN];  // consumers only
  auto slab = [&](auto role, const TileCoord& cc, int kt) {
    if constexpr (decltype(role)::value) {  // producer
      // the slab after this one (the last iteration of a tile: the next tile's first) -> the other stage
      if (kt + 1 == cc.nk) flush_rs(cc);  // every slab of this tile has been written
      if (held) put(buf ^ 1);
      fetch();
      wait_lgkm0();  // the plane writes are in LDS before the barrier publishes them
    } else {
      const char* st = sm + buf * STB;
      constexpr int PA[6] = {1, 2, 0, 1, 0, 0}, PB[6] = {1, 0, 2, 0, 1, 0};  // mma6's products and order
      // fragments one 32-row group ahead of the MFMAs that use them (the scheduling barriers keep the
      // compiler from hoisting a whole slab's reads), so each group's MFMAs wait with a counted lgkmcnt for
      // their own reads only: 6 transposed reads per 12 MFMAs, B's 12 of the second k-step beside the first
      // k-step's last group
      auto load_b = [&](int hs, bf16x8 (&bh)[TN][3]) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int p = 0; p < 3; ++p)
            bh[j][p] = frag_pl_rc<WS_BN>(reinterpret_cast<const float*>(st + 3 * PLA + p * PLBN), wn * 64 + j * 32,
                                         lane, hs);
      };
      auto load_a = [&](int i, int hs, bf16x8 (&ah)[3]) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
          ah[p] = frag_pl_rc<BMT>(reinterpret_cast<const float*>(st + p * PLA), wm * TM * 32 + i * 32, lane, hs);
      };
      bf16x8 bh[2][TN][3], ah[2][3];
      load_b(0, bh[0]);
      load_a(0, 0, ah[0]);
#pragma unroll
      for (int u = 0; u < 2 * TM; ++u) {  // u = hs * TM + i
        const int hs = u / TM, i = u % TM;
        if (u + 1 < 2 * TM) {
          if (i + 1 == TM) load_b(1, bh[1]);
          load_a((u + 1) % TM, (u + 1) / TM, ah[(u + 1) & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int p = 0; p < 6; ++p)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[u & 1][PA[p]], bh[hs][j][PB[p]], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      wait_lgkm0();  // this wave's reads of the stage are retired before the barrier frees it
    }
    raw_barrier();  // both roles, once per slab
    buf ^= 1;
  };

  // The whole schedule, written once and instantiated per role (left as a run-time branch inside the loops, the
  // wave-uniform role keeps both roles' registers live in every wave: the accumulators are then held twice
  // and moved at both ends of every iteration, and the producers' slab registers sit beside them).  Either
  // instantiation executes the prologue barrier and then slab() -- whose last statement is the slab's barrier
  // for either role -- c.nk times per tile, over the same wave-uniform tile sequence.
  auto run = [&](auto role) {
    constexpr bool P = decltype(role)::value;
    if constexpr (P) {
      sa.init_lane(pw, lane);
      sb.init_lane(pw, lane);
      fetch();
      put(0);
      fetch();
      wait_lgkm0();
    }
    raw_barrier();
    for (;;) {
      const int tnext = t + G;
      const bool has_next = tnext < x.ntiles;
      if constexpr (!P) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
      }
      for (int kt = 0; kt < c.nk; ++kt) slab(role, c, kt);
      if constexpr (!P) {
        // gemm_glds_kernel's EPI_PLAIN epilogue (g.wide: host)
        const int mr0 = c.m0 + wm * TM * 32, nc0 = c.n0 + wn * TN * 32;
        float* W = g.splits > 1 ? g.work + ((long)c.split * g.batch + c.z) * (long)g.M * g.N : nullptr;
        if (W && mr0 + TM * 32 <= g.M && nc0 + TN * 32 <= g.N)
          store_cols<EPI_P0, TM, TN, true>(g, 0, g.N, mr0, nc0, lane, acc, W);
        else if (W) store_partials_wide<TM, TN>(g, W, mr0, nc0, lane, acc);
        else store_tiles_wide<EPI_PLAIN, TM, TN>(g, c.z, mr0, nc0, lane, acc, false);
      }
      if (!has_next) break;
      t = tnext;
      c = tile_coord<WS_BN, BMT>(g, x, t, G);
    }
  };
  if (producer) run(std::true_type{});
  else run(std::false_type{});
}

}  // namespace

bool wgrad_ws_launch(bool gather_b, bool rs, dim3 grid, hipStream_t st, const GemmArgs& g, const GldsArgs& x) {
  if (g.bm != WGRAD_WS_BM || g.bnt != WS_BN) return false;
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(WS_NT), 0, st, g, x); };
  if (gather_b) {
    if (rs) go(gemm_wgrad_ws_kernel<WGRAD_WS_BM, true, true>);
    else go(gemm_wgrad_ws_kernel<WGRAD_WS_BM, false, true>);
  } else {
    if (rs) go(gemm_wgrad_ws_kernel<WGRAD_WS_BM, true, false>);
    else go(gemm_wgrad_ws_kernel<WGRAD_WS_BM, false, false>);
  }
  return true;
}

#else

bool wgrad_ws_launch(bool, bool, dim3, hipStream_t, const GemmArgs&, const GldsArgs&) { return false; }

#endif

}  // namespace espg
