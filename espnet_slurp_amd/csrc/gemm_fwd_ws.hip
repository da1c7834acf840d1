// gemm_fwd_ws_kernel: the long-K forward GEMMs on B planes (PREC 3: fp32 A, the weight B as its three bf16 split
// planes in HBM) with A gathered and split ONCE per block on dedicated waves: KC x KC, the Linear forward with the
// bias + dropout + residual epilogue (EPI_BDR: FFN w_2) or bias + ReLU (EPI_BRELU), and I2C_KC x KC (GA), the conv2
// forward with A the im2col view of the NHWC conv1 map (EPI_BRELU).
//
// gemm_glds_kernel<., KC, 128, ., ., 3> stages A as fp32 and splits it in registers on the MFMA waves: every A value
// is split by both waves that share its tile row, and again in every 128-wide column tile, and the conv2 gather is
// repeated per column tile.  Here one 128 x 256 tile covers N = 256, so every A value is fetched and split once.
//
// One 512-thread block per CU, two roles (the structure of gemm_wgrad_ws_kernel):
//   producers (waves 4-7; VALU + memory only): a lane fetches 16-byte quads along k of A (KC: row-major; GA: the 32
//     channels of one tap of the row's pixel, contiguous in the map; the pixel's receptive-field origin is decoded
//     per load by i2c_pix_off24, no carried state and no branch) into registers one slab ahead, splits every value
//     once (split3_pair's v_sub form: a non-finite value leaves its pair partner's parts finite) and writes the three
//     planes with ds_write_b64 into the KC plane image frag_pl_kc reads (StageP<KC>'s: row r's 16-byte chunk c at
//     position c ^ pl_kc_swz(r)).  No fp32 lands in LDS.  B's planes go from HBM to the same image by LDS-DMA
//     (StageP<KC, 256>).  vmcnt retires in order: a slab's DMA is issued BEFORE the next slab's register loads, and
//     the wait before the barrier that publishes the stage is counted so that it covers the DMA alone.
//   consumers (waves 0-3, 2 x 2, one per SIMD, 64 x 128 each: TM = 2, TN = 4; no split VALU): fragments of both
//     operands by ds_read_b128 (frag_pl_kc), the six split products in mma6's order with its k-grouping (k-step hs
//     of half h: k = 16h + 8hs + 0..7), so every accumulator sees the MFMAs gemm_glds_kernel<., KC, ., ., ., 3>
//     issues, in its order: C is the same bit for bit.  A k-step's A fragments (both 32-row groups) stay in
//     registers while B's four 32-column fragments pass by, each read one group ahead of its 12 MFMAs.
//
// Ring and synchronisation: two plane stages of 72 KB (A 3 x 8 KB, B 3 x 16 KB).  In iteration s the consumers read
// stage s % 2 while the producers fill the other stage with slab s + 1 and then fetch slab s + 2's A into
// registers; ONE raw s_barrier per slab closes the iteration for both roles.  The schedule (run()) is written once
// with the role as a compile-time parameter; the tile / slab sequence is computed from wave-uniform launch values
// alone, so every wave executes 1 + sum over the block's tiles of nk barriers, and the hand-over to the block's next
// tile (whose first slab the producers stage during the current tile's last slab) is an iteration of the same loop.
// A stage is rewritten only after the barrier that follows the consumers' lgkmcnt(0) on their reads of it.
// Bounds: rows past M / N read clamped in-range rows and their outputs are discarded; A's K tail (KC: K % 8 == 0,
// whole quads) is written as zeros, B's reads clamped chunks (finite values).
// Epilogue: store_spec (EPI_BRELU / EPI_BDR) at TM = 2, TN = 4, by the consumers.
// Not here: split-K, row sums, batches, the bf16 modes (the host keeps such launches on gemm_glds_kernel).
#include "gemm_kernels.h"

namespace espg {

#if ESP_FWD_WS && ESP_F32_SPLIT

namespace {

constexpr int FW_NT = 512;
constexpr int FW_PLB = FWD_WS_BN * 64;                           // bytes of one B plane image (A: FW_PLA)
constexpr int FW_STB = 3 * (FW_PLA + FW_PLB);                    // bytes of one stage

// (a producer lane's share of an A slab: FwStageA, gemm_kernels.h)

// GA: A gathered from an NHWC map (I2C_KC) instead of read as a row-major [M][K] matrix (KC)
template <bool GA, int EPI>
__global__ __launch_bounds__(FW_NT, 1) void gemm_fwd_ws_kernel(GemmArgs g, GldsArgs x) {
  constexpr int TM = 2, TN = 4;  // a consumer wave: 64 x 128
  static_assert(2 * FW_STB <= 163840, "LDS");
  __shared__ __attribute__((aligned(16))) float smem[2 * FW_STB / 4];
  char* const sm = reinterpret_cast<char*>(smem);

  const int G = gridDim.x;
  int t = blockIdx.x;
  if (t >= x.ntiles) return;  // block-uniform
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool producer = wave >= 4;
  const int pw = wave & 3;  // producer: its row share; consumer: (wm, wn)
  const int wm = pw >> 1, wn = pw & 1;
  const int h = lane >> 5, l32 = lane & 31;

  TileCoord c = tile_coord<FWD_WS_BN, FWD_WS_BM>(g, x, t, G);

  // ---- producer state: the A slab held in registers (fetched, not yet staged) and the next one to fetch
  FwStageA<GA> sa;
  StageP<KC, FWD_WS_BN, 4> sb;
  constexpr int NIA = FwStageA<GA>::NI;
  float4 va[NIA];
  bool held = false, held_first = false;  // registers hold a slab; it is its tile's first
  int held_kv = GL_BK, held_k0 = 0, held_n0 = 0;
  int lt = t, lkt = 0;                    // fetch cursor: tile, slab
  TileCoord lc = c;
  bool lok = true;
  const uint32_t smem_lds = lds_addr(smem);
  auto fetch = [&]() {  // registers <- A of slab (lc, lkt); advance the cursor
    held = lok;
    if (!lok) return;
    const int k0 = lkt * GL_BK;
    const long tap = GA ? sa.tap_off(g, x, k0) : 0;
#pragma unroll
    for (int i = 0; i < NIA; ++i) va[i] = sa.load(g, x, lc.m0, k0, tap, i);
    held_kv = g.K - k0;
    held_k0 = k0;
    held_n0 = lc.n0;
    held_first = lkt == 0;
    if (++lkt == lc.nk) {
      lt += G;
      lkt = 0;
      lok = lt < x.ntiles;
      if (lok) lc = tile_coord<FWD_WS_BN, FWD_WS_BM>(g, x, lt, G);
    }
  };
  auto put = [&](int stage) {  // the held slab -> stage: B's planes by LDS-DMA (issued first), A's planes split here
    // (the wait for the held registers sits at their first use below, behind the DMA's issue, so it also covers the
    // DMA; taking it before the DMA instead, so that the split runs under the DMA's latency, measured 2 % slower per
    // shape: the producers are not the slab's critical path)
    if (held_first) sb.init(g.b, g.b.p, g.N, held_n0, 0, pw, lane);
    sb.issue(g.K, held_k0, smem_lds + (uint32_t)(stage * FW_STB + 3 * FW_PLA), pw);
    char* st = sm + stage * FW_STB;
#pragma unroll
    for (int i = 0; i < NIA; ++i) sa.store(va[i], i, st, held_kv);
  };
  // before the barrier that publishes a stage: its DMA has landed (every later vector-memory operation of this wave
  // is one of fetch()'s NIA register loads) and the plane writes are in LDS
  auto publish = [&]() {
    if (held) wait_vm_n<NIA>();
    else wait_vm0();
    wait_lgkm0();
  };

  int buf = 0;

  // One iteration per slab for both roles: the role's work, then ONE raw s_barrier.
  f32x16 acc[TM][TN];  // consumers only
  auto slab = [&](auto role) {
    if constexpr (decltype(role)::value) {  // producer
      // the slab after this one (the last iteration of a tile: the next tile's first) -> the other stage
      if (held) put(buf ^ 1);
      fetch();
      publish();
    } else {
      const char* st = sm + buf * FW_STB;
      constexpr int PA[6] = {1, 2, 0, 1, 0, 0}, PB[6] = {1, 0, 2, 0, 1, 0};  // mma6's products and order
      // unit u = (k-step hs, column group j): 12 MFMAs (both row groups x six products) on B fragment j, which is
      // read one unit ahead; the next k-step's A fragments are read beside the last unit of the current one (the
      // scheduling barriers keep the compiler from hoisting a whole slab's reads), so each unit's MFMAs wait with a
      // counted lgkmcnt for their own reads only
      auto load_b = [&](int j, int hs, bf16x8 (&bh)[3]) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
          bh[p] = frag_pl_kc(reinterpret_cast<const float*>(st + 3 * FW_PLA + p * FW_PLB), wn * TN * 32 + j * 32 + l32, h,
                             hs);
      };
      auto load_a = [&](int hs, bf16x8 (&ah)[TM][3]) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int p = 0; p < 3; ++p)
            ah[i][p] = frag_pl_kc(reinterpret_cast<const float*>(st + p * FW_PLA), wm * TM * 32 + i * 32 + l32, h, hs);
      };
      bf16x8 ah[2][TM][3], bh[2][3];
      load_a(0, ah[0]);
      load_b(0, 0, bh[0]);
#pragma unroll
      for (int u = 0; u < 2 * TN; ++u) {  // u = hs * TN + j
        const int hs = u / TN, j = u % TN;
        if (u + 1 < 2 * TN) {
          load_b((u + 1) % TN, (u + 1) / TN, bh[(u + 1) & 1]);
          if (j + 1 == TN) load_a(1, ah[1]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int p = 0; p < 6; ++p)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[hs][i][PA[p]], bh[u & 1][PB[p]], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      wait_lgkm0();  // this wave's reads of the stage are retired before the barrier frees it
    }
    raw_barrier();  // both roles, once per slab
    buf ^= 1;
  };

  // The whole schedule, written once and instantiated per role (a run-time role branch inside the loops keeps both
  // roles' registers live in every wave: gemm_wgrad_ws.hip).  Either instantiation executes the prologue barrier
  // and then slab() -- whose last statement is the slab's barrier for either role -- c.nk times per tile, over the
  // same wave-uniform tile sequence.
  auto run = [&](auto role) {
    constexpr bool P = decltype(role)::value;
    if constexpr (P) {
      sa.init_lane(pw, lane);
      fetch();
      put(0);
      fetch();
      publish();
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
      for (int kt = 0; kt < c.nk; ++kt) slab(role);
      if constexpr (!P) store_spec_tiles<EPI, TM, TN>(g, 0, c.m0 + wm * TM * 32, c.n0 + wn * TN * 32, lane, acc);
      if (!has_next) break;
      t = tnext;
      c = tile_coord<FWD_WS_BN, FWD_WS_BM>(g, x, t, G);
    }
  };
  if (producer) run(std::true_type{});
  else run(std::false_type{});
}

}  // namespace

bool fwd_ws_launch(bool gather_a, int epi, dim3 grid, hipStream_t st, const GemmArgs& g, const GldsArgs& x) {
  if (g.bm != FWD_WS_BM || g.bnt != FWD_WS_BN) return false;
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(FW_NT), 0, st, g, x); };
  if (gather_a && epi == EPI_BRELU) go(gemm_fwd_ws_kernel<true, EPI_BRELU>);
  else if (!gather_a && epi == EPI_BRELU) go(gemm_fwd_ws_kernel<false, EPI_BRELU>);
  else if (!gather_a && epi == EPI_BDR) go(gemm_fwd_ws_kernel<false, EPI_BDR>);
  else return false;
  return true;
}

#else

bool fwd_ws_launch(bool, int, dim3, hipStream_t, const GemmArgs&, const GldsArgs&) { return false; }

#endif

}  // namespace espg
