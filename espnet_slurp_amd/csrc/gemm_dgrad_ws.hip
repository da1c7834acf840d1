// gemm_dgrad_ws_kernel: the conv2 input gradient's parity-class GEMMs (I2CT_KC x RC in PREC 3: A the fp32 dz2
// gathered through the transposed-conv tap map, B the class weights as their three bf16 split planes in HBM) with A
// gathered and split ONCE per block on dedicated waves.
//
// gemm_glds_kernel<I2CT_KC, RC, 128, ., ., 3> stages dz2 as fp32 by LDS-DMA and splits it in registers on the MFMA
// waves: EPI_C1FOLD pins it to 128 x 128 tiles, so at N = 256 every dz2 value is gathered (address decode included)
// for two column tiles and split by both waves that share its tile row.  Here one 128 x 256 tile covers N = 256.
//
// The structure is gemm_fwd_ws_kernel's (gemm_fwd_ws.hip: the ring, the barrier schedule and run() / slab() with a
// compile-time role are its): one 512-thread block per CU,
//   producers (waves 4-7): A in FwStageA's lane layout (8 lanes cover the 32 channels of one tap of a row's source
//     pixel, 4 loads per slab, held one slab ahead in registers).  A slab lies inside one tap (C % 32 == 0), so the
//     tap's (dt, df) is wave-uniform; the class-grid row (b, a, e) is decoded per load (no carried state) and the
//     source pixel is (a - dt, e - df) of the T2 x F2 grid.  Outside the grid the address is clamped into the map
//     and the value selected to 0 before the split -- no branch, no out-of-bounds read, and the same exact 0 the
//     LDS-DMA kernel reads from its zero page.  Split once (split3_pair's v_sub form) into the KC plane image
//     (FwStageA::store).  B's RC planes (ld = N) go from HBM to LDS by LDS-DMA (StageP<RC, 256>), issued before the
//     next slab's register loads; the wait before the publishing barrier counts those loads.
//   consumers (waves 0-3, 2 x 2, 64 x 128 each: TM = 2, TN = 4): A fragments by frag_pl_kc, B fragments by
//     frag_pl_rc<256>, the six split products in mma6's order with its k-grouping, B read one unit ahead: every
//     accumulator sees the MFMA sequence of gemm_glds_kernel<I2CT_KC, RC, 128, false, ., 3, 128>, so the masked dz1
//     is the same bit for bit.
// Epilogues, by the consumers:
//   EPI_RMASKMAP  dz1 through the class row map (store_spec_tiles, the LDS-DMA kernel's own store)
//   EPI_C1FOLD    store_c1fold's sums at TN = 4 (dg_fold), with the rows' operands staged by the PRODUCERS: one
//     block per CU leaves a consumer's epilogue uncovered by other waves' MFMAs, and store_c1fold's per-row decode and
//     its 9 patch loads + mask word per row and sub-tile (L2 round trips, 32 in sequence per tile) were that
//     epilogue's time.  In a tile's second slab iteration two producer lanes per tile row decode the row once, load
//     its 3 x 3 conv1-input patch and its 8 mask words (loads older than the iteration's DMA, their latency under the
//     split of A) and write them to a 10 KB LDS buffer (the consumers' reads of the previous tile's rows ended
//     before the first iteration's barrier).  The consumers' epilogue reads LDS only.
//     The 5 * TN sums stay in registers across the block's tiles of one column tile (a read-modify-write of the
//     records per tile instead measured 0.85 ms per C2 B=384 call slower) and land in the LDS-DMA kernel's
//     record layout ([block][tn C1NT][wave 4][lane 64][10], 128 columns per tn): consumer wave (wm, wn) of column
//     tile tx owns tn = 2 tx + wn, and its sub-tile j fills wave slot 2 wm + (j >> 1), sums 5 (j & 1) + u -- the
//     128-column tile's wave (wm, j >> 1), sub-tile j & 1 -- so c1fold_reduce / c1fold_finalize read it unchanged.
// Bounds: rows past M read a clamped in-range row and are discarded by the epilogues; K = taps * C is whole slabs;
// N % 256 == 0 (host).  Decode limits (host): M, B * T2 * F2 < 2^24 (24-bit multiplies), dz2 < 2^32 elements.
// Not here: the bf16 dz2 path, split-K, row sums (the host keeps such launches on gemm_glds_kernel).
#include "gemm_kernels.h"

namespace espg {

#if ESP_DGRAD_WS && ESP_F32_SPLIT

namespace {

constexpr int DW_NT = 512;
constexpr int DW_BM = FWD_WS_BM, DW_BN = FWD_WS_BN;
constexpr int DW_PLB = DW_BN * 64;                // bytes of one B plane image (A: FW_PLA)
constexpr int DW_STB = 3 * (FW_PLA + DW_PLB);     // bytes of one stage
static_assert(2 * DW_BN / 128 <= C1NT, "EPI_C1FOLD records: 128 columns each");

constexpr int DW_FOLD_PT = 12;                                 // floats per row of the patch image (9 taps, padded)
constexpr int DW_FOLD_FLOATS = DW_BM * DW_FOLD_PT + DW_BM * 8;  // + 8 mask words per row (256 columns)

// EPI_C1FOLD at TN = 4 from the LDS images of the tile's rows (patch: [row][DW_FOLD_PT], mask: [row][8 words]):
// store_c1fold's sums in its order -- per 32-column sub-tile j the lane's 8 rows x 4 columns x (9 taps + 1), then
// c1fold_scatter over the 8 lanes sharing the columns -- added into k[5 j ..]; rloc0: the wave's first tile row
template <int TM, int TN>
__device__ __forceinline__ void dg_fold(const GemmArgs& g, int mrow0, int rloc0, int wn, int lane, f32x16 (&acc)[TM][TN],
                                        const float* patch, const uint32_t* mask, float (&k)[5 * TN]) {
  const int h = lane >> 5, l32 = lane & 31;
  const int sh = 4 * (l32 >> 2);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    float a[40];
#pragma unroll
    for (int v = 0; v < 40; ++v) a[v] = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      quad_transpose(acc[i][j], lane);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = i * 32 + 8 * q + 4 * h + (l32 & 3);
        if (mrow0 + r >= g.M) continue;
        const uint32_t w = mask[(rloc0 + r) * 8 + wn * TN + j] >> sh;
        const float* xp = patch + (rloc0 + r) * DW_FOLD_PT;
        const float4 p0 = *reinterpret_cast<const float4*>(xp), p1 = *reinterpret_cast<const float4*>(xp + 4);
        const float pt[9] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, xp[8]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = (w >> e) & 1u ? acc[i][j][4 * q + e] : 0.f;
#pragma unroll
          for (int t = 0; t < 9; ++t) a[e * 10 + t] = fmaf(d, pt[t], a[e * 10 + t]);
          a[e * 10 + 9] += d;
        }
      }
    }
    c1fold_scatter(a, lane, &k[5 * j]);
  }
}

// the tap of a slab: wave-uniform (k0 % 32 == 0, C % 32 == 0)
struct DgTap {
  int dt, df, o0;
};
__device__ __forceinline__ DgTap dg_tap(const GldsArgs& x, int k0) {
  const int t = (int)fdiv((uint32_t)k0, x.c_a);
  return DgTap{x.t_dt[t], x.t_df[t], k0 - t * x.t_C};
}
// load i of a slab of tap tp of the tile at row m0: the lane's quad of channels of the row's source pixel, clamped
// into the T2 x F2 grid; in: the pixel is inside it (else the caller writes zeros)
__device__ __forceinline__ float4 dg_load(const GemmArgs& g, const GldsArgs& x, const FwStageA<false>& sa, int m0,
                                          const DgTap& tp, int i, bool& in) {
  const uint32_t m = (uint32_t)min(m0 + sa.rl + 32 * i, g.M - 1);
  const uint32_t bb = fdiv(m, x.t_hw);
  const uint32_t rem = m - __umul24(bb, x.t_hw.d);
  const uint32_t aa = fdiv(rem, x.t_w);
  const int a = (int)aa - tp.dt, e = (int)(rem - __umul24(aa, x.t_w.d)) - tp.df;
  in = (uint32_t)a < (uint32_t)x.t_T2 && (uint32_t)e < (uint32_t)x.t_F2;
  const uint32_t ac = (uint32_t)min(max(a, 0), x.t_T2 - 1), ec = (uint32_t)min(max(e, 0), x.t_F2 - 1);
  const uint32_t off = __umul24(__umul24(__umul24(bb, (uint32_t)x.t_T2) + ac, (uint32_t)x.t_F2) + ec, (uint32_t)x.t_C);
  return *reinterpret_cast<const float4*>(g.a.p + tp.o0 + sa.kq + off);
}

template <int EPI>
__global__ __launch_bounds__(DW_NT, 1) void gemm_dgrad_ws_kernel(GemmArgs g, GldsArgs x) {
  static_assert(EPI == EPI_RMASKMAP || EPI == EPI_C1FOLD, "the conv2 input gradient's epilogues");
  constexpr int TM = 2, TN = 4;  // a consumer wave: 64 x 128
  static_assert(2 * DW_STB + 4 * (EPI == EPI_C1FOLD ? DW_FOLD_FLOATS : 0) <= 163840, "LDS");
  __shared__ __attribute__((aligned(16))) float smem[2 * DW_STB / 4 + (EPI == EPI_C1FOLD ? DW_FOLD_FLOATS : 0)];
  float* const fold_pt = smem + 2 * DW_STB / 4;  // EPI_C1FOLD: the tile's rows' patches and mask words
  uint32_t* const fold_mk = reinterpret_cast<uint32_t*>(fold_pt + DW_BM * DW_FOLD_PT);
  char* const sm = reinterpret_cast<char*>(smem);

  const int G = gridDim.x;
  int t = blockIdx.x;
  if (t >= x.ntiles) {  // block-uniform
    if constexpr (EPI == EPI_C1FOLD) {  // a block without tiles: zero records (c1fold_reduce reads every block's)
      float* dst = g.c1_part + (long)blockIdx.x * C1NT * 2560;
      for (int e = threadIdx.x; e < 2 * x.ntx * 2560; e += DW_NT) dst[e] = 0.f;
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool producer = wave >= 4;
  const int pw = wave & 3;  // producer: its row share; consumer: (wm, wn)
  const int wm = pw >> 1, wn = pw & 1;
  const int h = lane >> 5, l32 = lane & 31;

  TileCoord c = tile_coord<DW_BN, DW_BM>(g, x, t, G);

  // ---- producer state: the A slab held in registers (fetched, not yet staged) and the next one to fetch
  FwStageA<false> sa;
  StageP<RC, DW_BN, 4> sb;
  constexpr int NIA = FwStageA<false>::NI;
  float4 va[NIA];
  uint32_t held_in = 0;                   // bit i: load i's pixel is inside the grid
  bool held = false, held_first = false;  // registers hold a slab; it is its tile's first
  int held_k0 = 0, held_n0 = 0;
  int lt = t, lkt = 0;                    // fetch cursor: tile, slab
  TileCoord lc = c;
  bool lok = true;
  const uint32_t smem_lds = lds_addr(smem);
  auto fetch = [&]() {  // registers <- A of slab (lc, lkt); advance the cursor
    held = lok;
    if (!lok) return;
    const int k0 = lkt * GL_BK;
    const DgTap tp = dg_tap(x, k0);
    held_in = 0;
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      bool in;
      va[i] = dg_load(g, x, sa, lc.m0, tp, i, in);
      held_in |= (uint32_t)in << i;
    }
    held_k0 = k0;
    held_n0 = lc.n0;
    held_first = lkt == 0;
    if (++lkt == lc.nk) {
      lt += G;
      lkt = 0;
      lok = lt < x.ntiles;
      if (lok) lc = tile_coord<DW_BN, DW_BM>(g, x, lt, G);
    }
  };
  auto put = [&](int stage) {  // the held slab -> stage: B's planes by LDS-DMA (issued first), A's planes split here
    if (held_first) sb.init(g.b, g.b.p, g.N, held_n0, 0, pw, lane);
    sb.issue(g.K, held_k0, smem_lds + (uint32_t)(stage * DW_STB + 3 * FW_PLA), pw);
    char* st = sm + stage * DW_STB;
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      const float4 w = (held_in >> i) & 1u ? va[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      sa.store(w, i, st, GL_BK);
    }
  };
  // before the barrier that publishes a stage: its DMA has landed (every later vector-memory operation of this wave
  // is one of fetch()'s NIA register loads) and the plane writes are in LDS
  auto publish = [&]() {
    if (held) wait_vm_n<NIA>();
    else wait_vm0();
    wait_lgkm0();
  };

  // EPI_C1FOLD, producers: lane pair (2 r, 2 r + 1) of the 256 producer lanes takes tile row r -- taps 0-4 and mask
  // words 0-3, taps 5-8 and words 4-7 -- into registers and on to LDS in the tile's slab iteration 1
  float fold_x[5];
  uint32_t fold_w[4];
  auto fold_fetch = [&]() {
    const int ptid = pw * 64 + lane, r = ptid >> 1, hf = ptid & 1;
    int b, t1, f1;
    row_btf(g, min(c.m0 + r, g.M - 1), b, t1, f1);
    const float* xp = g.c1_x + ((long)b * g.c1_T + 2 * t1) * g.c1_F + 2 * f1;
    const uint32_t* wp = g.cm_bits + (((long)b * g.cm_T1 + t1) * g.cm_F1 + f1) * g.cm_bw + (c.n0 >> 5) + 4 * hf;
#pragma unroll
    for (int u = 0; u < 4; ++u) fold_w[u] = wp[u];
#pragma unroll
    for (int u = 0; u < 5; ++u) {  // tap 5 hf + u (the second half's u = 4: tap 8 again, into the padding)
      const int k0 = u, k1 = min(5 + u, 8);
      fold_x[u] = xp[hf ? (k1 / 3) * g.c1_F + k1 % 3 : (k0 / 3) * g.c1_F + k0 % 3];
    }
  };
  auto fold_put = [&]() {
    const int ptid = pw * 64 + lane, r = ptid >> 1, hf = ptid & 1;
#pragma unroll
    for (int u = 0; u < 4; ++u) fold_mk[r * 8 + 4 * hf + u] = fold_w[u];
#pragma unroll
    for (int u = 0; u < 5; ++u) fold_pt[r * DW_FOLD_PT + 5 * hf + u] = fold_x[u];
  };

  int buf = 0;

  // One iteration per slab for both roles: the role's work, then ONE raw s_barrier.  kt: the slab of the tile.
  f32x16 acc[TM][TN];  // consumers only
  auto slab = [&](auto role, int kt) {
    if constexpr (decltype(role)::value) {  // producer
      // EPI_C1FOLD: the tile's rows' operands, in its iteration 1 (the consumers' epilogue of the block's previous tile
      // ended before iteration 0's barrier).  The loads are older than the DMA, so their latency runs under put()'s
      // split and the wait for them asks no more than publish()'s
      const bool fold = EPI == EPI_C1FOLD && kt == 1;
      if (fold) fold_fetch();
      // the slab after this one (the last iteration of a tile: the next tile's first) -> the other stage
      if (held) put(buf ^ 1);
      fetch();
      if (fold) fold_put();
      publish();
    } else {
      const char* st = sm + buf * DW_STB;
      constexpr int PA[6] = {1, 2, 0, 1, 0, 0}, PB[6] = {1, 0, 2, 0, 1, 0};  // mma6's products and order
      // unit u = (k-step hs, column group j): 12 MFMAs on B fragment j, which is read one unit ahead; the next
      // k-step's A fragments are read beside the last unit of the current one (gemm_fwd_ws_kernel's schedule)
      auto load_b = [&](int j, int hs, bf16x8 (&bh)[3]) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
          bh[p] = frag_pl_rc<DW_BN>(reinterpret_cast<const float*>(st + 3 * FW_PLA + p * DW_PLB), wn * TN * 32 + j * 32,
                                    lane, hs);
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

  // EPI_C1FOLD (consumers): the wave's conv1-gradient sums over its tiles of one column tile tx, written (first
  // time) or added (the block returns to tx) to its records when the column tile changes, and at the end
  constexpr int C1K = EPI == EPI_C1FOLD ? 5 * TN : 1;
  float c1k[C1K];
  int c1tx = -1;
  uint32_t c1seen = 0;
  auto c1rec = [&](int tx, int j) {  // sub-tile j's five sums of this lane
    return g.c1_part + ((((long)blockIdx.x * C1NT + 2 * tx + wn) * 4 + 2 * wm + (j >> 1)) * 64 + lane) * 10 + 5 * (j & 1);
  };
  auto c1flush = [&]() {
    if (c1tx < 0) return;
    const bool seen = (c1seen >> c1tx) & 1u;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      float* dst = c1rec(c1tx, j);
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        dst[u] = seen ? dst[u] + c1k[5 * j + u] : c1k[5 * j + u];
        c1k[5 * j + u] = 0.f;
      }
    }
    c1seen |= 1u << c1tx;
  };

  // The whole schedule, written once and instantiated per role: either instantiation executes the prologue barrier
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
    } else if constexpr (EPI == EPI_C1FOLD) {
#pragma unroll
      for (int u = 0; u < C1K; ++u) c1k[u] = 0.f;
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
      for (int kt = 0; kt < c.nk; ++kt) slab(role, kt);
      if constexpr (!P) {
        const int mr0 = c.m0 + wm * TM * 32, nc0 = c.n0 + wn * TN * 32;
        if constexpr (EPI == EPI_C1FOLD) {
          if (c.tn != c1tx) {
            c1flush();
            c1tx = c.tn;
          }
          dg_fold<TM, TN>(g, mr0, wm * TM * 32, wn, lane, acc, fold_pt, fold_mk, c1k);
        } else {
          store_spec_tiles<EPI, TM, TN>(g, 0, mr0, nc0, lane, acc);
        }
      }
      if (!has_next) break;
      t = tnext;
      c = tile_coord<DW_BN, DW_BM>(g, x, t, G);
    }
    if constexpr (!P && EPI == EPI_C1FOLD) {
      c1flush();
      for (int tx = 0; tx < x.ntx; ++tx)  // column tiles this block never ran: zero records
        if (!((c1seen >> tx) & 1u)) {
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            float* dst = c1rec(tx, j);
#pragma unroll
            for (int u = 0; u < 5; ++u) dst[u] = 0.f;
          }
        }
    }
  };
  if (producer) run(std::true_type{});
  else run(std::false_type{});
}

}  // namespace

bool dgrad_ws_launch(int epi, dim3 grid, hipStream_t st, const GemmArgs& g, const GldsArgs& x) {
  if (g.bm != DW_BM || g.bnt != DW_BN || g.N % DW_BN || g.K % GL_BK || g.K < 2 * GL_BK || x.t_C % GL_BK || 2 * x.ntx > C1NT)
    return false;
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(DW_NT), 0, st, g, x); };
  if (epi == EPI_RMASKMAP) go(gemm_dgrad_ws_kernel<EPI_RMASKMAP>);
  else if (epi == EPI_C1FOLD) go(gemm_dgrad_ws_kernel<EPI_C1FOLD>);
  else return false;
  return true;
}

#else

bool dgrad_ws_launch(int, dim3, hipStream_t, const GemmArgs&, const GldsArgs&) { return false; }

#endif

}  // namespace espg
