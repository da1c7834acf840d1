// Convolutional spatial gating unit of the Branchformer's cgMLP branch (espnet2/asr/layers/cgmlp.py:15-81),
// gate_activation identity, no linear after the convolution.  v (M, U) is channel_proj1's plain output
// (M = B*T rows, U = 2C); GELU (exact erf form) is applied on load, so neither a = GELU(v) nor the
// normalised gate n = LayerNorm_C(a_g) reaches HBM in the forward:
//   esp_csgu_stats     mean / rstd of a_g = GELU(v[:, C:]) per row (two passes, fp32)
//   esp_csgu_fwd       o = drop(a_r * (dwconv_k(n) + bias)): n staged per (utterance, 64 frames, 64 channels)
//                      tile in LDS from v, the statistics, gamma and beta; the window in registers
//   esp_csgu_bwd_gate  the same tile with dout: dv[:, :C] = drop'(dout) g GELU'(v_r), dg = drop'(dout) a_r,
//                      and n itself (the depthwise weight gradient's operand)
//   esp_csgu_bwd_norm  LayerNorm adjoint per row on the recomputed a_g: dv[:, C:] = LN'(dn) GELU'(v_g), and
//                      dn * xhat (whose column sum is the LayerNorm weight gradient)
// The convolution adjoints between the two backward kernels are esp_dwconv1d(flip) / esp_dwconv1d_wgrad /
// esp_colsum (kernels.csgu_bwd).
// The cgMLP takes no mask: the window reads every frame of the utterance's own T rows (padded frames of a
// short utterance included, as the reference does), zero outside [0, T) and -- length-bucketed batches, see
// valid_T in norm.hip -- at or after *tvalid; rows at or after *tvalid are written as 0.
#include "common.h"

namespace {

__device__ __forceinline__ int valid_T(const int* tvalid, int T) { return tvalid ? min(T, *tvalid) : T; }

__device__ __forceinline__ float gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
// a = GELU(v) and da/dv = Phi(v) + v phi(v)
__device__ __forceinline__ void gelu_d(float v, float& a, float& d) {
  const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752f));
  a = v * cdf;
  d = cdf + v * 0.39894228040143268f * __expf(-0.5f * v * v);
}

// one wave per row: mean and 1/sqrt(var + eps) (biased variance, about the mean) of GELU(v[row, C:2C])
__global__ __launch_bounds__(256) void csgu_stats_kernel(const float* __restrict__ v, long M, int C, float eps,
                                                         float* __restrict__ mean, float* __restrict__ rstd) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63, C4 = C >> 2;
  const float4* vg = reinterpret_cast<const float4*>(v + row * 2 * C + C);
  float s = 0.f;
  for (int i = lane; i < C4; i += 64) {
    const float4 x = vg[i];
    s += (gelu(x.x) + gelu(x.y)) + (gelu(x.z) + gelu(x.w));
  }
  const float mu = esp::wave_sum(s) / (float)C;
  float q = 0.f;
  for (int i = lane; i < C4; i += 64) {
    const float4 x = vg[i];
    const float a = gelu(x.x) - mu, b = gelu(x.y) - mu, c = gelu(x.z) - mu, d = gelu(x.w) - mu;
    q += (a * a + b * b) + (c * c + d * d);
  }
  q = esp::wave_sum(q) / (float)C;
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = 1.0f / sqrtf(q + eps);
  }
}

constexpr int CG_PT = 16, CG_TT = 4 * CG_PT;  // outputs per thread, frames per block

struct TileArgs {
  const float* v;      // (B*T, 2C)
  const float* mean;   // (B*T)
  const float* rstd;
  const float* gamma;  // (C)  csgu.norm
  const float* beta;
  const float* W;      // (C, k) csgu.conv.weight
  const float* bias;   // (C)
  const float* dout;   // BWD: (B*T, C) gradient of o
  float* o;            // FWD: (B*T, C)
  float* dg;           // BWD: (B*T, C)
  float* nout;         // BWD: (B*T, C)
  void* dv;            // BWD: (B*T, 2C) fp32, or bf16 planes (np = 1 or 3, plane stride ps)
  long ps;
  int np;
  int T, C, k;
  uint32_t thr;
  float scale;
  uint64_t seed;
  const uint64_t* key;
  const int* tvalid;
};

// Block (channel tile of 64, frame tile of CG_TT, utterance).  k <= KT taps, centred in the KT-tap window
// (the other taps are 0), so one instantiation serves every odd k up to KT with the same sums.
template <int KT, bool BWD>
__global__ __launch_bounds__(256) void csgu_tile_kernel(const TileArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[CG_TT + KT - 1][64];
  __shared__ __attribute__((aligned(16))) float gs[CG_TT][64];
  __shared__ float ws[KT][64];
  constexpr int pad = (KT - 1) / 2;
  const int T = a.T, C = a.C, k = a.k;
  const int Tv = valid_T(a.tvalid, T);
  const int c0 = blockIdx.x * 64, t0 = blockIdx.y * CG_TT, b = blockIdx.z;
  const long row0 = (long)b * T;
  // ---- filters: ws[j][cc] = W[c0 + cc][j - (KT - k) / 2], 0 outside the k taps and beyond C
  const int koff = (KT - k) / 2;
  for (int i = threadIdx.x; i < KT * 64; i += 256) {
    const int j = i >> 6, cc = i & 63, kk = j - koff;
    ws[j][cc] = (c0 + cc < C && kk >= 0 && kk < k) ? a.W[(long)(c0 + cc) * k + kk] : 0.f;
  }
  // ---- n = (GELU(v_g) - mean) rstd gamma + beta for frames t0 - pad .. t0 + CG_TT + pad - 1; float4 per
  // lane: 16 lanes per row, 16 rows per pass
  const int q = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  const int c = c0 + 4 * q;
  const bool cin = c < C;  // (C % 4 == 0: the four channels are inside together)
  float4 gm = make_float4(0.f, 0.f, 0.f, 0.f), bt = gm;
  if (cin) {
    gm = *reinterpret_cast<const float4*>(a.gamma + c);
    bt = *reinterpret_cast<const float4*>(a.beta + c);
  }
  for (int r = r0; r < CG_TT + KT - 1; r += 16) {
    const int t = t0 - pad + r;
    float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cin && t >= 0 && t < Tv) {
      const long row = row0 + t;
      const float4 x = *reinterpret_cast<const float4*>(a.v + row * 2 * C + C + c);
      const float mu = a.mean[row], rs = a.rstd[row];
      n.x = (gelu(x.x) - mu) * rs * gm.x + bt.x;
      n.y = (gelu(x.y) - mu) * rs * gm.y + bt.y;
      n.z = (gelu(x.z) - mu) * rs * gm.z + bt.z;
      n.w = (gelu(x.w) - mu) * rs * gm.w + bt.w;
    }
    *reinterpret_cast<float4*>(&xs[r][4 * q]) = n;
  }
  __syncthreads();
  // ---- depthwise window: thread = (channel, 16 consecutive frames), filters and window in registers
  {
    const int cl = threadIdx.x & 63, tg = threadIdx.x >> 6;
    float w[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) w[j] = ws[j][cl];
    float win[CG_PT + KT - 1];
#pragma unroll
    for (int i = 0; i < CG_PT + KT - 1; ++i) win[i] = xs[tg * CG_PT + i][cl];
    const float bv = c0 + cl < C ? a.bias[c0 + cl] : 0.f;
#pragma unroll
    for (int j = 0; j < CG_PT; ++j) {
      float acc = bv;
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) acc += w[kk] * win[j + kk];
      gs[tg * CG_PT + j][cl] = acc;
    }
  }
  __syncthreads();
  // ---- gate, dropout, store: float4 per lane again
  if (!cin) return;
  const uint64_t seed = esp::keyed(a.seed, a.key);
  for (int r = r0; r < CG_TT; r += 16) {
    const int t = t0 + r;
    if (t >= T) break;
    const long row = row0 + t;
    const long off = row * C + c;
    float4 res = make_float4(0.f, 0.f, 0.f, 0.f), res2 = res, nn = res;
    if (t < Tv) {
      const float4 g = *reinterpret_cast<const float4*>(&gs[r][4 * q]);
      const float4 x = *reinterpret_cast<const float4*>(a.v + row * 2 * C + c);
      bool kp[4] = {true, true, true, true};
      if (a.thr) {
        esp::keep_pair(seed, (uint64_t)off, a.thr, kp[0], kp[1]);
        esp::keep_pair(seed, (uint64_t)off + 2, a.thr, kp[2], kp[3]);
      }
      const float gv[4] = {g.x, g.y, g.z, g.w}, xv[4] = {x.x, x.y, x.z, x.w};
      float o1[4], o2[4];
      if constexpr (!BWD) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = gelu(xv[e]) * gv[e];
          o1[e] = a.thr ? (kp[e] ? p * a.scale : 0.f) : p;
        }
      } else {
        const float4 d4 = *reinterpret_cast<const float4*>(a.dout + off);
        const float dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = a.thr ? (kp[e] ? dd[e] * a.scale : 0.f) : dd[e];
          float ar, dar;
          gelu_d(xv[e], ar, dar);
          o1[e] = d * gv[e] * dar;  // d a_r GELU'(v_r)
          o2[e] = d * ar;           // dg
        }
        res2 = make_float4(o2[0], o2[1], o2[2], o2[3]);
        nn = *reinterpret_cast<const float4*>(&xs[r + pad][4 * q]);
      }
      res = make_float4(o1[0], o1[1], o1[2], o1[3]);
    }
    if constexpr (!BWD) {
      *reinterpret_cast<float4*>(a.o + off) = res;
    } else {
      *reinterpret_cast<float4*>(a.dg + off) = res2;
      *reinterpret_cast<float4*>(a.nout + off) = nn;
      const long voff = row * 2 * C + c;
      if (a.np)
        esp::store_planes4(reinterpret_cast<uint16_t*>(a.dv), voff, a.ps, a.np, res.x, res.y, res.z, res.w);
      else
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.dv) + voff) = res;
    }
  }
}

// One wave per row.  xhat = (GELU(v_g) - mean) rstd, gy = dn gamma:
//   da_g = rstd (gy - mean_c(gy) - xhat mean_c(gy xhat)),  dv[:, C:] = da_g GELU'(v_g),  pxh = dn xhat.
// Rows at or after *tvalid: zeros.
__global__ __launch_bounds__(256) void csgu_bwd_norm_kernel(const float* __restrict__ v, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ dn, void* __restrict__ dv,
                                                            long ps, int np, float* __restrict__ pxh, long M, int T,
                                                            int C, const int* __restrict__ tvalid) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63, C4 = C >> 2;
  const int Tv = valid_T(tvalid, T);
  const bool live = (int)(row % T) < Tv;
  const float4* vg = reinterpret_cast<const float4*>(v + row * 2 * C + C);
  const float4* dn4 = reinterpret_cast<const float4*>(dn + row * C);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float mu = mean[row], rs = rstd[row];
  float s1 = 0.f, s2 = 0.f;
  if (live) {
    for (int i = lane; i < C4; i += 64) {
      const float4 x = vg[i], d = dn4[i], g = g4[i];
      const float xv[4] = {x.x, x.y, x.z, x.w}, dd[4] = {d.x, d.y, d.z, d.w}, gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gy = dd[e] * gg[e];
        s1 += gy;
        s2 += gy * ((gelu(xv[e]) - mu) * rs);
      }
    }
    s1 = esp::wave_sum(s1) / (float)C;
    s2 = esp::wave_sum(s2) / (float)C;
  }
  for (int i = lane; i < C4; i += 64) {
    float o[4] = {0.f, 0.f, 0.f, 0.f}, p[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      const float4 x = vg[i], d = dn4[i], g = g4[i];
      const float xv[4] = {x.x, x.y, x.z, x.w}, dd[4] = {d.x, d.y, d.z, d.w}, gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float ag, dag;
        gelu_d(xv[e], ag, dag);
        const float xh = (ag - mu) * rs;
        o[e] = rs * (dd[e] * gg[e] - s1 - xh * s2) * dag;
        p[e] = dd[e] * xh;
      }
    }
    reinterpret_cast<float4*>(pxh + row * C)[i] = make_float4(p[0], p[1], p[2], p[3]);
    const long voff = row * 2 * C + C + 4 * i;
    if (np)
      esp::store_planes4(reinterpret_cast<uint16_t*>(dv), voff, ps, np, o[0], o[1], o[2], o[3]);
    else
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(dv) + voff) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

constexpr int CG_KMAX = 63;

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool BWD>
int launch_tile(const TileArgs& a, int B, hipStream_t st) {
  const dim3 grid((a.C + 63) / 64, (a.T + CG_TT - 1) / CG_TT, B);
  if (a.k <= 7)
    hipLaunchKernelGGL((csgu_tile_kernel<7, BWD>), grid, dim3(256), 0, st, a);
  else if (a.k <= 15)
    hipLaunchKernelGGL((csgu_tile_kernel<15, BWD>), grid, dim3(256), 0, st, a);
  else if (a.k <= 31)
    hipLaunchKernelGGL((csgu_tile_kernel<31, BWD>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((csgu_tile_kernel<CG_KMAX, BWD>), grid, dim3(256), 0, st, a);
  return 0;
}

}  // namespace

#define CSGU_SHAPE_CHECK(name)                                                                                   \
  ESP_ARG_CHECK(B >= 0 && T >= 1 && C >= 4 && C % 4 == 0 && k >= 1 && k % 2 == 1 && k <= CG_KMAX && B <= 65535 && \
                    (T + CG_TT - 1) / CG_TT <= 65535,                                                            \
                name ": bad shape B=%d T=%d C=%d k=%d (C %% 4 == 0, k odd and <= %d)", B, T, C, k, CG_KMAX)

ESP_API int esp_csgu_stats(const float* v, long M, int C, float eps, float* mean, float* rstd, void* stream) {
  ESP_ARG_CHECK(M >= 0 && C >= 4 && C % 4 == 0 && (M + 3) / 4 < (1L << 31), "esp_csgu_stats: bad shape M=%ld C=%d", M, C);
  ESP_ARG_CHECK(v && mean && rstd && al16(v), "esp_csgu_stats: null or unaligned operand");
  if (M == 0) return 0;
  hipLaunchKernelGGL(csgu_stats_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, v, M, C, eps,
                     mean, rstd);
  ESP_CHECK_LAUNCH("esp_csgu_stats");
  return 0;
}

ESP_API int esp_csgu_fwd(const float* v, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* W, const float* bias, float* o, int B, int T, int C, int k, float drop_p,
                         unsigned long long seed, const int* tvalid, void* stream) {
  CSGU_SHAPE_CHECK("esp_csgu_fwd");
  ESP_ARG_CHECK(drop_p < 1.f, "dropout p must be < 1 (got %g)", (double)drop_p);
  ESP_ARG_CHECK(v && mean && rstd && gamma && beta && W && bias && o && al16(v) && al16(gamma) && al16(beta) && al16(o),
                "esp_csgu_fwd: null or unaligned operand");
  if (B == 0) return 0;
  TileArgs a{};
  a.v = v; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.W = W; a.bias = bias; a.o = o;
  a.T = T; a.C = C; a.k = k;
  a.thr = esp::drop_threshold(drop_p);
  a.scale = esp::drop_scale(a.thr);
  a.seed = (uint64_t)seed;
  a.key = esp::rng_key_ptr();
  a.tvalid = tvalid;
  launch_tile<false>(a, B, (hipStream_t)stream);
  ESP_CHECK_LAUNCH("esp_csgu_fwd");
  return 0;
}

ESP_API int esp_csgu_bwd_gate(const float* v, const float* mean, const float* rstd, const float* gamma,
                              const float* beta, const float* W, const float* bias, const float* dout, void* dv,
                              long pstride, int nplanes, float* dg, float* n, int B, int T, int C, int k, float drop_p,
                              unsigned long long seed, const int* tvalid, void* stream) {
  CSGU_SHAPE_CHECK("esp_csgu_bwd_gate");
  ESP_ARG_CHECK(drop_p < 1.f, "dropout p must be < 1 (got %g)", (double)drop_p);
  ESP_ARG_CHECK(v && mean && rstd && gamma && beta && W && bias && dout && dv && dg && n && al16(v) && al16(gamma) &&
                    al16(beta) && al16(dout) && al16(dv) && al16(dg) && al16(n),
                "esp_csgu_bwd_gate: null or unaligned operand");
  ESP_ARG_CHECK(nplanes == 0 || ((nplanes == 1 || nplanes == 3) && pstride % 4 == 0 && pstride >= (long)B * T * 2 * C),
                "esp_csgu_bwd_gate: nplanes 0 (fp32 dv), 1 or 3 with pstride >= B*T*2C");
  if (B == 0) return 0;
  TileArgs a{};
  a.v = v; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.W = W; a.bias = bias; a.dout = dout;
  a.dv = dv; a.ps = pstride; a.np = nplanes; a.dg = dg; a.nout = n;
  a.T = T; a.C = C; a.k = k;
  a.thr = esp::drop_threshold(drop_p);
  a.scale = esp::drop_scale(a.thr);
  a.seed = (uint64_t)seed;
  a.key = esp::rng_key_ptr();
  a.tvalid = tvalid;
  launch_tile<true>(a, B, (hipStream_t)stream);
  ESP_CHECK_LAUNCH("esp_csgu_bwd_gate");
  return 0;
}

ESP_API int esp_csgu_bwd_norm(const float* v, const float* mean, const float* rstd, const float* gamma, const float* dn,
                              void* dv, long pstride, int nplanes, float* pxh, int B, int T, int C, const int* tvalid,
                              void* stream) {
  ESP_ARG_CHECK(B >= 0 && T >= 1 && C >= 4 && C % 4 == 0, "esp_csgu_bwd_norm: bad shape B=%d T=%d C=%d", B, T, C);
  ESP_ARG_CHECK(v && mean && rstd && gamma && dn && dv && pxh && al16(v) && al16(gamma) && al16(dn) && al16(dv) &&
                    al16(pxh),
                "esp_csgu_bwd_norm: null or unaligned operand");
  ESP_ARG_CHECK(nplanes == 0 || ((nplanes == 1 || nplanes == 3) && pstride % 4 == 0 && pstride >= (long)B * T * 2 * C),
                "esp_csgu_bwd_norm: nplanes 0 (fp32 dv), 1 or 3 with pstride >= B*T*2C");
  const long M = (long)B * T;
  if (M == 0) return 0;
  ESP_ARG_CHECK((M + 3) / 4 < (1L << 31), "esp_csgu_bwd_norm: %ld rows", M);
  hipLaunchKernelGGL(csgu_bwd_norm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, v, mean,
                     rstd, gamma, dn, dv, pstride, nplanes, pxh, M, T, C, tvalid);
  ESP_CHECK_LAUNCH("esp_csgu_bwd_norm");
  return 0;
}
