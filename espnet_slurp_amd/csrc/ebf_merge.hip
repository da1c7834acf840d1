// The E-Branchformer's enhanced merge (espnet2/asr/encoder/e_branchformer_encoder.py:158-163) around merge_proj:
//   u[b,t,c] = xc[b,t,c] + bias[c] + sum_j W[c,j] xc[b, t + j - pad, c]        (depthwise_conv_fusion + the add)
// xc (B*T, C) is the concatenation [x1, x2] of the two branch outputs (C = 2D), W (C, k) the depthwise taps.
//   esp_ebf_merge_fwd  u in one pass over xc, written in merge_proj's operand format: fp32 (nplanes 0) or bf16
//                      split planes (nplanes 1 / 3)
//   esp_ebf_merge_bwd  from du = dL/du: dxc = du + conv^T(du) as the two contiguous (B*T, D) halves d1 | d2, and
//                      in the same pass over du and xc the block's partial sums of dW[c,j] = sum du[t] xc[t+j-pad]
//                      and dbias[c] = sum du[t] into the workspace; a second kernel adds the partials in a fixed
//                      order into dW / dbias (+=).  No atomics: two launches give the same bits.
// Tile = (utterance, EM_TT frames, 64 channels) as csgu_tile_kernel (cgmlp.hip): the window staged in LDS by
// float4 rows, a thread owns one channel and EM_PT consecutive frames with the taps and the window in registers.
// The convolution takes no mask: every frame of the utterance's own T rows is read (padded frames included, as
// the reference does), zero outside [0, T) and -- length-bucketed batches, valid_T in norm.hip -- at or after
// *tvalid; rows at or after *tvalid are written as 0.
#include "common.h"

namespace {

__device__ __forceinline__ int valid_T(const int* tvalid, int T) { return tvalid ? min(T, *tvalid) : T; }

constexpr int EM_PT = 16, EM_TT = 4 * EM_PT;  // outputs per thread, frames per block
constexpr int EM_KMAX = 31;

struct MergeArgs {
  const float* xc;    // (B*T, C)
  const float* W;     // (C, k)
  const float* bias;  // (C)            FWD
  const float* du;    // (B*T, C)       BWD
  void* u;            // FWD: (B*T, C) fp32, or bf16 planes (np = 1 or 3, plane stride ps)
  long ps;
  int np;
  float* d1;          // BWD: (B*T, C/2) each
  float* d2;
  float* part;        // BWD: (B * blocks per utterance, C, k + 1) partial sums, column k = the bias gradient's
  int T, C, k;
  const int* tvalid;
};

// rows t0 - pad .. t0 + EM_TT + pad - 1 of channels c0 .. c0 + 63 of src into xs (zero outside [0, Tv) x [0, C)):
// float4 per lane, 16 lanes per row, 16 rows per pass
template <int KT>
__device__ __forceinline__ void stage_rows(float (*xs)[64], const float* __restrict__ src, long row0, int t0, int Tv,
                                           int C, int c0) {
  constexpr int pad = (KT - 1) / 2;
  const int q = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  const int c = c0 + 4 * q;
  const bool cin = c < C;  // (C % 4 == 0: the four channels are inside together)
  for (int r = r0; r < EM_TT + KT - 1; r += 16) {
    const int t = t0 - pad + r;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cin && t >= 0 && t < Tv) x = *reinterpret_cast<const float4*>(src + (row0 + t) * C + c);
    *reinterpret_cast<float4*>(&xs[r][4 * q]) = x;
  }
}

// ws[j][cc] = W[c0 + cc][j - (KT - k) / 2] (flip: the mirrored tap), 0 outside the k taps and beyond C: the k
// taps sit centred in the KT-tap window, so one instantiation serves every odd k up to KT with the same sums
template <int KT>
__device__ __forceinline__ void stage_taps(float (*ws)[64], const float* __restrict__ W, int C, int k, int c0,
                                           bool flip) {
  const int koff = (KT - k) / 2;
  for (int i = threadIdx.x; i < KT * 64; i += 256) {
    const int j = i >> 6, cc = i & 63, kk = (flip ? KT - 1 - j : j) - koff;
    ws[j][cc] = (c0 + cc < C && kk >= 0 && kk < k) ? W[(long)(c0 + cc) * k + kk] : 0.f;
  }
}

template <int KT>
__global__ __launch_bounds__(256) void ebf_merge_fwd_kernel(const MergeArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[EM_TT + KT - 1][64];
  __shared__ __attribute__((aligned(16))) float us[EM_TT][64];
  __shared__ float ws[KT][64];
  constexpr int pad = (KT - 1) / 2;
  const int T = a.T, C = a.C;
  const int Tv = valid_T(a.tvalid, T);
  const int c0 = blockIdx.x * 64, t0 = blockIdx.y * EM_TT, b = blockIdx.z;
  const long row0 = (long)b * T;
  stage_taps<KT>(ws, a.W, C, a.k, c0, false);
  stage_rows<KT>(xs, a.xc, row0, t0, Tv, C, c0);
  __syncthreads();
  {
    const int cl = threadIdx.x & 63, tg = threadIdx.x >> 6;
    float w[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) w[j] = ws[j][cl];
    float win[EM_PT + KT - 1];
#pragma unroll
    for (int i = 0; i < EM_PT + KT - 1; ++i) win[i] = xs[tg * EM_PT + i][cl];
    const float bv = c0 + cl < C ? a.bias[c0 + cl] : 0.f;
#pragma unroll
    for (int j = 0; j < EM_PT; ++j) {
      float acc = bv;
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) acc += w[kk] * win[j + kk];
      us[tg * EM_PT + j][cl] = win[j + pad] + acc;
    }
  }
  __syncthreads();
  const int q = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  const int c = c0 + 4 * q;
  if (c >= C) return;
  for (int r = r0; r < EM_TT; r += 16) {
    const int t = t0 + r;
    if (t >= T) break;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < Tv) v = *reinterpret_cast<const float4*>(&us[r][4 * q]);
    const long off = (row0 + t) * C + c;
    if (a.np)
      esp::store_planes4(reinterpret_cast<uint16_t*>(a.u), off, a.ps, a.np, v.x, v.y, v.z, v.w);
    else
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.u) + off) = v;
  }
}

// A block walks EM_FPB consecutive frame tiles of its utterance with the parameter sums in registers, so the
// workspace holds one partial per (utterance, EM_FPB frame tiles), not one per tile.
constexpr int EM_FPB = 4;

template <int KT>
__global__ __launch_bounds__(256) void ebf_merge_bwd_kernel(const MergeArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[EM_TT + KT - 1][64];  // xc window; then the dxc tile
  __shared__ __attribute__((aligned(16))) float ds[EM_TT + KT - 1][64];  // du window
  __shared__ float ws[KT + 1][64];                                       // flipped taps; then the block's sums
  constexpr int pad = (KT - 1) / 2;
  const int T = a.T, C = a.C, k = a.k;
  const int Tv = valid_T(a.tvalid, T);
  const int c0 = blockIdx.x * 64, b = blockIdx.z;
  const long row0 = (long)b * T;
  const int cl = threadIdx.x & 63, tg = threadIdx.x >> 6;
  const int q = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  const int c = c0 + 4 * q;
  const int D = C >> 1;
  // (D % 4 == 0: a lane's four channels are in one half together)
  float* dst = c < D ? a.d1 + c : a.d2 + (c - D);
  stage_taps<KT>(ws, a.W, C, k, c0, true);
  __syncthreads();
  float w[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) w[j] = ws[j][cl];
  // the thread's share of the parameter sums over its 16 frames of every tile:
  // pw[j] = sum du[t] xc[t + j - pad], pb = sum du[t]  (frames at or after Tv hold du = 0 in ds)
  float pw[KT], pb = 0.f;
#pragma unroll
  for (int j = 0; j < KT; ++j) pw[j] = 0.f;
  for (int f = 0; f < EM_FPB; ++f) {
    const int t0 = (blockIdx.y * EM_FPB + f) * EM_TT;
    if (t0 >= T) break;  // (uniform over the block)
    stage_rows<KT>(xs, a.xc, row0, t0, Tv, C, c0);
    stage_rows<KT>(ds, a.du, row0, t0, Tv, C, c0);
    __syncthreads();
    {
      float g[EM_PT];
#pragma unroll
      for (int i = 0; i < EM_PT; ++i) {
        g[i] = ds[tg * EM_PT + i + pad][cl];
        pb += g[i];
      }
      float win[EM_PT + KT - 1];
#pragma unroll
      for (int i = 0; i < EM_PT + KT - 1; ++i) win[i] = xs[tg * EM_PT + i][cl];
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        float acc = pw[j];
#pragma unroll
        for (int i = 0; i < EM_PT; ++i) acc += g[i] * win[i + j];
        pw[j] = acc;
      }
    }
    __syncthreads();  // xs is free
    // ---- dxc = du + sum_j W[j] du[t - j + pad] into xs rows 0 .. EM_TT - 1
    {
      float win[EM_PT + KT - 1];
#pragma unroll
      for (int i = 0; i < EM_PT + KT - 1; ++i) win[i] = ds[tg * EM_PT + i][cl];
#pragma unroll
      for (int j = 0; j < EM_PT; ++j) {
        float acc = win[j + pad];
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) acc += w[kk] * win[j + kk];
        xs[tg * EM_PT + j][cl] = acc;
      }
    }
    __syncthreads();
    // ---- d1 | d2: float4 per lane
    if (c < C) {
      for (int r = r0; r < EM_TT; r += 16) {
        const int t = t0 + r;
        if (t >= T) break;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < Tv) v = *reinterpret_cast<const float4*>(&xs[r][4 * q]);
        *reinterpret_cast<float4*>(dst + (row0 + t) * D) = v;
      }
    }
    __syncthreads();  // xs and ds are free for the next tile
  }
  // ---- the four frame groups' sums added in the order 0, 1, 2, 3 (ws: every thread holds its taps)
  for (int g = 0; g < 4; ++g) {
    if (tg == g) {
#pragma unroll
      for (int j = 0; j < KT; ++j) ws[j][cl] = g ? ws[j][cl] + pw[j] : pw[j];
      ws[KT][cl] = g ? ws[KT][cl] + pb : pb;
    }
    __syncthreads();
  }
  // partial sums: part[block][c][0 .. k-1] = dW, [k] = dbias
  const int koff = (KT - k) / 2;
  float* pr = a.part + ((long)(b * gridDim.y + blockIdx.y) * C + c0) * (k + 1);
  for (int i = threadIdx.x; i < 64 * (k + 1); i += 256) {
    const int cc = i / (k + 1), j = i - cc * (k + 1);
    if (c0 + cc < C) pr[i] = j < k ? ws[j + koff][cc] : ws[KT][cc];
  }
}

// out[e] += the sum over the partials of part[i][e], e < n = C * (k + 1): column j < k of channel c is dW[c][j],
// column k is dbias[c].  Thread (e, g) adds the partials i = g, g + 4, ... in that order; the four sums are then
// added in the order 0, 1, 2, 3.
__global__ __launch_bounds__(256) void ebf_merge_reduce_kernel(const float* __restrict__ part, int nparts, int C, int k,
                                                               float* __restrict__ dW, float* __restrict__ dbias) {
  __shared__ float sh[4][64];
  const int el = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;
  const int n = C * (k + 1);
  float s = 0.f;
  if (e < n)
    for (int i = g; i < nparts; i += 4) s += part[(long)i * n + e];
  sh[g][el] = s;
  __syncthreads();
  if (g || e >= n) return;
  s = ((sh[0][el] + sh[1][el]) + sh[2][el]) + sh[3][el];
  const int c = e / (k + 1), j = e - c * (k + 1);
  if (j < k)
    dW[(long)c * k + j] += s;
  else
    dbias[c] += s;
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int frame_tiles(int T) { return (T + EM_TT - 1) / EM_TT; }
int frame_blocks(int T) { return (frame_tiles(T) + EM_FPB - 1) / EM_FPB; }  // the backward's blocks per utterance

bool shape_ok(int B, int T, int C, int k) {
  return B >= 0 && B <= 65535 && T >= 1 && frame_tiles(T) <= 65535 && C >= 8 && C % 8 == 0 && k >= 1 && k % 2 == 1 &&
         k <= EM_KMAX;
}

template <template <int> class L>
void dispatch(int k, dim3 grid, hipStream_t st, const MergeArgs& a) {
  if (k <= 7)
    L<7>::launch(grid, st, a);
  else if (k <= 15)
    L<15>::launch(grid, st, a);
  else
    L<31>::launch(grid, st, a);
}
template <int KT>
struct Fwd {
  static void launch(dim3 grid, hipStream_t st, const MergeArgs& a) {
    hipLaunchKernelGGL(ebf_merge_fwd_kernel<KT>, grid, dim3(256), 0, st, a);
  }
};
template <int KT>
struct Bwd {
  static void launch(dim3 grid, hipStream_t st, const MergeArgs& a) {
    hipLaunchKernelGGL(ebf_merge_bwd_kernel<KT>, grid, dim3(256), 0, st, a);
  }
};

}  // namespace

#define EBF_SHAPE_CHECK(name)                                                                                   \
  ESP_ARG_CHECK(shape_ok(B, T, C, k), name ": bad shape B=%d T=%d C=%d k=%d (C %% 8 == 0, k odd and <= %d)", B, T, C, \
                k, EM_KMAX)

ESP_API int esp_ebf_merge_fwd(const float* xc, const float* W, const float* bias, void* u, long pstride, int nplanes,
                              int B, int T, int C, int k, const int* tvalid, void* stream) {
  EBF_SHAPE_CHECK("esp_ebf_merge_fwd");
  ESP_ARG_CHECK(xc && W && bias && u && al16(xc) && al16(u), "esp_ebf_merge_fwd: null or unaligned operand");
  ESP_ARG_CHECK(nplanes == 0 || ((nplanes == 1 || nplanes == 3) && pstride % 4 == 0 && pstride >= (long)B * T * C),
                "esp_ebf_merge_fwd: nplanes 0 (fp32 u), 1 or 3 with pstride >= B*T*C");
  if (B == 0) return 0;
  MergeArgs a{};
  a.xc = xc; a.W = W; a.bias = bias; a.u = u; a.ps = pstride; a.np = nplanes;
  a.T = T; a.C = C; a.k = k; a.tvalid = tvalid;
  dispatch<Fwd>(k, dim3((C + 63) / 64, frame_tiles(T), B), (hipStream_t)stream, a);
  ESP_CHECK_LAUNCH("esp_ebf_merge_fwd");
  return 0;
}

// workspace: B * (backward blocks per utterance) * C * (k + 1) floats
ESP_API long esp_ebf_merge_bwd_workspace_bytes(int B, int T, int C, int k) {
  return B <= 0 || T <= 0 || C <= 0 || k <= 0 ? 0 : 4L * B * frame_blocks(T) * C * (k + 1);
}

ESP_API int esp_ebf_merge_bwd(const float* du, const float* xc, const float* W, float* d1, float* d2, float* dW,
                              float* dbias, int B, int T, int C, int k, float* work, long work_bytes,
                              const int* tvalid, void* stream) {
  EBF_SHAPE_CHECK("esp_ebf_merge_bwd");
  ESP_ARG_CHECK(du && xc && W && d1 && d2 && dW && dbias && al16(du) && al16(xc) && al16(d1) && al16(d2),
                "esp_ebf_merge_bwd: null or unaligned operand");
  const long need__ = esp_ebf_merge_bwd_workspace_bytes(B, T, C, k);
  ESP_ARG_CHECK(work_bytes >= need__ && (work || need__ == 0),
                "esp_ebf_merge_bwd: workspace %ld B < %ld B required (esp_ebf_merge_bwd_workspace_bytes)", work_bytes,
                need__);
  ESP_ARG_CHECK((long)B * frame_blocks(T) < (1L << 31) && (long)C * (k + 1) < (1L << 31),
                "esp_ebf_merge_bwd: %ld partial sums", (long)B * frame_blocks(T));
  if (B == 0) return 0;
  MergeArgs a{};
  a.du = du; a.xc = xc; a.W = W; a.d1 = d1; a.d2 = d2; a.part = work;
  a.T = T; a.C = C; a.k = k; a.tvalid = tvalid;
  hipStream_t st = (hipStream_t)stream;
  dispatch<Bwd>(k, dim3((C + 63) / 64, frame_blocks(T), B), st, a);
  hipLaunchKernelGGL(ebf_merge_reduce_kernel, dim3((C * (k + 1) + 63) / 64), dim3(256), 0, st, work,
                     B * frame_blocks(T), C, k, dW, dbias);
  ESP_CHECK_LAUNCH("esp_ebf_merge_bwd");
  return 0;
}
