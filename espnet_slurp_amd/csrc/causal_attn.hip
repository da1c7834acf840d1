// Causal self-attention of the Transformer LM's training step (espnet2/lm/transformer_lm.py forward over
// espnet/nets/pytorch_backend/transformer/attention.py:16-114 with the LM's _target_mask: causality and a key
// length per sequence; attention_dropout_rate is 0.0 in the reference's LM, so there is no dropout here).
//
// esp_causal_attn_fwd / _bwd: B sequences of L <= 64 tokens, one workgroup per (sequence b, head h), on the tiles
// of attn_tile.h (thread layout, LDS pitch, exact fp32 FMA).  Key j is visible to query i iff j <= i and
// j < klen[b]; the scale is 1 / sqrt(dk).
//   forward   Q, K, V (klen[b] rows each, the rest zero-filled) are staged once in LDS; Q.K^T (only the 16 x 16
//             tiles on and below the diagonal), the mask, the softmax and P.V stay in registers and LDS; only ctx and
//             the row log-sum-exp reach memory.
//   backward  recomputes P = exp(s - lse) from Q and K, forms dP = dctx.V^T, dS = P (dP - sum_j P dP) / sqrt(dk),
//             then dV = P^T dctx, dK = dS^T Q, dQ = dS K.  Every element of dqkv has one owner and is written: no
//             pre-zeroing, no atomics, results repeat bit for bit.
//   padding   query rows i >= klen[b]: ctx = 0, lse = 0, dq = 0; key rows j >= klen[b]: dk = dv = 0 (exact zeros:
//             their P and dS columns are zero and the staged operands are finite).  klen[b] is clamped to [0, L].
//   shapes    dk in {16, 32, 64, 128}, 1 <= L <= Lmax(dk):
//                 dk    16   32   64   128
//                 Lmax  64   64   64    64
//             LDS at L > 48: forward (region_a + 2 tiles) 27 / 35 / 51 / 99 KiB, backward (region_a + 3 tiles)
//             32 / 44 / 68 / 132 KiB of the CU's 160 KiB (dk = 128, L = 64: 4 x 64 x 132 floats), granted per
//             kernel above 64 KiB; so dk = 128 reaches L = 64 without a loop over key tiles.
#include "attn_tile.h"

namespace {

constexpr int kMaxL = 64;

__device__ __forceinline__ int clamp_len(const int* __restrict__ klen, long b, int L) {
  const int n = klen[b];
  return n < 0 ? 0 : (n > L ? L : n);
}

template <int DK, int NA>
__global__ void __launch_bounds__(kThreads)
causal_attn_fwd_kernel(const float* __restrict__ qkv, const int* __restrict__ klen, float* __restrict__ ctx,
                       float* __restrict__ lse, int L, int H, float inv_sqrt_dk) {
  extern __shared__ float4 smem4[];
  constexpr int SP = 16 * NA, P = DK + 4, PP = SP + 4;
  float* sQ = reinterpret_cast<float*>(smem4);  // later the probabilities
  float* sK = sQ + region_a<DK, NA>();
  float* sV = sK + SP * P;
  const long zh = blockIdx.x;
  const long b = zh / H;
  const int h = (int)(zh - b * H);
  const int kl = clamp_len(klen, b, L);
  const long D = (long)H * DK, ld = 3 * D;
  const float* base = qkv + b * L * ld + (long)h * DK;
  stage_tile<DK>(sQ, base, ld, kl, SP);
  stage_tile<DK>(sK, base + D, ld, kl, SP);
  stage_tile<DK>(sV, base + 2 * D, ld, kl, SP);
  __syncthreads();
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  float s[NA][NA];
  mm_nt<DK, NA, true>(sQ, sK, ti, tj, s);
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = ti + 16 * a;
    const bool live = i < kl;
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < NA; ++c) {
      const int j = tj + 16 * c;
      s[a][c] *= inv_sqrt_dk;
      if (live && j <= i) m = fmaxf(m, s[a][c]);
    }
    m = group_max(m);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NA; ++c) {
      const int j = tj + 16 * c;
      s[a][c] = live && j <= i ? expf(s[a][c] - m) : 0.f;
      sum += s[a][c];
    }
    sum = group_sum(sum);
    const float inv = live ? 1.0f / sum : 0.f;  // (a live row sees key 0 at least: sum >= 1)
    if (tj == 0 && i < L) lse[zh * L + i] = live ? m + logf(sum) : 0.f;
#pragma unroll
    for (int c = 0; c < NA; ++c) s[a][c] *= inv;
  }
  __syncthreads();  // every thread has read its Q rows
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int c = 0; c < NA; ++c) sQ[(ti + 16 * a) * PP + tj + 16 * c] = s[a][c];
  __syncthreads();
  float o[NA][DK / 16];
  mm_nn<DK, NA>(sQ, PP, sV, (kl + 3) & ~3, ti, tj, o);
  store_rows<DK, NA>(ctx + b * L * D + (long)h * DK, D, L, ti, tj, o);
}

template <int DK, int NA>
__global__ void __launch_bounds__(kThreads)
causal_attn_bwd_kernel(const float* __restrict__ qkv, const int* __restrict__ klen, const float* __restrict__ dctx,
                       const float* __restrict__ lse, float* __restrict__ dqkv, int L, int H, float inv_sqrt_dk) {
  extern __shared__ float4 smem4[];
  constexpr int SP = 16 * NA, P = DK + 4, PP = SP + 4;
  float* sV = reinterpret_cast<float*>(smem4);  // later P, then dS
  float* sQ = sV + region_a<DK, NA>();
  float* sK = sQ + SP * P;
  float* sG = sK + SP * P;  // dctx
  const long zh = blockIdx.x;
  const long b = zh / H;
  const int h = (int)(zh - b * H);
  const int kl = clamp_len(klen, b, L);
  const long D = (long)H * DK, ld = 3 * D;
  const float* base = qkv + b * L * ld + (long)h * DK;
  stage_tile<DK>(sQ, base, ld, kl, SP);
  stage_tile<DK>(sK, base + D, ld, kl, SP);
  stage_tile<DK>(sV, base + 2 * D, ld, kl, SP);
  stage_tile<DK>(sG, dctx + b * L * D + (long)h * DK, D, kl, SP);
  __syncthreads();
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  float s[NA][NA], g[NA][NA];
  mm_nt<DK, NA, true>(sQ, sK, ti, tj, s);  // scores
  mm_nt<DK, NA, true>(sG, sV, ti, tj, g);  // dP = dctx . V^T
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = ti + 16 * a;
    const bool live = i < kl;
    const float l = live ? lse[zh * L + i] : 0.f;
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < NA; ++c) {
      const int j = tj + 16 * c;
      const float p = live && j <= i ? expf(s[a][c] * inv_sqrt_dk - l) : 0.f;
      dot = fmaf(p, g[a][c], dot);
      s[a][c] = p;
    }
    dot = group_sum(dot);
#pragma unroll
    for (int c = 0; c < NA; ++c) g[a][c] = s[a][c] * (g[a][c] - dot) * inv_sqrt_dk;  // dS
  }
  __syncthreads();  // every thread has read its V rows
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int c = 0; c < NA; ++c) sV[(ti + 16 * a) * PP + tj + 16 * c] = s[a][c];
  __syncthreads();
  float* out = dqkv + b * L * ld + (long)h * DK;
  float r[NA][DK / 16];
  mm_tn<DK, NA>(sV, PP, sG, kl, ti, tj, r);  // dV = P^T dctx
  store_rows<DK, NA>(out + 2 * D, ld, L, ti, tj, r);
  __syncthreads();
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int c = 0; c < NA; ++c) sV[(ti + 16 * a) * PP + tj + 16 * c] = g[a][c];
  __syncthreads();
  mm_tn<DK, NA>(sV, PP, sQ, kl, ti, tj, r);  // dK = dS^T Q
  store_rows<DK, NA>(out + D, ld, L, ti, tj, r);
  mm_nn<DK, NA>(sV, PP, sK, (kl + 3) & ~3, ti, tj, r);  // dQ = dS K
  store_rows<DK, NA>(out, ld, L, ti, tj, r);
}

template <int DK, int NA>
int launch_fwd(const float* qkv, const int* klen, float* ctx, float* lse, int B, int L, int H, hipStream_t st) {
  auto kern = causal_attn_fwd_kernel<DK, NA>;
  const size_t lds = sizeof(float) * (region_a<DK, NA>() + 2 * 16 * NA * (DK + 4));
  // asked once per instantiation and process (the answer is kept): no launch inside a stream capture asks again
  static const hipError_t e = grant_lds(kern, lds);
  ESP_ARG_CHECK(e == hipSuccess, "esp_causal_attn_fwd: %zu bytes of LDS not granted: %s", lds, hipGetErrorString(e));
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * H)), dim3(kThreads), lds, st, qkv, klen, ctx, lse, L, H,
                     1.0f / sqrtf((float)DK));
  ESP_CHECK_LAUNCH("esp_causal_attn_fwd");
  return 0;
}

template <int DK, int NA>
int launch_bwd(const float* qkv, const int* klen, const float* dctx, const float* lse, float* dqkv, int B, int L,
               int H, hipStream_t st) {
  auto kern = causal_attn_bwd_kernel<DK, NA>;
  const size_t lds = sizeof(float) * (region_a<DK, NA>() + 3 * 16 * NA * (DK + 4));
  static const hipError_t e = grant_lds(kern, lds);
  ESP_ARG_CHECK(e == hipSuccess, "esp_causal_attn_bwd: %zu bytes of LDS not granted: %s", lds, hipGetErrorString(e));
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * H)), dim3(kThreads), lds, st, qkv, klen, dctx, lse, dqkv, L, H,
                     1.0f / sqrtf((float)DK));
  ESP_CHECK_LAUNCH("esp_causal_attn_bwd");
  return 0;
}

#define CAUSAL_DISPATCH_DK(FN, DKV, ...)        \
  do {                                          \
    if (na == 1) return FN<DKV, 1>(__VA_ARGS__); \
    if (na == 2) return FN<DKV, 2>(__VA_ARGS__); \
    if (na == 3) return FN<DKV, 3>(__VA_ARGS__); \
    return FN<DKV, 4>(__VA_ARGS__);             \
  } while (0)

#define CAUSAL_DISPATCH(FN, ...)                                  \
  do {                                                            \
    const int na = (L + 15) / 16;                                 \
    if (dk == 16) CAUSAL_DISPATCH_DK(FN, 16, __VA_ARGS__);        \
    if (dk == 32) CAUSAL_DISPATCH_DK(FN, 32, __VA_ARGS__);        \
    if (dk == 64) CAUSAL_DISPATCH_DK(FN, 64, __VA_ARGS__);        \
    CAUSAL_DISPATCH_DK(FN, 128, __VA_ARGS__);                     \
  } while (0)

bool shape_ok(int B, int L, int H, int dk) {
  return L >= 1 && L <= kMaxL && (dk == 16 || dk == 32 || dk == 64 || dk == 128) && H >= 1 && B >= 1 &&
         (long)B * H <= 0x7fffffffL;
}

}  // namespace

ESP_API int esp_causal_attn_fwd(const float* qkv, const int* klen, float* ctx, float* lse, int B, int L, int H, int dk,
                                void* stream) {
  ESP_ARG_CHECK(qkv && klen && ctx && lse, "esp_causal_attn_fwd: null buffer");
  ESP_ARG_CHECK(shape_ok(B, L, H, dk),
                "esp_causal_attn_fwd: unsupported shape B=%d L=%d H=%d dk=%d (1 <= L <= %d, dk 16 / 32 / 64 / 128)", B,
                L, H, dk, kMaxL);
  ESP_ARG_CHECK(!(((uintptr_t)qkv | (uintptr_t)ctx) & 15), "esp_causal_attn_fwd: qkv / ctx need 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  CAUSAL_DISPATCH(launch_fwd, qkv, klen, ctx, lse, B, L, H, st);
}

ESP_API int esp_causal_attn_bwd(const float* qkv, const int* klen, const float* dctx, const float* lse, float* dqkv,
                                int B, int L, int H, int dk, void* stream) {
  ESP_ARG_CHECK(qkv && klen && dctx && lse && dqkv, "esp_causal_attn_bwd: null buffer");
  ESP_ARG_CHECK(shape_ok(B, L, H, dk),
                "esp_causal_attn_bwd: unsupported shape B=%d L=%d H=%d dk=%d (1 <= L <= %d, dk 16 / 32 / 64 / 128)", B,
                L, H, dk, kMaxL);
  ESP_ARG_CHECK(!(((uintptr_t)qkv | (uintptr_t)dctx | (uintptr_t)dqkv) & 15),
                "esp_causal_attn_bwd: qkv / dctx / dqkv need 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  CAUSAL_DISPATCH(launch_bwd, qkv, klen, dctx, lse, dqkv, B, L, H, st);
}
