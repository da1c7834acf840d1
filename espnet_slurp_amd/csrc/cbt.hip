// Kernels of the contextual block Transformer encoder (espnet2/asr/encoder/contextual_block_transformer_encoder.py
// forward_train over espnet/nets/pytorch_backend/transformer/contextual_block_encoder_layer.py).
//
// The encoder cuts the T frames of an utterance into nblk overlapping blocks of S = block_size + 2 slots (slot 0 the
// previous block's context vector, slots 1..bs the frames blk*hop .. blk*hop + bs - 1, slot bs + 1 the block's own
// context vector) and runs every layer on all B*nblk blocks at once.
//
// esp_block_attn_fwd / _bwd: self-attention over Z independent sequences of S <= 64 slots, one workgroup per
// (sequence, head).  Q, K and V (S x dk each) are staged once in LDS; the scores, the fixed mask (key j valid iff
// j <= S - 2, query row 0 dead: its output is zero), the softmax, the dropout and P.V stay in registers and LDS.
// The tile helpers live in attn_tile.h (shared with causal_attn.hip):
//   threads  = 256, thread (ti, tj) = (tid / 16, tid % 16) owns score rows ti + 16a and columns tj + 16b
//              (a, b < NA = ceil(S / 16)): a 16-lane row group reduces a score row with four xor shuffles.
//   LDS      = row-major tiles of pitch dk + 4 (S x S tiles: 16 NA + 4) floats.  The pitch / 4 is odd, so the 16
//              lanes of a row group that read 16 different rows with one ds_read_b128 hit 16 different 16-byte slots
//              of the 256-byte bank row; the rows ti + 16a are shared by a whole row group (a broadcast).
//   products = fp32 FMA (4 x 4 register tiles for Q.K^T and dO.V^T, 4 x dk/16 for P.V and the three gradients).
//   forward  saves only the row log-sum-exp; the backward recomputes P = exp(s - lse) from Q and K and regenerates
//              the dropout mask from the same (seed, index): index = ((z*H + h)*64 + i)*64 + j.
// No atomics: every output element has one owner, so results repeat bit for bit.
//
// esp_cbt_chunk_fwd / _bwd, esp_cbt_ctx_shift_fwd / _bwd, esp_cbt_unchunk_fwd / _bwd: the block layout around the
// layers (see include/espnet_mi355.h); all backward passes are gathers.
#include "attn_tile.h"  // stage_tile, mm_nt / mm_nn / mm_tn, group_max / group_sum, store_rows, region_a, grant_lds

namespace {

constexpr int kMaxS = 64;

__device__ __forceinline__ float drop_mul(uint64_t seed, uint32_t thresh, float dscale, long zh, int i, int j) {
  if (!thresh) return 1.f;
  return esp::keep_elem(seed, (uint64_t)((zh * kMaxS + i) * kMaxS + j), thresh) ? dscale : 0.f;
}

template <int DK, int NA>
__global__ void __launch_bounds__(kThreads)
block_attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ ctx, float* __restrict__ lse, int S, int H,
                      float inv_sqrt_dk, uint64_t seed, const uint64_t* __restrict__ key, uint32_t thresh,
                      float dscale) {
  extern __shared__ float4 smem4[];
  constexpr int SP = 16 * NA, P = DK + 4, PP = SP + 4;
  float* sQ = reinterpret_cast<float*>(smem4);  // later the probabilities
  float* sK = sQ + region_a<DK, NA>();
  float* sV = sK + SP * P;
  const long zh = blockIdx.x;
  const long z = zh / H;
  const int h = (int)(zh - z * H);
  const long D = (long)H * DK, ld = 3 * D;
  const float* base = qkv + z * S * ld + (long)h * DK;
  stage_tile<DK>(sQ, base, ld, S, SP);
  stage_tile<DK>(sK, base + D, ld, S, SP);
  stage_tile<DK>(sV, base + 2 * D, ld, S, SP);
  __syncthreads();
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  float s[NA][NA];
  mm_nt<DK, NA>(sQ, sK, ti, tj, s);
  seed = esp::keyed(seed, key);
  const int nkeys = S - 1;  // keys 0 .. bs
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = ti + 16 * a;
    float m = -INFINITY;
#pragma unroll
    for (int b = 0; b < NA; ++b) {
      s[a][b] *= inv_sqrt_dk;
      if (tj + 16 * b < nkeys) m = fmaxf(m, s[a][b]);
    }
    m = group_max(m);
    float sum = 0.f;
#pragma unroll
    for (int b = 0; b < NA; ++b) {
      s[a][b] = tj + 16 * b < nkeys ? expf(s[a][b] - m) : 0.f;
      sum += s[a][b];
    }
    sum = group_sum(sum);
    const bool live = i >= 1 && i < S;
    const float inv = live ? 1.0f / sum : 0.f;
    if (tj == 0 && i < S) lse[zh * S + i] = m + logf(sum);
#pragma unroll
    for (int b = 0; b < NA; ++b) s[a][b] *= inv * drop_mul(seed, thresh, dscale, zh, i, tj + 16 * b);
  }
  __syncthreads();  // every thread has read its Q rows
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) sQ[(ti + 16 * a) * PP + tj + 16 * b] = s[a][b];
  __syncthreads();
  float o[NA][DK / 16];
  mm_nn<DK, NA>(sQ, PP, sV, (S + 3) & ~3, ti, tj, o);
  store_rows<DK, NA>(ctx + z * S * D + (long)h * DK, D, S, ti, tj, o);
}

template <int DK, int NA>
__global__ void __launch_bounds__(kThreads)
block_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx, const float* __restrict__ lse,
                      float* __restrict__ dqkv, int S, int H, float inv_sqrt_dk, uint64_t seed,
                      const uint64_t* __restrict__ key, uint32_t thresh, float dscale) {
  extern __shared__ float4 smem4[];
  constexpr int SP = 16 * NA, P = DK + 4, PP = SP + 4;
  float* sV = reinterpret_cast<float*>(smem4);  // later P_drop, then dS
  float* sQ = sV + region_a<DK, NA>();
  float* sK = sQ + SP * P;
  float* sG = sK + SP * P;  // dctx
  const long zh = blockIdx.x;
  const long z = zh / H;
  const int h = (int)(zh - z * H);
  const long D = (long)H * DK, ld = 3 * D;
  const float* base = qkv + z * S * ld + (long)h * DK;
  stage_tile<DK>(sQ, base, ld, S, SP);
  stage_tile<DK>(sK, base + D, ld, S, SP);
  stage_tile<DK>(sV, base + 2 * D, ld, S, SP);
  stage_tile<DK>(sG, dctx + z * S * D + (long)h * DK, D, S, SP);
  __syncthreads();
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  float s[NA][NA], g[NA][NA];
  mm_nt<DK, NA>(sQ, sK, ti, tj, s);   // scores
  mm_nt<DK, NA>(sG, sV, ti, tj, g);   // d(P_drop) = dctx . V^T
  seed = esp::keyed(seed, key);
  const int nkeys = S - 1;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = ti + 16 * a;
    const bool live = i >= 1 && i < S;
    const float l = live ? lse[zh * S + i] : 0.f;
    float dot = 0.f, mk[NA];
#pragma unroll
    for (int b = 0; b < NA; ++b) {
      const int j = tj + 16 * b;
      const float p = live && j < nkeys ? expf(s[a][b] * inv_sqrt_dk - l) : 0.f;
      mk[b] = drop_mul(seed, thresh, dscale, zh, i, j);
      const float dp = g[a][b] * mk[b];  // dP
      dot = fmaf(p, dp, dot);
      s[a][b] = p;
      g[a][b] = dp;
    }
    dot = group_sum(dot);
#pragma unroll
    for (int b = 0; b < NA; ++b) {
      const float p = s[a][b];
      s[a][b] = p * mk[b];                          // P_drop
      g[a][b] = p * (g[a][b] - dot) * inv_sqrt_dk;  // dS
    }
  }
  __syncthreads();  // every thread has read its V rows
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) sV[(ti + 16 * a) * PP + tj + 16 * b] = s[a][b];
  __syncthreads();
  float* out = dqkv + z * S * ld + (long)h * DK;
  float r[NA][DK / 16];
  mm_tn<DK, NA>(sV, PP, sG, S, ti, tj, r);  // dV = P_drop^T dctx
  store_rows<DK, NA>(out + 2 * D, ld, S, ti, tj, r);
  __syncthreads();
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) sV[(ti + 16 * a) * PP + tj + 16 * b] = g[a][b];
  __syncthreads();
  mm_tn<DK, NA>(sV, PP, sQ, S, ti, tj, r);  // dK = dS^T Q
  store_rows<DK, NA>(out + D, ld, S, ti, tj, r);
  mm_nn<DK, NA>(sV, PP, sK, (S + 3) & ~3, ti, tj, r);  // dQ = dS K
  store_rows<DK, NA>(out, ld, S, ti, tj, r);
}

template <int DK, int NA>
size_t fwd_lds() { return sizeof(float) * (region_a<DK, NA>() + 2 * 16 * NA * (DK + 4)); }
template <int DK, int NA>
size_t bwd_lds() { return sizeof(float) * (region_a<DK, NA>() + 3 * 16 * NA * (DK + 4)); }

template <int DK, int NA>
int launch_fwd(const float* qkv, float* ctx, float* lse, long Z, int S, int H, float p, uint64_t seed,
               hipStream_t st) {
  const uint32_t thresh = esp::drop_threshold(p);
  auto kern = block_attn_fwd_kernel<DK, NA>;
  const size_t lds = fwd_lds<DK, NA>();
  hipLaunchKernelGGL(kern, dim3((unsigned)(Z * H)), dim3(kThreads), lds, st,
                     qkv, ctx, lse, S, H, 1.0f / sqrtf((float)DK), seed, esp::rng_key_ptr(), thresh,
                     esp::drop_scale(thresh));
  ESP_CHECK_LAUNCH("esp_block_attn_fwd");
  return 0;
}

template <int DK, int NA>
int launch_bwd(const float* qkv, const float* dctx, const float* lse, float* dqkv, long Z, int S, int H, float p,
               uint64_t seed, hipStream_t st) {
  const uint32_t thresh = esp::drop_threshold(p);
  auto kern = block_attn_bwd_kernel<DK, NA>;
  const size_t lds = bwd_lds<DK, NA>();
  // asked once per instantiation and process (the answer is kept): no launch inside a stream capture asks again
  static const hipError_t e = grant_lds(kern, lds);
  ESP_ARG_CHECK(e == hipSuccess, "esp_block_attn_bwd: %zu bytes of LDS not granted: %s", lds, hipGetErrorString(e));
  hipLaunchKernelGGL(kern, dim3((unsigned)(Z * H)), dim3(kThreads), lds, st,
                     qkv, dctx, lse, dqkv, S, H, 1.0f / sqrtf((float)DK), seed, esp::rng_key_ptr(), thresh,
                     esp::drop_scale(thresh));
  ESP_CHECK_LAUNCH("esp_block_attn_bwd");
  return 0;
}

#define CBT_DISPATCH(FN, ...)                                   \
  do {                                                          \
    const int na = (S + 15) / 16;                               \
    if (dk == 16) {                                             \
      if (na == 1) return FN<16, 1>(__VA_ARGS__);               \
      if (na == 2) return FN<16, 2>(__VA_ARGS__);               \
      if (na == 3) return FN<16, 3>(__VA_ARGS__);               \
      return FN<16, 4>(__VA_ARGS__);                            \
    }                                                           \
    if (dk == 32) {                                             \
      if (na == 1) return FN<32, 1>(__VA_ARGS__);               \
      if (na == 2) return FN<32, 2>(__VA_ARGS__);               \
      if (na == 3) return FN<32, 3>(__VA_ARGS__);               \
      return FN<32, 4>(__VA_ARGS__);                            \
    }                                                           \
    if (na == 1) return FN<64, 1>(__VA_ARGS__);                 \
    if (na == 2) return FN<64, 2>(__VA_ARGS__);                 \
    if (na == 3) return FN<64, 3>(__VA_ARGS__);                 \
    return FN<64, 4>(__VA_ARGS__);                              \
  } while (0)

// ------------------------------------------------------------------------------------------------ block layout
struct Layout {
  int T, bs, hop, la, nblk, S;
};

// blocks whose frame window [blk*hop, blk*hop + bs) holds frame t
__device__ __forceinline__ void blocks_of(const Layout& L, int t, int& lo, int& hi) {
  lo = t - L.bs + 1 <= 0 ? 0 : (t - L.bs + L.hop) / L.hop;
  hi = t / L.hop;
  if (hi > L.nblk - 1) hi = L.nblk - 1;
}
__device__ __forceinline__ int window_len(const Layout& L, int blk) {
  const int n = L.T - blk * L.hop;
  return n < L.bs ? n : L.bs;
}
// the (block, slot) an output frame is copied from
__device__ __forceinline__ void source_of(const Layout& L, int t, int& blk, int& slot) {
  const int first = L.bs - L.la;
  if (t < first) {
    blk = 0;
  } else {
    blk = (t - first) / L.hop + 1;
    if (blk > L.nblk - 1) blk = L.nblk - 1;
  }
  slot = t - blk * L.hop + 1;
}

// one workgroup per (b, blk); thread per channel
__global__ void __launch_bounds__(kThreads)
chunk_fwd_kernel(const float* __restrict__ x, const float* __restrict__ pe, float* __restrict__ xs, Layout L, int D,
                 float xscale, int ctx_pe, uint64_t seed_x, uint64_t seed_c, const uint64_t* __restrict__ key,
                 uint32_t thresh, float dscale) {
  const int b = blockIdx.x / L.nblk, blk = blockIdx.x - b * L.nblk;
  seed_x = esp::keyed(seed_x, key);
  seed_c = esp::keyed(seed_c, key);
  const float* xb = x + (long)b * L.T * D;
  float* out = xs + (long)blockIdx.x * L.S * D;
  for (int c = threadIdx.x; c < D; c += kThreads) {
    // the context vectors of this block and of the one before it: window means of the un-scaled frames
    float mean[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const int kb = w == 0 ? (blk > 0 ? blk - 1 : 0) : blk;
      const int n = window_len(L, kb);
      float sum = 0.f;
      for (int t = kb * L.hop; t < kb * L.hop + n; ++t) sum += xb[(long)t * D + c];
      float v = sum / (float)n;
      if (ctx_pe) {
        v = fmaf(v, xscale, pe[(long)kb * D + c]);
        if (thresh) v = esp::keep_elem(seed_c, (uint64_t)(((long)b * L.nblk + kb) * D + c), thresh) ? v * dscale : 0.f;
      }
      mean[w] = v;
    }
    out[c] = mean[0];
    out[(long)(L.bs + 1) * D + c] = mean[1];
    for (int s = 1; s <= L.bs; ++s) {
      const int t = blk * L.hop + s - 1;
      float v = 0.f;
      if (t < L.T) {
        v = fmaf(xb[(long)t * D + c], xscale, pe[(long)t * D + c]);
        if (thresh) v = esp::keep_elem(seed_x, (uint64_t)(((long)b * L.T + t) * D + c), thresh) ? v * dscale : 0.f;
      }
      out[(long)s * D + c] = v;
    }
  }
}

// thread per (b, t, c): the blocks that hold frame t and the means whose window holds it are the same blocks
__global__ void __launch_bounds__(kThreads)
chunk_bwd_kernel(const float* __restrict__ dxs, float* __restrict__ dx, Layout L, int D, long total, float xscale,
                 int ctx_pe, uint64_t seed_x, uint64_t seed_c, const uint64_t* __restrict__ key, uint32_t thresh,
                 float dscale) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  seed_x = esp::keyed(seed_x, key);
  seed_c = esp::keyed(seed_c, key);
  const int c = (int)(e % D);
  const long bt = e / D;
  const int t = (int)(bt % L.T), b = (int)(bt / L.T);
  int lo, hi;
  blocks_of(L, t, lo, hi);
  const long SD = (long)L.S * D;
  const float* db = dxs + (long)b * L.nblk * SD + c;
  float gf = 0.f, gm = 0.f;
  for (int blk = lo; blk <= hi; ++blk) {
    gf += db[blk * SD + (long)(t - blk * L.hop + 1) * D];
    // gradient of block blk's context vector: its own slot, the next block's slot 0, and block 0's slot 0
    float ga = db[blk * SD + (long)(L.bs + 1) * D];
    if (blk + 1 < L.nblk) ga += db[(blk + 1) * SD];
    if (blk == 0) ga += db[0];
    if (ctx_pe) {
      ga *= xscale;
      if (thresh) ga = esp::keep_elem(seed_c, (uint64_t)(((long)b * L.nblk + blk) * D + c), thresh) ? ga * dscale : 0.f;
    }
    gm += ga / (float)window_len(L, blk);
  }
  gf *= xscale;
  if (thresh) gf = esp::keep_elem(seed_x, (uint64_t)(e), thresh) ? gf * dscale : 0.f;
  dx[e] = gf + gm;
}

// thread per (b, blk, c): slot 0 <- the context slot of the block before (block 0: its own)
__global__ void __launch_bounds__(kThreads)
ctx_shift_fwd_kernel(float* __restrict__ x, int nblk, int S, int D, long total) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % D);
  const long bb = e / D;
  const int blk = (int)(bb % nblk);
  const long SD = (long)S * D;
  const long src = blk > 0 ? bb - 1 : bb;
  x[bb * SD + c] = x[src * SD + (long)(S - 1) * D + c];
}

// thread per (b, target block j, c): the slot-0 gradients that flow into j's context slot are read and zeroed by
// this thread alone (block j + 1's, and block 0's own for j = 0)
__global__ void __launch_bounds__(kThreads)
ctx_shift_bwd_kernel(float* __restrict__ d, int nblk, int S, int D, long total) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % D);
  const long bb = e / D;
  const int j = (int)(bb % nblk);
  const long SD = (long)S * D;
  float g = 0.f;
  if (j + 1 < nblk) {
    g = d[(bb + 1) * SD + c];
    d[(bb + 1) * SD + c] = 0.f;
  }
  if (j == 0) {
    g += d[bb * SD + c];
    d[bb * SD + c] = 0.f;
  }
  d[bb * SD + (long)(S - 1) * D + c] += g;
}

__global__ void __launch_bounds__(kThreads)
unchunk_fwd_kernel(const float* __restrict__ xs, float* __restrict__ y, Layout L, int D, long total) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % D);
  const long bt = e / D;
  const int t = (int)(bt % L.T);
  const long b = bt / L.T;
  int blk, slot;
  source_of(L, t, blk, slot);
  y[e] = xs[((b * L.nblk + blk) * L.S + slot) * D + c];
}

// thread per element of the chunk gradient: dy of the frame this (block, slot) is the source of, else 0
__global__ void __launch_bounds__(kThreads)
unchunk_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dxs, Layout L, int D, long total) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % D);
  const long r = e / D;
  const int s = (int)(r % L.S);
  const long bb = r / L.S;
  const int blk = (int)(bb % L.nblk);
  const long b = bb / L.nblk;
  float v = 0.f;
  const int t = blk * L.hop + s - 1;
  if (s >= 1 && s <= L.bs && t < L.T) {
    int sb, ss;
    source_of(L, t, sb, ss);
    if (sb == blk) v = dy[(b * L.T + t) * D + c];
  }
  dxs[e] = v;
}

// the layout's block count, as the reference computes it: ceil((T - past - look_ahead) / hop), past = bs - hop - la
bool make_layout(int T, int bs, int hop, int la, int nblk, Layout& L) {
  // (no cap on bs here: only esp_block_attn_* is limited to 64 slots; larger blocks run the generic attention)
  if (bs < 1 || hop < 1 || la < 0 || bs - hop - la < 0 || T <= bs) return false;
  const int n = (T - bs + hop + hop - 1) / hop;
  if (n != nblk) return false;
  L = Layout{T, bs, hop, la, nblk, bs + 2};
  return true;
}

unsigned blocks_for(long total) { return (unsigned)((total + kThreads - 1) / kThreads); }

}  // namespace

ESP_API int esp_block_attn_fwd(const float* qkv, float* ctx, float* lse, long Z, int S, int H, int dk, float drop_p,
                               unsigned long long seed, void* stream) {
  ESP_ARG_CHECK(qkv && ctx && lse, "esp_block_attn_fwd: null buffer");
  ESP_ARG_CHECK(S >= 3 && S <= kMaxS && (dk == 16 || dk == 32 || dk == 64) && H >= 1 && Z >= 1 &&
                    Z * H <= 0x7fffffffL,
                "esp_block_attn_fwd: unsupported shape S=%d dk=%d H=%d Z=%ld (3 <= S <= %d, dk 16 / 32 / 64)", S, dk, H,
                Z, kMaxS);
  ESP_ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "esp_block_attn_fwd: dropout %f outside [0, 1)", drop_p);
  ESP_ARG_CHECK(!(((uintptr_t)qkv | (uintptr_t)ctx) & 15), "esp_block_attn_fwd: qkv / ctx need 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  CBT_DISPATCH(launch_fwd, qkv, ctx, lse, Z, S, H, drop_p, (uint64_t)seed, st);
}

ESP_API int esp_block_attn_bwd(const float* qkv, const float* dctx, const float* lse, float* dqkv, long Z, int S,
                               int H, int dk, float drop_p, unsigned long long seed, void* stream) {
  ESP_ARG_CHECK(qkv && dctx && lse && dqkv, "esp_block_attn_bwd: null buffer");
  ESP_ARG_CHECK(S >= 3 && S <= kMaxS && (dk == 16 || dk == 32 || dk == 64) && H >= 1 && Z >= 1 &&
                    Z * H <= 0x7fffffffL,
                "esp_block_attn_bwd: unsupported shape S=%d dk=%d H=%d Z=%ld (3 <= S <= %d, dk 16 / 32 / 64)", S, dk, H,
                Z, kMaxS);
  ESP_ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "esp_block_attn_bwd: dropout %f outside [0, 1)", drop_p);
  ESP_ARG_CHECK(!(((uintptr_t)qkv | (uintptr_t)dctx | (uintptr_t)dqkv) & 15),
                "esp_block_attn_bwd: qkv / dctx / dqkv need 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  CBT_DISPATCH(launch_bwd, qkv, dctx, lse, dqkv, Z, S, H, drop_p, (uint64_t)seed, st);
}

ESP_API int esp_cbt_chunk_fwd(const float* x, const float* pe, int pe_rows, float* xs, int B, int T, int D, int bs,
                              int hop, int la, int nblk, float xscale, int ctx_pos_enc, float drop_p,
                              unsigned long long seed_x, unsigned long long seed_c, void* stream) {
  Layout L;
  ESP_ARG_CHECK(x && pe && xs && B >= 1 && D >= 1, "esp_cbt_chunk_fwd: bad arguments B=%d D=%d", B, D);
  ESP_ARG_CHECK(make_layout(T, bs, hop, la, nblk, L), "esp_cbt_chunk_fwd: bad layout T=%d bs=%d hop=%d la=%d nblk=%d",
                T, bs, hop, la, nblk);
  ESP_ARG_CHECK(pe_rows >= T && pe_rows >= nblk, "esp_cbt_chunk_fwd: positional table of %d rows for T=%d", pe_rows, T);
  ESP_ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "esp_cbt_chunk_fwd: dropout %f outside [0, 1)", drop_p);
  ESP_ARG_CHECK((long)B * nblk <= 0x7fffffffL, "esp_cbt_chunk_fwd: too many blocks");
  const uint32_t thresh = esp::drop_threshold(drop_p);
  hipLaunchKernelGGL(chunk_fwd_kernel, dim3((unsigned)(B * nblk)), dim3(kThreads), 0, (hipStream_t)stream, x, pe, xs, L,
                     D, xscale, ctx_pos_enc, (uint64_t)seed_x, (uint64_t)seed_c, esp::rng_key_ptr(), thresh,
                     esp::drop_scale(thresh));
  ESP_CHECK_LAUNCH("esp_cbt_chunk_fwd");
  return 0;
}

ESP_API int esp_cbt_chunk_bwd(const float* dxs, float* dx, int B, int T, int D, int bs, int hop, int la, int nblk,
                              float xscale, int ctx_pos_enc, float drop_p, unsigned long long seed_x,
                              unsigned long long seed_c, void* stream) {
  Layout L;
  ESP_ARG_CHECK(dxs && dx && B >= 1 && D >= 1, "esp_cbt_chunk_bwd: bad arguments B=%d D=%d", B, D);
  ESP_ARG_CHECK(make_layout(T, bs, hop, la, nblk, L), "esp_cbt_chunk_bwd: bad layout T=%d bs=%d hop=%d la=%d nblk=%d",
                T, bs, hop, la, nblk);
  ESP_ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "esp_cbt_chunk_bwd: dropout %f outside [0, 1)", drop_p);
  const long total = (long)B * T * D;
  ESP_ARG_CHECK(blocks_for(total) == (total + kThreads - 1) / kThreads, "esp_cbt_chunk_bwd: too many elements");
  const uint32_t thresh = esp::drop_threshold(drop_p);
  hipLaunchKernelGGL(chunk_bwd_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, dxs, dx, L, D,
                     total, xscale, ctx_pos_enc, (uint64_t)seed_x, (uint64_t)seed_c, esp::rng_key_ptr(), thresh,
                     esp::drop_scale(thresh));
  ESP_CHECK_LAUNCH("esp_cbt_chunk_bwd");
  return 0;
}

ESP_API int esp_cbt_ctx_shift_fwd(float* xs, int B, int nblk, int S, int D, void* stream) {
  ESP_ARG_CHECK(xs && B >= 1 && nblk >= 1 && S >= 3 && D >= 1, "esp_cbt_ctx_shift_fwd: bad arguments");
  const long total = (long)B * nblk * D;
  ESP_ARG_CHECK(blocks_for(total) == (total + kThreads - 1) / kThreads, "esp_cbt_ctx_shift_fwd: too many elements");
  hipLaunchKernelGGL(ctx_shift_fwd_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, xs, nblk, S,
                     D, total);
  ESP_CHECK_LAUNCH("esp_cbt_ctx_shift_fwd");
  return 0;
}

ESP_API int esp_cbt_ctx_shift_bwd(float* dxs, int B, int nblk, int S, int D, void* stream) {
  ESP_ARG_CHECK(dxs && B >= 1 && nblk >= 1 && S >= 3 && D >= 1, "esp_cbt_ctx_shift_bwd: bad arguments");
  const long total = (long)B * nblk * D;
  ESP_ARG_CHECK(blocks_for(total) == (total + kThreads - 1) / kThreads, "esp_cbt_ctx_shift_bwd: too many elements");
  hipLaunchKernelGGL(ctx_shift_bwd_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, dxs, nblk,
                     S, D, total);
  ESP_CHECK_LAUNCH("esp_cbt_ctx_shift_bwd");
  return 0;
}

ESP_API int esp_cbt_unchunk_fwd(const float* xs, float* y, int B, int T, int D, int bs, int hop, int la, int nblk,
                                void* stream) {
  Layout L;
  ESP_ARG_CHECK(xs && y && B >= 1 && D >= 1, "esp_cbt_unchunk_fwd: bad arguments B=%d D=%d", B, D);
  ESP_ARG_CHECK(make_layout(T, bs, hop, la, nblk, L), "esp_cbt_unchunk_fwd: bad layout T=%d bs=%d hop=%d la=%d nblk=%d",
                T, bs, hop, la, nblk);
  const long total = (long)B * T * D;
  ESP_ARG_CHECK(blocks_for(total) == (total + kThreads - 1) / kThreads, "esp_cbt_unchunk_fwd: too many elements");
  hipLaunchKernelGGL(unchunk_fwd_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, xs, y, L, D,
                     total);
  ESP_CHECK_LAUNCH("esp_cbt_unchunk_fwd");
  return 0;
}

ESP_API int esp_cbt_unchunk_bwd(const float* dy, float* dxs, int B, int T, int D, int bs, int hop, int la, int nblk,
                                void* stream) {
  Layout L;
  ESP_ARG_CHECK(dy && dxs && B >= 1 && D >= 1, "esp_cbt_unchunk_bwd: bad arguments B=%d D=%d", B, D);
  ESP_ARG_CHECK(make_layout(T, bs, hop, la, nblk, L), "esp_cbt_unchunk_bwd: bad layout T=%d bs=%d hop=%d la=%d nblk=%d",
                T, bs, hop, la, nblk);
  const long total = (long)B * nblk * L.S * D;
  ESP_ARG_CHECK(blocks_for(total) == (total + kThreads - 1) / kThreads, "esp_cbt_unchunk_bwd: too many elements");
  hipLaunchKernelGGL(unchunk_bwd_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, dy, dxs, L, D,
                     total);
  ESP_CHECK_LAUNCH("esp_cbt_unchunk_bwd");
  return 0;
}
