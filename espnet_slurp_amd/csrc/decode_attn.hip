// Single-query attention for the cached decoder step (beam search inference; the reference computes the
// same thing through MultiHeadedAttention on a one-row query, transformer/attention.py:55-114, from
// TransformerDecoder.forward_one_step, espnet2/asr/decoder/transformer_decoder.py:147-190).
//
//   out[n, h] = softmax(q[n, h] . K[src[n], :klen[n], h] / sqrt(d_k)) . V[src[n], :klen[n], h]
//
// N decode rows, one query vector each.  Self-attention: src[n] = n, klen = the prefix length, K / V the
// row's cached prefix.  Source attention: src[n] = the row's utterance, klen = that utterance's encoder
// length, K / V the utterance's projected memory (many rows share one src).
//
// Layout of the work: one wave per (row, head), four waves to a block.  A lane owns one key of each
// 64-key chunk: it reads that key's d_k floats (float4 loads; a lane reads whole 64 / 128 / 256-byte
// runs), forms the score, and the wave reduces the chunk's maximum (online softmax: running maximum m,
// per-lane partial denominators l and per-lane partial outputs acc[d_k], all rescaled by the wave-uniform
// exp(m_old - m_new)).  The lane then reads its key's V row and adds p * V.  After the last chunk l and
// the d_k accumulators are summed across the wave once.  Keys at or beyond klen[n] are never read: their
// lanes skip both loads and carry p = 0.  All arithmetic is fp32.
// Rows with the same src read the same K / V bytes; this version leaves that sharing to the L2 (the
// rows arrive sorted by utterance, so the waves of one utterance run close together in time).
//
// esp_decode_attn_masked (the Transformer LM step) is the same kernel with a per-row key-validity byte mask
// (N, Tk): key j of row n takes part when j < klen[n] and mask[n, j] != 0 (the reference LM hides every key
// whose token id is 0, espnet2/lm/transformer_lm.py _target_mask).  A masked lane behaves as a lane beyond klen:
// no load, score -inf, p = 0.  A chunk whose 64 keys are all masked while no key has been seen yet (m = -inf)
// is skipped before exp(m - mn) could form exp(-inf - -inf); once a key has been seen m is finite and an
// all-masked chunk rescales by exp(0) = 1.  Contract: at least one valid key per row.  With an all-ones mask
// the arithmetic is that of the unmasked kernel, operation for operation.
#include "common.h"

namespace {

constexpr int kDecodeChunk = 64;  // keys per online-softmax step: one per lane

template <int DK, bool MASKED>
__global__ void __launch_bounds__(256)
decode_attn_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ k, long ldk, long sk,
                   const float* __restrict__ v, long ldv, long sv, float* __restrict__ out, long ldo,
                   const int* __restrict__ src, const int* __restrict__ klen, int N, int H, float inv_sqrt_dk,
                   const unsigned char* __restrict__ mask, long ldm) {
  const int lane = threadIdx.x & 63;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)N * H) return;  // wave-uniform
  const int n = (int)(item / H), h = (int)(item - (long)n * H);
  const int s = src[n], len = klen[n];
  float qr[DK];
  {
    const float4* qp = reinterpret_cast<const float4*>(q + (long)n * ldq + (long)h * DK);
#pragma unroll
    for (int d = 0; d < DK / 4; ++d) {
      const float4 t = qp[d];
      qr[4 * d] = t.x, qr[4 * d + 1] = t.y, qr[4 * d + 2] = t.z, qr[4 * d + 3] = t.w;
    }
  }
  const float* kp = k + (long)s * sk + (long)h * DK;
  const float* vp = v + (long)s * sv + (long)h * DK;
  float m = -INFINITY, l = 0.f;
  float acc[DK];
#pragma unroll
  for (int d = 0; d < DK; ++d) acc[d] = 0.f;
  for (int j0 = 0; j0 < len; j0 += kDecodeChunk) {
    const int j = j0 + lane;
    bool live = j < len;
    if constexpr (MASKED) live = live && mask[(long)n * ldm + j] != 0;
    float sc = -INFINITY;
    if (live) {
      const float4* kr = reinterpret_cast<const float4*>(kp + (long)j * ldk);
      float dot = 0.f;
#pragma unroll
      for (int d = 0; d < DK / 4; ++d) {
        const float4 t = kr[d];
        dot = fmaf(qr[4 * d], t.x, dot);
        dot = fmaf(qr[4 * d + 1], t.y, dot);
        dot = fmaf(qr[4 * d + 2], t.z, dot);
        dot = fmaf(qr[4 * d + 3], t.w, dot);
      }
      sc = dot * inv_sqrt_dk;
    }
    // unmasked: lane 0 of every chunk is live (j0 < len), so mn is finite; exp(-inf) = 0 on the first chunk
    const float mn = fmaxf(m, esp::wave_max(sc));
    if constexpr (MASKED) {
      if (mn == -INFINITY) continue;  // wave-uniform: nothing valid yet, l and acc are still 0
    }
    const float a = __expf(m - mn);
    const float p = live ? __expf(sc - mn) : 0.f;
    l = l * a + p;
    if (live) {
      const float4* vr = reinterpret_cast<const float4*>(vp + (long)j * ldv);
#pragma unroll
      for (int d = 0; d < DK / 4; ++d) {
        const float4 t = vr[d];
        acc[4 * d] = fmaf(p, t.x, acc[4 * d] * a);
        acc[4 * d + 1] = fmaf(p, t.y, acc[4 * d + 1] * a);
        acc[4 * d + 2] = fmaf(p, t.z, acc[4 * d + 2] * a);
        acc[4 * d + 3] = fmaf(p, t.w, acc[4 * d + 3] * a);
      }
    } else {
#pragma unroll
      for (int d = 0; d < DK; ++d) acc[d] *= a;
    }
    m = mn;
  }
  const float inv_l = 1.f / esp::wave_sum(l);
  float o = 0.f;  // lane d keeps column d
#pragma unroll
  for (int d = 0; d < DK; ++d) {
    const float t = esp::wave_sum(acc[d]);
    if (lane == d) o = t;
  }
  if (lane < DK) out[(long)n * ldo + (long)h * DK + lane] = o * inv_l;
}

}  // namespace

static int decode_attn_launch(const char* name, const float* q, long ldq, long qoff, const float* k, long ldk, long sk,
                              long koff, const float* v, long ldv, long sv, long voff, float* out, long ldo, long ooff,
                              const int* idx_host, const int* idx_dev, const unsigned char* mask, long ldm, int N, int H,
                              int dk, int nsrc, int Tk, void* stream) {
  ESP_ARG_CHECK(dk == 16 || dk == 32 || dk == 64, "%s: d_k %d not supported (16, 32, 64)", name, dk);
  ESP_ARG_CHECK(N >= 1 && H >= 1 && nsrc >= 1 && Tk >= 1 && (long)N * H < (1L << 31),
                "%s: bad sizes N=%d H=%d nsrc=%d Tk=%d", name, N, H, nsrc, Tk);
  ESP_ARG_CHECK(q && k && v && out && idx_host && idx_dev, "%s: null argument", name);
  const long w = (long)H * dk;
  ESP_ARG_CHECK(qoff >= 0 && koff >= 0 && voff >= 0 && ooff >= 0 && ldq >= qoff + w && ldk >= koff + w &&
                    ldv >= voff + w && ldo >= ooff + w,
                "%s: a row (offset + H*d_k) does not fit its leading dimension", name);
  ESP_ARG_CHECK(sk >= 0 && sv >= 0 && (nsrc == 1 || (sk >= (long)Tk * ldk && sv >= (long)Tk * ldv)),
                "%s: source stride smaller than Tk rows", name);
  ESP_ARG_CHECK(!((ldq | qoff | ldk | sk | koff | ldv | sv | voff) & 3) &&
                    !(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15),
                "%s: q / K / V need 16-byte aligned rows (pointers, strides and offsets %% 4 floats)", name);
  int maxlen = 0;
  for (int n = 0; n < N; ++n) {
    const int s = idx_host[n], len = idx_host[N + n];
    ESP_ARG_CHECK(s >= 0 && s < nsrc, "%s: src[%d] = %d outside [0, %d)", name, n, s, nsrc);
    ESP_ARG_CHECK(len >= 1 && len <= Tk, "%s: klen[%d] = %d outside [1, %d]", name, n, len, Tk);
    maxlen = len > maxlen ? len : maxlen;
  }
  ESP_ARG_CHECK(!mask || ldm >= maxlen, "%s: mask row pitch %ld smaller than the longest klen %d", name, ldm, maxlen);
  const float inv = 1.0f / sqrtf((float)dk);
  const dim3 grid((unsigned)(((long)N * H + 3) / 4)), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define ESP_DECODE_ATTN_LAUNCH(DK, MASKED)                                                                        \
  hipLaunchKernelGGL((decode_attn_kernel<DK, MASKED>), grid, block, 0, st, q + qoff, ldq, k + koff, ldk, sk, v + voff, \
                     ldv, sv, out + ooff, ldo, idx_dev, idx_dev + N, N, H, inv, mask, ldm)
  if (mask) {
    if (dk == 16) ESP_DECODE_ATTN_LAUNCH(16, true);
    else if (dk == 32) ESP_DECODE_ATTN_LAUNCH(32, true);
    else ESP_DECODE_ATTN_LAUNCH(64, true);
  } else {
    if (dk == 16) ESP_DECODE_ATTN_LAUNCH(16, false);
    else if (dk == 32) ESP_DECODE_ATTN_LAUNCH(32, false);
    else ESP_DECODE_ATTN_LAUNCH(64, false);
  }
#undef ESP_DECODE_ATTN_LAUNCH
  ESP_CHECK_LAUNCH(name);
  return 0;
}

ESP_API int esp_decode_attn(const float* q, long ldq, long qoff, const float* k, long ldk, long sk, long koff,
                            const float* v, long ldv, long sv, long voff, float* out, long ldo, long ooff,
                            const int* idx_host, const int* idx_dev, int N, int H, int dk, int nsrc, int Tk,
                            void* stream) {
  return decode_attn_launch("esp_decode_attn", q, ldq, qoff, k, ldk, sk, koff, v, ldv, sv, voff, out, ldo, ooff,
                            idx_host, idx_dev, nullptr, 0, N, H, dk, nsrc, Tk, stream);
}

ESP_API int esp_decode_attn_masked(const float* q, long ldq, long qoff, const float* k, long ldk, long sk, long koff,
                                   const float* v, long ldv, long sv, long voff, float* out, long ldo, long ooff,
                                   const int* idx_host, const int* idx_dev, const unsigned char* mask, long ldm, int N,
                                   int H, int dk, int nsrc, int Tk, void* stream) {
  ESP_ARG_CHECK(mask, "esp_decode_attn_masked: null mask");
  return decode_attn_launch("esp_decode_attn_masked", q, ldq, qoff, k, ldk, sk, koff, v, ldv, sv, voff, out, ldo, ooff,
                            idx_host, idx_dev, mask, ldm, N, H, dk, nsrc, Tk, stream);
}

// Row gather of the self-attention K/V cache into a second buffer (DecoderCache.reorder_keep: the parent selection
// of a beam search that may roll one step back, so the source rows must survive):
//   dst[l, i, p, :] = src[l, index[i], p, :]   for l < NL, i < n, p < len
// src (NL, src_R, src_C, W), dst (NL, dst_R, dst_C, W) fp32, W floats per position (K | V), one launch for all
// layers.  A thread moves one float4; index (device int64) may repeat; an entry outside [0, src_n) is skipped (its
// destination row is left as it was), so nothing outside the two buffers is touched whatever the index holds.
namespace {
__global__ void __launch_bounds__(256)
cache_gather_kernel(const float* __restrict__ src, float* __restrict__ dst, const long long* __restrict__ index, int NL,
                    int n, int len, int W4, int src_n, long src_R, long src_C, long dst_R, long dst_C) {
  const long per_row = (long)len * W4;  // float4s per (layer, row): positions [0, len) are contiguous
  const long total = (long)NL * n * per_row;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long row = e / per_row, off = e - row * per_row;
    const int l = (int)(row / n), i = (int)(row - (long)l * n);
    const long long s = index[i];
    if (s < 0 || s >= src_n) continue;
    const float4* sp = reinterpret_cast<const float4*>(src) + ((long)l * src_R + s) * src_C * W4 + off;
    float4* dp = reinterpret_cast<float4*>(dst) + ((long)l * dst_R + i) * dst_C * W4 + off;
    *dp = *sp;
  }
}
}  // namespace

ESP_API int esp_cache_gather(const float* src, float* dst, const long long* index, int NL, int n, int len, int W,
                             int src_n, int src_R, int src_C, int dst_R, int dst_C, void* stream) {
  ESP_ARG_CHECK(NL >= 1 && n >= 1 && len >= 0 && W >= 4 && !(W & 3) && src_n >= 1 && src_n <= src_R && n <= dst_R &&
                    len <= src_C && len <= dst_C,
                "esp_cache_gather: bad sizes NL=%d n=%d len=%d W=%d src %d of %d x %d dst %d x %d", NL, n, len, W, src_n,
                src_R, src_C, dst_R, dst_C);
  ESP_ARG_CHECK(src && dst && index && src != dst && !(((uintptr_t)src | (uintptr_t)dst) & 15),
                "esp_cache_gather: buffers must be distinct, non-null and 16-byte aligned");
  if (len == 0) return 0;
  const long total = (long)NL * n * len * (W / 4);
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(cache_gather_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     (hipStream_t)stream, src, dst, index, NL, n, len, W / 4, src_n, (long)src_R, (long)src_C,
                     (long)dst_R, (long)dst_C);
  ESP_CHECK_LAUNCH("esp_cache_gather");
  return 0;
}
