// Mask-CTC mask-predict decoding on the device (espnet2/asr/maskctc_model.py MaskCTCInference.forward):
//   esp_maskctc_init  greedy CTC -> collapsed tokens, their confidences, the masked decoder input (:288-317)
//   esp_maskctc_fill  one refinement step on the decoder's logits (:327-331, :336-337)
// One workgroup per utterance, 4 waves; selection only (max / argmax / rank), so every id and every selected
// value is reproducible bit for bit.  Plain C++ and vector stores, wave64 shuffles, no atomics.
#include "common.h"

namespace {

constexpr int MC_NT = 256;         // threads per block (4 waves)
constexpr int MC_FILL_MAXL = 2048;  // positions esp_maskctc_fill ranks in LDS

// (max, first index of it) over a row, one wave; NaN never wins (the inputs are log-probabilities / logits)
__device__ __forceinline__ void wave_argmax(const float* __restrict__ row, int n, float& m, int& am) {
  const int lane = threadIdx.x & 63;
  m = -INFINITY;
  am = 0x7fffffff;
  for (int c = lane; c < n; c += 64) {
    const float v = row[c];
    if (v > m || (v == m && c < am)) { m = v; am = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
  if (am == 0x7fffffff) am = 0;  // a row of -inf / NaN only
}

// exclusive prefix sum of one int per thread over the block (MC_NT threads); total: the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* sh /* >= MC_NT / 64 */, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  __syncthreads();  // sh may still be read from the previous call
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < MC_NT / 64; ++i) {
    if (i < w) base += sh[i];
    total += sh[i];
  }
  return base + incl - v;
}

__global__ __launch_bounds__(MC_NT) void maskctc_init_kernel(const float* __restrict__ lp, int T, int V, int blank,
                                                            long long mask_token, double thr, int* __restrict__ fid,
                                                            float* __restrict__ flp, long long* __restrict__ y_in,
                                                            float* __restrict__ tok_logp, float* __restrict__ tok_prob,
                                                            int* __restrict__ counts) {
  __shared__ int sh[MC_NT / 64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // 1. per-frame argmax of the log-probabilities (exp is monotone: the argmax of the probabilities)
  for (int t = w; t < T; t += MC_NT / 64) {
    float m;
    int am;
    wave_argmax(lp + (long)t * V, V, m, am);
    if (lane == 0) {
      fid[t] = am;
      flp[t] = m;
    }
  }
  __threadfence_block();
  __syncthreads();
  // 2. run starts, compaction of the non-blank runs, each run's maximum, the threshold
  int base = 0, nmask = 0;
  for (int t0 = 0; t0 < T; t0 += MC_NT) {
    const int t = t0 + threadIdx.x;
    int id = blank, flag = 0;
    if (t < T) {
      id = fid[t];
      flag = (id != blank) && (t == 0 || fid[t - 1] != id);
    }
    int total;
    const int pos = base + block_excl_scan(flag, sh, total);
    if (flag) {
      float m = flp[t];
      for (int u = t + 1; u < T && fid[u] == id; ++u) m = fmaxf(m, flp[u]);
      const float p = expf(m);
      const bool masked = (double)p < thr;
      y_in[pos] = masked ? mask_token : (long long)id;
      tok_logp[pos] = m;
      tok_prob[pos] = p;
      nmask += masked ? 1 : 0;
    }
    base += total;
  }
  int total;
  block_excl_scan(nmask, sh, total);
  if (threadIdx.x == 0) {
    counts[0] = base;
    counts[1] = total;
  }
}

__global__ __launch_bounds__(MC_NT) void maskctc_fill_kernel(const float* __restrict__ logits, int L, int V1,
                                                            long long* __restrict__ y_in, long long mask_token, int k) {
  __shared__ float score[MC_FILL_MAXL];
  __shared__ int arg[MC_FILL_MAXL];  // -1: the position is not masked
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = w; i < L; i += MC_NT / 64) {
    const bool masked = y_in[i] == mask_token;  // wave-uniform
    float m = -INFINITY;
    int am = -1;
    if (masked) wave_argmax(logits + (long)i * V1, V1, m, am);
    if (lane == 0) {
      score[i] = m;
      arg[i] = am;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < L; i += MC_NT) {
    if (arg[i] < 0) continue;
    bool fill = true;
    if (k > 0) {  // rank among the masked positions by counting; the lower index wins a tie
      const float s = score[i];
      int rank = 0;
      for (int j = 0; j < L; ++j) rank += (arg[j] >= 0 && (score[j] > s || (score[j] == s && j < i))) ? 1 : 0;
      fill = rank < k;
    }
    if (fill) y_in[i] = (long long)arg[i];
  }
}

}  // namespace

ESP_API int esp_maskctc_init(const float* lp, int T, int V, int blank, long long mask_token, double threshold, int* fid,
                             float* flp, long long* y_in, float* tok_logp, float* tok_prob, int* counts, void* stream) {
  ESP_ARG_CHECK(T >= 1 && V >= 1 && blank >= 0 && blank < V, "esp_maskctc_init: bad sizes T=%d V=%d blank=%d", T, V,
                blank);
  hipLaunchKernelGGL(maskctc_init_kernel, dim3(1), dim3(MC_NT), 0, (hipStream_t)stream, lp, T, V, blank, mask_token,
                     threshold, fid, flp, y_in, tok_logp, tok_prob, counts);
  ESP_CHECK_LAUNCH("esp_maskctc_init");
  return 0;
}

ESP_API int esp_maskctc_fill(const float* logits, int L, int V1, long long* y_in, long long mask_token, int k,
                             void* stream) {
  ESP_ARG_CHECK(L >= 1 && L <= MC_FILL_MAXL && V1 >= 1 && k >= 0, "esp_maskctc_fill: bad sizes L=%d (max %d) V1=%d k=%d",
                L, MC_FILL_MAXL, V1, k);
  hipLaunchKernelGGL(maskctc_fill_kernel, dim3(1), dim3(MC_NT), 0, (hipStream_t)stream, logits, L, V1, y_in, mask_token,
                     k);
  ESP_CHECK_LAUNCH("esp_maskctc_fill");
  return 0;
}
