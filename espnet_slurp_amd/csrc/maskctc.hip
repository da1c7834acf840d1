// Mask-CTC mask-predict decoding on the device (espnet2/asr/maskctc_model.py MaskCTCInference.forward):
//   esp_maskctc_init  greedy CTC -> collapsed tokens, their confidences, the masked decoder input (:288-317)
//   esp_maskctc_fill  one refinement step on the decoder's logits (:327-331, :336-337)
//   esp_maskctc_init_batch / esp_maskctc_fill_batch  the same device bodies for U ragged utterances, grid = U, with
//                     the per-utterance pass plan (num_iter, k: :319-323) kept on the device
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

// esp_maskctc_init's work for one utterance, by the whole block: returns L, nmask_total the masked tokens (both
// block-uniform)
__device__ __forceinline__ int maskctc_init_body(const float* __restrict__ lp, int T, int V, int blank,
                                                 long long mask_token, double thr, int* __restrict__ fid,
                                                 float* __restrict__ flp, long long* __restrict__ y_in,
                                                 float* __restrict__ tok_logp, float* __restrict__ tok_prob, int* sh,
                                                 int& nmask_total) {
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
  block_excl_scan(nmask, sh, nmask_total);
  return base;
}

__global__ __launch_bounds__(MC_NT) void maskctc_init_kernel(const float* __restrict__ lp, int T, int V, int blank,
                                                            long long mask_token, double thr, int* __restrict__ fid,
                                                            float* __restrict__ flp, long long* __restrict__ y_in,
                                                            float* __restrict__ tok_logp, float* __restrict__ tok_prob,
                                                            int* __restrict__ counts) {
  __shared__ int sh[MC_NT / 64];
  int nmask;
  const int L = maskctc_init_body(lp, T, V, blank, mask_token, thr, fid, flp, y_in, tok_logp, tok_prob, sh, nmask);
  if (threadIdx.x == 0) {
    counts[0] = L;
    counts[1] = nmask;
  }
}

// one workgroup per utterance: frames [0, tlens[u]) of its (Tmax, V) block, the pass plan into counts[u]
__global__ __launch_bounds__(MC_NT) void maskctc_init_batch_kernel(
    const float* __restrict__ lp, const int* __restrict__ tlens, int Tmax, int V, int blank, long long mask_token,
    double thr, int n_iterations, int* __restrict__ fid, float* __restrict__ flp, long long* __restrict__ y_in,
    float* __restrict__ tok_logp, float* __restrict__ tok_prob, int* __restrict__ counts) {
  __shared__ int sh[MC_NT / 64];
  const int u = blockIdx.x;
  const long o = (long)u * Tmax;
  const int T = min(max(tlens[u], 0), Tmax);
  int nmask;
  const int L = maskctc_init_body(lp + o * V, T, V, blank, mask_token, thr, fid + o, flp + o, y_in + o, tok_logp + o,
                                  tok_prob + o, sh, nmask);
  for (int i = L + threadIdx.x; i < Tmax; i += MC_NT) y_in[o + i] = 0;
  if (threadIdx.x == 0) {
    const int num_iter = (nmask >= n_iterations && n_iterations > 0) ? n_iterations : nmask;
    counts[4 * u + 0] = L;
    counts[4 * u + 1] = nmask;
    counts[4 * u + 2] = num_iter;
    counts[4 * u + 3] = num_iter > 0 ? nmask / num_iter : 0;
  }
}

// esp_maskctc_fill's work for one utterance, by the whole block; score / arg: MC_FILL_MAXL entries of LDS each
__device__ __forceinline__ void maskctc_fill_body(const float* __restrict__ logits, int L, int V1,
                                                  long long* __restrict__ y_in, long long mask_token, int k,
                                                  float* score, int* arg /* -1: the position is not masked */) {
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

__global__ __launch_bounds__(MC_NT) void maskctc_fill_kernel(const float* __restrict__ logits, int L, int V1,
                                                            long long* __restrict__ y_in, long long mask_token, int k) {
  __shared__ float score[MC_FILL_MAXL];
  __shared__ int arg[MC_FILL_MAXL];
  maskctc_fill_body(logits, L, V1, y_in, mask_token, k, score, arg);
}

// workgroup a: pass t of utterance rows[a] on logits block a, by that utterance's plan counts[u] = {L, mask_num,
// num_iter, k}.  The skip follows the plan, not the masks: a position filled with <mask> by the last pass stays.
__global__ __launch_bounds__(MC_NT) void maskctc_fill_batch_kernel(const float* __restrict__ logits, int Lmax, int V1,
                                                                  long long* __restrict__ y_in, int ld,
                                                                  const int* __restrict__ counts,
                                                                  const int* __restrict__ rows, int U,
                                                                  long long mask_token, int t) {
  __shared__ float score[MC_FILL_MAXL];
  __shared__ int arg[MC_FILL_MAXL];
  const int a = blockIdx.x, u = rows[a];
  if (u < 0 || u >= U) return;  // block-uniform, as every return below
  const int L = min(max(counts[4 * u], 0), Lmax), num_iter = counts[4 * u + 2];
  if (t >= num_iter) return;
  const int k = t < num_iter - 1 ? counts[4 * u + 3] : 0;
  if (t < num_iter - 1 && k <= 0) return;  // not a plan esp_maskctc_init_batch writes (k >= 1 there)
  maskctc_fill_body(logits + (long)a * Lmax * V1, L, V1, y_in + (long)u * ld, mask_token, k, score, arg);
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

ESP_API int esp_maskctc_init_batch(const float* lp, const int* tlens, int U, int Tmax, int V, int blank,
                                   long long mask_token, double threshold, int n_iterations, int* fid, float* flp,
                                   long long* y_in, float* tok_logp, float* tok_prob, int* counts, void* stream) {
  ESP_ARG_CHECK(U >= 1 && Tmax >= 1 && V >= 1 && blank >= 0 && blank < V && n_iterations >= 0,
                "esp_maskctc_init_batch: bad sizes U=%d Tmax=%d V=%d blank=%d n_iterations=%d", U, Tmax, V, blank,
                n_iterations);
  hipLaunchKernelGGL(maskctc_init_batch_kernel, dim3(U), dim3(MC_NT), 0, (hipStream_t)stream, lp, tlens, Tmax, V, blank,
                     mask_token, threshold, n_iterations, fid, flp, y_in, tok_logp, tok_prob, counts);
  ESP_CHECK_LAUNCH("esp_maskctc_init_batch");
  return 0;
}

ESP_API int esp_maskctc_fill_batch(const float* logits, int Ua, int Lmax, int V1, long long* y_in, int ld,
                                   const int* counts, const int* rows, int U, long long mask_token, int t,
                                   void* stream) {
  ESP_ARG_CHECK(Ua >= 1 && U >= 1 && Lmax >= 1 && Lmax <= MC_FILL_MAXL && V1 >= 1 && ld >= Lmax && t >= 0,
                "esp_maskctc_fill_batch: bad sizes Ua=%d U=%d Lmax=%d (max %d) V1=%d ld=%d t=%d", Ua, U, Lmax,
                MC_FILL_MAXL, V1, ld, t);
  hipLaunchKernelGGL(maskctc_fill_batch_kernel, dim3(Ua), dim3(MC_NT), 0, (hipStream_t)stream, logits, Lmax, V1, y_in,
                     ld, counts, rows, U, mask_token, t);
  ESP_CHECK_LAUNCH("esp_maskctc_fill_batch");
  return 0;
}
