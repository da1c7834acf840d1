// Decode-row kernels of the Transformer LM step (shallow fusion; the reference runs the same arithmetic through
// espnet/nets/pytorch_backend/transformer/encoder.py forward_one_step from espnet2/lm/transformer_lm.py batch_score).
//
// esp_step_linear: out[n, :] = act(LN?(x[n, :]) . W^T + b) (+ R[n, :]) for a handful of decode rows n.
// The shape is skinny (N rows against a (M, K) weight), so the time is the one pass over W, not the FMAs: the
// kernel streams W from HBM once per tile of 8 rows and keeps that tile's (normalised) x rows in LDS.
//   block  = 4 waves; a wave owns 4 output columns, the block 16; grid = (ceil(M / 16), ceil(N / 8)).
//   k loop = lane l of a wave reads floats [k0 + 4l, k0 + 4l + 4) of its 4 weight rows (one float4 each, a wave
//            reads a whole 1 KiB run of every row) and of the 8 x rows from LDS (consecutive lanes, consecutive
//            16 bytes: no bank conflict), 128 FMAs; k0 advances by 256.
//   reduce = every lane holds 32 partial sums (4 columns x 8 rows) to be added across the 64 lanes.  Instead of
//            32 butterflies (192 shuffles) the sums are halved five times: at step s a lane keeps the even or
//            the odd slot of every pair (by one bit of its lane id), sends the other to the partner lane, and
//            adds what it receives (16 + 8 + 4 + 2 + 1 = 31 shuffles); a last plain exchange adds the two lanes
//            that end with the same slot.  Lane l (even) ends with the total of slot
//            j = b5 + 2 b4 + 4 b3 + 8 b2 + 16 b1 (b_i = bit i of l), column j / 8, row j % 8, and stores it.
//   LN     = the optional LayerNorm prologue normalises the tile's rows in LDS (two passes over the row held in
//            LDS: mean, then the centred sum of squares), each block for itself: the rows are a few KiB and
//            come from L2, against the 16 weight rows the block then streams.
//   store  = columns [0, c0) go to the dense `out` (row pitch ldo), columns [c0, M) to a second buffer at
//            out2 + n * row_stride2 + pos * (M - c0): with out2 = a DecoderCache layer and c0 = att_unit the
//            q | k | v projection writes q densely and K | V straight to position `pos` of every row's cache.
// All arithmetic is fp32 FMA.  K % 4 == 0, K <= 2048 (the LDS tile: 8 rows x 2048 floats = 64 KiB).
//
// esp_step_ln_act: y[r, :] = relu(LN(x[r, :])) * xscale + pe[pos0 + r % L, :] -- the tail of the LM's input layer
// (Linear -> torch.nn.LayerNorm -> ReLU -> positional step; pe NULL: the identity positional step).  A wave per row.
//
// esp_lm_front_fwd / _bwd: the same tail in training form (espnet1 encoder.py input_layer "linear": LayerNorm ->
// Dropout -> ReLU -> pos_enc_class, whose PositionalEncoding ends in a second Dropout): y = drop2(relu(drop1(LN(x)))
// * xscale + pe[r % L]); pe NULL: y = relu(drop1(LN(x))).  The masks come from the counter RNG by element index
// r*D + c, so they do not depend on the launch geometry and the backward regenerates them from the same seeds; the
// forward saves the row mean / rstd, the backward recomputes the ReLU decision from them and hands the gradient of
// LN(x) to esp_layernorm_bwd.  At p1 = 0 the forward's values are esp_step_ln_act's bit for bit.
#include "common.h"

namespace {

constexpr int kRT = 8;     // rows per tile
constexpr int kCPW = 4;    // columns per wave
constexpr int kCPB = 16;   // columns per block (4 waves)
constexpr int kMaxK = 2048;

__global__ void __launch_bounds__(256)
step_linear_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ W, long ldw,
                   const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ beta,
                   float eps, int relu, const float* __restrict__ R, long ldr, float* __restrict__ out, long ldo,
                   int c0, float* __restrict__ out2, long row_stride2, long off2, int N, int K, int M) {
  extern __shared__ float4 xs4[];  // kRT rows of K floats
  float* xs = reinterpret_cast<float*>(xs4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.y * kRT;
  const int K4 = K >> 2;
  // the tile's x rows -> LDS (rows beyond N: zeros)
  for (int i = threadIdx.x; i < kRT * K4; i += 256) {
    const int r = i / K4, c = i - r * K4;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n0 + r < N) t = reinterpret_cast<const float4*>(x + (long)(n0 + r) * ldx)[c];
    xs4[i] = t;
  }
  __syncthreads();
  if (gamma) {
    for (int r = wave; r < kRT; r += 4) {
      if (n0 + r >= N) continue;  // wave-uniform
      float* row = xs + r * K;
      float s = 0.f;
      for (int c = lane; c < K; c += 64) s += row[c];
      const float mean = esp::wave_sum(s) / (float)K;
      float q = 0.f;
      for (int c = lane; c < K; c += 64) {
        const float d = row[c] - mean;
        q = fmaf(d, d, q);
      }
      const float rstd = 1.0f / sqrtf(esp::wave_sum(q) / (float)K + eps);
      for (int c = lane; c < K; c += 64) row[c] = fmaf((row[c] - mean) * rstd, gamma[c], beta[c]);
    }
    __syncthreads();
  }
  const int m0 = blockIdx.x * kCPB + wave * kCPW;
  if (m0 >= M) return;  // wave-uniform, after the last barrier
  const float4* wr[kCPW];
#pragma unroll
  for (int c = 0; c < kCPW; ++c) {
    const int m = m0 + c < M ? m0 + c : M - 1;  // columns beyond M read a valid row and are not stored
    wr[c] = reinterpret_cast<const float4*>(W + (long)m * ldw);
  }
  float acc[kCPW * kRT];
#pragma unroll
  for (int j = 0; j < kCPW * kRT; ++j) acc[j] = 0.f;
  for (int k4 = lane; k4 < K4; k4 += 64) {
    float4 w[kCPW];
#pragma unroll
    for (int c = 0; c < kCPW; ++c) w[c] = wr[c][k4];
#pragma unroll
    for (int r = 0; r < kRT; ++r) {
      const float4 xv = xs4[r * K4 + k4];
#pragma unroll
      for (int c = 0; c < kCPW; ++c) {
        float a = acc[c * kRT + r];
        a = fmaf(w[c].x, xv.x, a);
        a = fmaf(w[c].y, xv.y, a);
        a = fmaf(w[c].z, xv.z, a);
        a = fmaf(w[c].w, xv.w, a);
        acc[c * kRT + r] = a;
      }
    }
  }
  // 32 sums across 64 lanes: halve the slots five times (lane bits 5..1), then add the lane pair
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int off = 32 >> s;
    const bool up = (lane & off) != 0;
    const int cnt = (kCPW * kRT) >> (s + 1);
#pragma unroll
    for (int i = 0; i < cnt; ++i) {
      const float keep = up ? acc[2 * i + 1] : acc[2 * i];
      const float send = up ? acc[2 * i] : acc[2 * i + 1];
      acc[i] = keep + __shfl_xor(send, off, 64);
    }
  }
  const float total = acc[0] + __shfl_xor(acc[0], 1, 64);
  if (lane & 1) return;
  const int j = ((lane >> 5) & 1) | (((lane >> 4) & 1) << 1) | (((lane >> 3) & 1) << 2) | (((lane >> 2) & 1) << 3) |
                (((lane >> 1) & 1) << 4);
  const int m = m0 + j / kRT, n = n0 + j % kRT;
  if (m >= M || n >= N) return;
  float v = total;
  if (bias) v += bias[m];
  if (relu) v = fmaxf(v, 0.f);
  if (R) v += R[(long)n * ldr + m];
  if (m < c0) out[(long)n * ldo + m] = v;
  else out2[(long)n * row_stride2 + off2 + (m - c0)] = v;
}

__global__ void __launch_bounds__(256)
step_ln_act_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                   float eps, float xscale, const float* __restrict__ pe, int L, int pos0, float* __restrict__ y,
                   int rows, int D) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // wave-uniform
  const float* xr = x + r * D;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) s += xr[c];
  const float mean = esp::wave_sum(s) / (float)D;
  float q = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float d = xr[c] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(esp::wave_sum(q) / (float)D + eps);
  const float* per = pe ? pe + (long)(pos0 + (int)(r % L)) * D : nullptr;
  for (int c = lane; c < D; c += 64) {
    float v = fmaxf(fmaf((xr[c] - mean) * rstd, gamma[c], beta[c]), 0.f);
    if (per) v = fmaf(v, xscale, per[c]);
    y[r * D + c] = v;
  }
}

// the front's pre-activation t = drop1(LN(x)) of one element; relu(t) > 0 iff the element is kept and LN(x) > 0
__device__ __forceinline__ float front_pre(float x, float mean, float rstd, float gamma, float beta, uint64_t seed1,
                                           uint32_t th1, float ds1, uint64_t idx) {
  float t = fmaf((x - mean) * rstd, gamma, beta);
  if (th1) t = esp::keep_elem(seed1, idx, th1) ? t * ds1 : 0.f;
  return t;
}

// step_ln_act_kernel's arithmetic with the two dropouts of the training form and the saved row statistics
__global__ void __launch_bounds__(256)
lm_front_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                    float eps, float xscale, const float* __restrict__ pe, int L, float* __restrict__ y,
                    float* __restrict__ mean_out, float* __restrict__ rstd_out, int rows, int D, uint64_t seed1,
                    uint64_t seed2, const uint64_t* __restrict__ key, uint32_t th1, float ds1, uint32_t th2,
                    float ds2) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // wave-uniform
  seed1 = esp::keyed(seed1, key);
  seed2 = esp::keyed(seed2, key);
  const float* xr = x + r * D;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) s += xr[c];
  const float mean = esp::wave_sum(s) / (float)D;
  float q = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float d = xr[c] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(esp::wave_sum(q) / (float)D + eps);
  if (lane == 0) {
    mean_out[r] = mean;
    rstd_out[r] = rstd;
  }
  const float* per = pe ? pe + (long)(r % L) * D : nullptr;
  for (int c = lane; c < D; c += 64) {
    const uint64_t idx = (uint64_t)(r * D + c);
    float v = fmaxf(front_pre(xr[c], mean, rstd, gamma[c], beta[c], seed1, th1, ds1, idx), 0.f);
    if (per) {
      v = fmaf(v, xscale, per[c]);
      if (th2) v = esp::keep_elem(seed2, idx, th2) ? v * ds2 : 0.f;
    }
    y[r * D + c] = v;
  }
}

// dz = gradient with respect to LN(x): the second dropout, the scale, the ReLU decision recomputed from the saved
// statistics, the first dropout; esp_layernorm_bwd takes it from there
__global__ void __launch_bounds__(256)
lm_front_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd,
                    float xscale, int has_pe, float* __restrict__ dz, int rows, int D, uint64_t seed1, uint64_t seed2,
                    const uint64_t* __restrict__ key, uint32_t th1, float ds1, uint32_t th2, float ds2) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // wave-uniform
  seed1 = esp::keyed(seed1, key);
  seed2 = esp::keyed(seed2, key);
  const float m = mean[r], rs = rstd[r];
  for (int c = lane; c < D; c += 64) {
    const uint64_t idx = (uint64_t)(r * D + c);
    float g = dy[r * D + c];
    if (has_pe) {
      if (th2) g = esp::keep_elem(seed2, idx, th2) ? g * ds2 : 0.f;
      g *= xscale;
    }
    const float t = front_pre(x[r * D + c], m, rs, gamma[c], beta[c], seed1, th1, ds1, idx);
    dz[r * D + c] = t > 0.f ? g * ds1 : 0.f;
  }
}

}  // namespace

ESP_API int esp_step_linear(const float* x, long ldx, const float* W, long ldw, const float* bias,
                            const float* ln_gamma, const float* ln_beta, float ln_eps, int relu, const float* R,
                            long ldr, float* out, long ldo, int c0, float* out2, long row_stride2, int pos,
                            int capacity2, int rows2, int N, int K, int M, void* stream) {
  ESP_ARG_CHECK(N >= 1 && N <= 65535 * kRT && M >= 1 && K >= 4 && K <= kMaxK && K % 4 == 0,
                "esp_step_linear: bad sizes N=%d K=%d M=%d (K a multiple of 4, at most %d)", N, K, M, kMaxK);
  ESP_ARG_CHECK(x && W, "esp_step_linear: null x / W");
  ESP_ARG_CHECK((ln_gamma == nullptr) == (ln_beta == nullptr), "esp_step_linear: LayerNorm needs gamma and beta");
  ESP_ARG_CHECK(ldx >= K && ldw >= K && !((ldx | ldw) & 3) && !(((uintptr_t)x | (uintptr_t)W) & 15),
                "esp_step_linear: x / W rows need 16-byte alignment and a pitch of at least K");
  ESP_ARG_CHECK(c0 >= 0 && c0 <= M, "esp_step_linear: split column %d outside [0, %d]", c0, M);
  ESP_ARG_CHECK(c0 == 0 || (out && ldo >= c0), "esp_step_linear: dense output missing or its pitch below %d", c0);
  ESP_ARG_CHECK(!R || ldr >= M, "esp_step_linear: residual pitch %ld below M = %d", ldr, M);
  long off2 = 0;
  if (c0 < M) {
    const long w2 = M - c0;
    ESP_ARG_CHECK(out2 && pos >= 0 && pos < capacity2 && N <= rows2 && row_stride2 >= (long)capacity2 * w2,
                  "esp_step_linear: split store outside its buffer (pos %d of %d positions, %d of %d rows, row "
                  "stride %ld for %ld columns)", pos, capacity2, N, rows2, row_stride2, w2);
    off2 = (long)pos * w2;
  }
  const dim3 grid((unsigned)((M + kCPB - 1) / kCPB), (unsigned)((N + kRT - 1) / kRT)), block(256);
  const size_t lds = (size_t)kRT * K * sizeof(float);
  hipLaunchKernelGGL(step_linear_kernel, grid, block, lds, (hipStream_t)stream, x, ldx, W, ldw, bias, ln_gamma, ln_beta,
                     ln_eps, relu, R, ldr, out, ldo, c0, out2, row_stride2, off2, N, K, M);
  ESP_CHECK_LAUNCH("esp_step_linear");
  return 0;
}

ESP_API int esp_step_ln_act(const float* x, const float* gamma, const float* beta, float eps, float xscale,
                            const float* pe, int L, int pos0, int pe_rows, float* y, int rows, int D, void* stream) {
  ESP_ARG_CHECK(x && gamma && beta && y && rows >= 1 && D >= 1 && L >= 1 && pos0 >= 0,
                "esp_step_ln_act: bad arguments rows=%d D=%d L=%d pos0=%d", rows, D, L, pos0);
  ESP_ARG_CHECK(!pe || pos0 + (rows < L ? rows : L) <= pe_rows,
                "esp_step_ln_act: positions [%d, %d) outside a table of %d rows", pos0, pos0 + (rows < L ? rows : L),
                pe_rows);
  hipLaunchKernelGGL(step_ln_act_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma,
                     beta, eps, xscale, pe, L, pos0, y, rows, D);
  ESP_CHECK_LAUNCH("esp_step_ln_act");
  return 0;
}

ESP_API int esp_lm_front_fwd(const float* x, const float* gamma, const float* beta, float eps, float xscale,
                             const float* pe, int L, int pe_rows, float p1, unsigned long long seed1, float p2,
                             unsigned long long seed2, float* y, float* mean, float* rstd, int rows, int D,
                             void* stream) {
  ESP_ARG_CHECK(x && gamma && beta && y && mean && rstd && rows >= 1 && D >= 1 && L >= 1,
                "esp_lm_front_fwd: bad arguments rows=%d D=%d L=%d", rows, D, L);
  ESP_ARG_CHECK(!pe || (rows < L ? rows : L) <= pe_rows, "esp_lm_front_fwd: %d positions outside a table of %d rows",
                rows < L ? rows : L, pe_rows);
  ESP_ARG_CHECK(p1 >= 0.f && p1 < 1.f && p2 >= 0.f && p2 < 1.f, "esp_lm_front_fwd: dropout %f / %f outside [0, 1)", p1,
                p2);
  const uint32_t th1 = esp::drop_threshold(p1), th2 = pe ? esp::drop_threshold(p2) : 0;
  hipLaunchKernelGGL(lm_front_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma,
                     beta, eps, xscale, pe, L, y, mean, rstd, rows, D, (uint64_t)seed1, (uint64_t)seed2,
                     esp::rng_key_ptr(), th1, esp::drop_scale(th1), th2, esp::drop_scale(th2));
  ESP_CHECK_LAUNCH("esp_lm_front_fwd");
  return 0;
}

ESP_API int esp_lm_front_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                             const float* rstd, float xscale, int has_pe, float p1, unsigned long long seed1, float p2,
                             unsigned long long seed2, float* dz, float* dx, float* dgamma, float* dbeta, int rows,
                             int D, float* work, long work_bytes, void* stream) {
  ESP_ARG_CHECK(dy && x && gamma && beta && mean && rstd && dz && dx && dgamma && dbeta && rows >= 1 && D >= 1,
                "esp_lm_front_bwd: bad arguments rows=%d D=%d", rows, D);
  ESP_ARG_CHECK(dz != dy && dz != dx, "esp_lm_front_bwd: dz must be a buffer of its own");
  ESP_ARG_CHECK(p1 >= 0.f && p1 < 1.f && p2 >= 0.f && p2 < 1.f, "esp_lm_front_bwd: dropout %f / %f outside [0, 1)", p1,
                p2);
  ESP_ARG_CHECK(D % 4 == 0 && work_bytes >= esp_layernorm_bwd_workspace_bytes(rows, D),
                "esp_lm_front_bwd: D=%d must be a multiple of 4 and the workspace (%ld B) esp_layernorm_bwd's", D,
                work_bytes);
  const uint32_t th1 = esp::drop_threshold(p1), th2 = has_pe ? esp::drop_threshold(p2) : 0;
  hipLaunchKernelGGL(lm_front_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dy, x,
                     gamma, beta, mean, rstd, xscale, has_pe, dz, rows, D, (uint64_t)seed1, (uint64_t)seed2,
                     esp::rng_key_ptr(), th1, esp::drop_scale(th1), th2, esp::drop_scale(th2));
  ESP_CHECK_LAUNCH("esp_lm_front_bwd");
  // dx = LN'(dz), dgamma / dbeta += (the LayerNorm adjoint every other norm of the model uses)
  return esp_layernorm_bwd(dz, x, gamma, mean, rstd, dx, 0, dgamma, dbeta, rows, D, work, work_bytes, stream);
}
