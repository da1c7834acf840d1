// One time step of a torch.nn.LSTM layer (gate order i, f, g, o) for B rows: the predictor of the RNN-Transducer
// (espnet2/asr/decoder/transducer_decoder.py rnn_forward).  The input projection x W_ih^T + b_ih + b_hh of every
// step is one GEMM outside; a step adds h_{u-1} W_hh^T as an exact fp32 FMA product inside the cell kernel (the
// few-row regime of esp_step_linear: W_hh streamed once per LSTM_BT rows), applies the nonlinearities and writes
// h_u, c_u and the gate activations.  The backward step forms dh_u = dh_above + dgates_{u+1} W_hh the same way,
// then the pre-activation gate gradients of step u.  One launch per step, nothing waits on another workgroup.
#include "common.h"

namespace {

constexpr int LSTM_BT = 8;  // rows per wave in the forward

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }

// grid (ceil(H / 4), ceil(B / LSTM_BT)), 256 threads: wave w of block x owns hidden unit j = 4 x + w for LSTM_BT
// rows; lanes stride the recurrent dot products over k (coalesced rows of W_hh), fixed-order wave reduction.
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(const float* __restrict__ xproj, long ldx,
                                                            const float* __restrict__ hprev, long ldh,
                                                            const float* __restrict__ cprev, long ldc,
                                                            const float* __restrict__ Whh, float* __restrict__ acts,
                                                            long lda, float* __restrict__ hout, long ldho,
                                                            float* __restrict__ hout2, long ldho2,
                                                            float* __restrict__ cout, long ldco, int B, int H) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b0 = blockIdx.y * LSTM_BT;
  if (j >= H) return;
  float acc[LSTM_BT][4];
#pragma unroll
  for (int r = 0; r < LSTM_BT; ++r)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[r][g] = 0.f;
  if (hprev) {
    for (int k0 = 0; k0 < H; k0 += 64) {
      const int k = k0 + lane;
      const bool kv = k < H;
      float w[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) w[g] = kv ? Whh[((long)g * H + j) * H + k] : 0.f;
#pragma unroll
      for (int r = 0; r < LSTM_BT; ++r) {
        const float hv = (kv && b0 + r < B) ? hprev[(long)(b0 + r) * ldh + k] : 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[r][g] = fmaf(w[g], hv, acc[r][g]);
      }
    }
#pragma unroll
    for (int r = 0; r < LSTM_BT; ++r)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[r][g] = esp::wave_sum(acc[r][g]);
  }
  float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < LSTM_BT; ++r)
    if (lane == r) {
#pragma unroll
      for (int g = 0; g < 4; ++g) p[g] = acc[r][g];
    }
  const int b = b0 + lane;
  if (lane >= LSTM_BT || b >= B) return;
  const float* xr = xproj + (long)b * ldx;
  const float gi = sigm(xr[j] + p[0]);
  const float gf = sigm(xr[H + j] + p[1]);
  const float gg = tanhf(xr[2 * H + j] + p[2]);
  const float go = sigm(xr[3 * H + j] + p[3]);
  const float cp = cprev ? cprev[(long)b * ldc + j] : 0.f;
  const float c = gf * cp + gi * gg;
  const float h = go * tanhf(c);
  if (acts) {
    float* ar = acts + (long)b * lda;
    ar[j] = gi;
    ar[H + j] = gf;
    ar[2 * H + j] = gg;
    ar[3 * H + j] = go;
  }
  cout[(long)b * ldco + j] = c;
  hout[(long)b * ldho + j] = h;
  if (hout2) hout2[(long)b * ldho2 + j] = h;
}

// grid (ceil(H / 64), ceil(B / 4)), 256 threads: a block owns 64 hidden units of 4 rows.  Wave w sums gate w's
// slice of dgates_{u+1} W_hh for the block's rows (lanes over j: coalesced rows of W_hh), the four slices are
// added in gate order, then thread (w, lane) finishes row b0 + w, unit j.
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float* __restrict__ dh, long lddh,
                                                            const float* __restrict__ dgnext, long ldgn,
                                                            const float* __restrict__ Whh,
                                                            const float* __restrict__ acts, long lda,
                                                            const float* __restrict__ c, long ldc,
                                                            const float* __restrict__ cprev, long ldcp,
                                                            const float* dc_in, float* dc_out,  // (may alias)
                                                            float* __restrict__ dgates, long ldg, int B, int H) {
  __shared__ float part[4][4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int b0 = blockIdx.y * 4;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (dgnext && j < H) {
    const float* wr = Whh + (long)w * H * H + j;
    for (int k = 0; k < H; ++k) {
      const float wv = wr[(long)k * H];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gv = b0 + r < B ? dgnext[(long)(b0 + r) * ldgn + (long)w * H + k] : 0.f;
        a[r] = fmaf(gv, wv, a[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) part[w][r][lane] = a[r];
  __syncthreads();
  const int b = b0 + w;
  if (j >= H || b >= B) return;
  const float rec = ((part[0][w][lane] + part[1][w][lane]) + part[2][w][lane]) + part[3][w][lane];
  const float dhv = dh[(long)b * lddh + j] + rec;
  const float* ar = acts + (long)b * lda;
  const float gi = ar[j], gf = ar[H + j], gg = ar[2 * H + j], go = ar[3 * H + j];
  const float tc = tanhf(c[(long)b * ldc + j]);
  const float cp = cprev ? cprev[(long)b * ldcp + j] : 0.f;
  const float dcv = dhv * go * (1.f - tc * tc) + (dc_in ? dc_in[(long)b * H + j] : 0.f);
  float* gr = dgates + (long)b * ldg;
  gr[j] = dcv * gg * gi * (1.f - gi);
  gr[H + j] = dcv * cp * gf * (1.f - gf);
  gr[2 * H + j] = dcv * gi * (1.f - gg * gg);
  gr[3 * H + j] = dhv * tc * go * (1.f - go);
  dc_out[(long)b * H + j] = dcv * gf;
}

}  // namespace

ESP_API int esp_lstm_cell_fwd(const float* xproj, long ldx, const float* hprev, long ldh, const float* cprev, long ldc,
                              const float* Whh, float* acts, long lda, float* hout, long ldho, float* hout2,
                              long ldho2, float* cout, long ldco, int B, int H, void* stream) {
  ESP_ARG_CHECK(B > 0 && H > 0 && B <= 65535 * LSTM_BT, "esp_lstm_cell_fwd: bad sizes B=%d H=%d", B, H);
  ESP_ARG_CHECK(ldx >= 4L * H && ldho >= H && ldco >= H && (!hprev || ldh >= H) && (!cprev || ldc >= H) &&
                    (!acts || lda >= 4L * H) && (!hout2 || ldho2 >= H),
                "esp_lstm_cell_fwd: a row pitch is smaller than its row (H=%d)", H);
  hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3((H + 3) / 4, (B + LSTM_BT - 1) / LSTM_BT), dim3(256), 0,
                     (hipStream_t)stream, xproj, ldx, hprev, ldh, cprev, ldc, Whh, acts, lda, hout, ldho, hout2, ldho2,
                     cout, ldco, B, H);
  ESP_CHECK_LAUNCH("esp_lstm_cell_fwd");
  return 0;
}

ESP_API int esp_lstm_cell_bwd(const float* dh, long lddh, const float* dgnext, long ldgn, const float* Whh,
                              const float* acts, long lda, const float* c, long ldc, const float* cprev, long ldcp,
                              const float* dc_in, float* dc_out, float* dgates, long ldg, int B, int H, void* stream) {
  ESP_ARG_CHECK(B > 0 && H > 0 && B <= 65535 * 4, "esp_lstm_cell_bwd: bad sizes B=%d H=%d", B, H);
  ESP_ARG_CHECK(lddh >= H && lda >= 4L * H && ldc >= H && ldg >= 4L * H && (!dgnext || ldgn >= 4L * H) &&
                    (!cprev || ldcp >= H),
                "esp_lstm_cell_bwd: a row pitch is smaller than its row (H=%d)", H);
  ESP_ARG_CHECK(dgnext != dgates, "esp_lstm_cell_bwd: dgates of step u must not alias those of step u + 1");
  hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3((H + 63) / 64, (B + 3) / 4), dim3(256), 0, (hipStream_t)stream, dh, lddh,
                     dgnext, ldgn, Whh, acts, lda, c, ldc, cprev, ldcp, dc_in, dc_out, dgates, ldg, B, H);
  ESP_CHECK_LAUNCH("esp_lstm_cell_bwd");
  return 0;
}
