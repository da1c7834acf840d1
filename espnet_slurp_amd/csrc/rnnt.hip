// RNN-Transducer head (espnet2/asr/espnet_model.py:542-588, espnet2/asr_transducer/joint_network.py):
//   * the broadcast joint z[b,t,u,:] = act(pe[b,t,:] + pd[b,u,:]) and its adjoint (two reductions, one over u
//     and one over t, summed in a fixed order without atomics: per-tile partials + a reduce pass)
//   * per lattice cell the log-sum-exp over the vocabulary and the blank / label log-probabilities
//   * the forward / backward lattice recursions in log space (fp64 values, one workgroup per utterance and
//     direction, anti-diagonal sweep)
//   * the gradient of gscale * sum_b nll_b w.r.t. the logits, written in place over the logits
// Lengths reach every kernel as device int32 (hlens[b] = T_b, tlens[b] = U_b) beside the padded extents
// T, Umax, U1 = Umax + 1, so one captured graph serves every batch of a length bucket.  Blank is token 0.
#include "common.h"

namespace {

constexpr int ACT_TANH = 0, ACT_RELU = 1;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------ joint
__global__ __launch_bounds__(256) void joint_fwd_kernel(const float* __restrict__ pe, const float* __restrict__ pd,
                                                        float* __restrict__ z, int T, int U1, int J, int act, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long cell = i / J;
    const int j = (int)(i - cell * J);
    const long bt = cell / U1;
    const int u = (int)(cell - bt * U1);
    const long b = bt / T;
    const float v = pe[bt * J + j] + pd[(b * U1 + u) * J + j];
    z[i] = act == ACT_TANH ? tanhf(v) : fmaxf(v, 0.f);
  }
}

// grid (ceil(J / 128), ceil(T / JB_TT), B), 128 threads: thread j of a block owns column j of one tile of JB_TT
// frames.  g = dz * act'(z) is formed once per cell; dpe[b,t,j] = sum_u g is complete inside the tile (u ascending),
// part[b,tile,u,j] = sum over the tile's frames (t ascending); joint_reduce_kernel adds the tiles in ascending order.
// Cells with t >= T_b or u > U_b are not read and contribute exactly zero.
constexpr int JB_TT = 16, JB_NT = 128;
__global__ __launch_bounds__(JB_NT) void joint_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ z,
                                                          const int* __restrict__ hlens, const int* __restrict__ tlens,
                                                          float* __restrict__ dpe, float* __restrict__ part, int T,
                                                          int U1, int J, int act, int ntile) {
  const int j = blockIdx.x * JB_NT + threadIdx.x;
  const int tile = blockIdx.y, b = blockIdx.z;
  if (j >= J) return;
  const int Tb = clampi(hlens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
  const int t0 = tile * JB_TT;
  const int nt = min(JB_TT, T - t0);          // frames of this tile inside the padded extent
  const int nv = clampi(Tb - t0, 0, nt);      // ... of which valid
  float ape[JB_TT];
#pragma unroll
  for (int k = 0; k < JB_TT; ++k) ape[k] = 0.f;
  float* pr = part + (((long)b * ntile + tile) * U1) * J + j;
  for (int u = 0; u < U1; ++u) {
    float apd = 0.f;
    if (u <= Ub) {
      const long base = (((long)b * T + t0) * U1 + u) * J + j;
#pragma unroll
      for (int k = 0; k < JB_TT; ++k) {
        if (k < nv) {
          const long o = base + (long)k * U1 * J;
          const float zz = z[o];
          const float g = dz[o] * (act == ACT_TANH ? 1.f - zz * zz : (zz > 0.f ? 1.f : 0.f));
          ape[k] += g;
          apd += g;
        }
      }
    }
    pr[(long)u * J] = apd;
  }
#pragma unroll
  for (int k = 0; k < JB_TT; ++k)
    if (k < nt) dpe[((long)b * T + t0 + k) * J + j] = ape[k];
}

__global__ __launch_bounds__(256) void joint_reduce_kernel(const float* __restrict__ part, float* __restrict__ dpd,
                                                           int U1, int J, int ntile, long n) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;  // (b, u, j)
  if (i >= n) return;
  const long uj = (long)U1 * J;
  const long b = i / uj;
  const long r = i - b * uj;
  const float* p = part + b * ntile * uj + r;
  float a = 0.f;
  for (int k = 0; k < ntile; ++k) a += p[(long)k * uj];
  dpd[i] = a;
}

// ------------------------------------------------------------------------------------------ lattice
// workspace layout (doubles, N = B*T*U1 each): lse | lp_blank | lp_y | alpha | beta
// One wave per cell, four cells per block.  Padded cells (t >= T_b or u > U_b) are not read: zeros in all five.
__global__ __launch_bounds__(256) void rnnt_logprobs_kernel(const float* __restrict__ x, const int64_t* __restrict__ ys,
                                                            int Umax, const int* __restrict__ hlens,
                                                            const int* __restrict__ tlens, int T, int U1, int V, long N,
                                                            double* __restrict__ work) {
  const int lane = threadIdx.x & 63;
  const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= N) return;
  const long bt = cell / U1;
  const int u = (int)(cell - bt * U1);
  const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
  const int Tb = clampi(hlens[b], 0, T), Ub = clampi(tlens[b], 0, Umax);
  double* lse = work;
  double* lpb = work + N;
  double* lpy = work + 2 * N;
  if (t >= Tb || u > Ub) {
    if (lane == 0) {  // (alpha / beta too: the recursions visit the valid cells only)
      lse[cell] = 0.0; lpb[cell] = 0.0; lpy[cell] = 0.0;
      work[3 * N + cell] = 0.0; work[4 * N + cell] = 0.0;
    }
    return;
  }
  const float* xr = x + cell * V;
  float m = -INFINITY;
  for (int c = lane; c < V; c += 64) m = fmaxf(m, xr[c]);
  m = esp::wave_max(m);
  double s = 0.0;
  for (int c = lane; c < V; c += 64) s += (double)expf(xr[c] - m);
  s = esp::wave_sum_d(s);
  if (lane == 0) {
    const double l = (double)m + log(s);
    lse[cell] = l;
    lpb[cell] = (double)xr[0] - l;
    double ly = 0.0;
    if (u < Ub) ly = (double)xr[clampi((int)ys[(long)b * Umax + u], 0, V - 1)] - l;
    lpy[cell] = ly;
  }
}

__device__ __forceinline__ double lse2(double a, double b) {
  const double m = fmax(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log1p(exp(-fabs(a - b)));
}

// blockIdx.x = utterance, blockIdx.y = 0 alpha / 1 beta.  Diagonal d holds the cells t + u = d; entry u of the
// LDS line of a diagonal is the cell (d - u, u), so both predecessors of a cell sit in the previous line (alpha: u and
// u - 1; beta: u and u + 1).  A thread owns u = tid, tid + NT, ... (RNNT_SPT cells at most).
constexpr int RNNT_NT = 256, RNNT_SPT = 4;
__global__ __launch_bounds__(RNNT_NT) void rnnt_alpha_beta_kernel(const int* __restrict__ hlens,
                                                                  const int* __restrict__ tlens, int T, int U1, long N,
                                                                  double* __restrict__ work, double* __restrict__ nll) {
  __shared__ double line[2][RNNT_NT * RNNT_SPT + 1];
  const int b = blockIdx.x, dir = blockIdx.y;
  const int Tb = clampi(hlens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
  if (Tb <= 0) {
    if (dir == 0 && threadIdx.x == 0) nll[b] = INFINITY;
    return;
  }
  const long off = (long)b * T * U1;
  const double* lpb = work + N + off;
  const double* lpy = work + 2 * N + off;
  double* out = work + (dir == 0 ? 3 : 4) * N + off;
  const int D = Tb + Ub;  // diagonals 0 .. D - 1
  int cur = 0;
  if (dir == 0) {
    for (int d = 0; d < D; ++d) {
      const int ulo = max(0, d - (Tb - 1)), uhi = min(Ub, d);
      for (int u = ulo + threadIdx.x; u <= uhi; u += RNNT_NT) {
        const int t = d - u;
        double v;
        if (d == 0) v = 0.0;
        else {
          const double a = t > 0 ? line[cur ^ 1][u] + lpb[(long)(t - 1) * U1 + u] : -INFINITY;
          const double c = u > 0 ? line[cur ^ 1][u - 1] + lpy[(long)t * U1 + u - 1] : -INFINITY;
          v = lse2(a, c);
        }
        line[cur][u] = v;
        out[(long)t * U1 + u] = v;
        if (t == Tb - 1 && u == Ub) nll[b] = -(v + lpb[(long)t * U1 + u]);
      }
      cur ^= 1;
      __syncthreads();
    }
  } else {
    for (int d = D - 1; d >= 0; --d) {
      const int ulo = max(0, d - (Tb - 1)), uhi = min(Ub, d);
      for (int u = ulo + threadIdx.x; u <= uhi; u += RNNT_NT) {
        const int t = d - u;
        const double pb = lpb[(long)t * U1 + u];
        double v;
        if (d == D - 1) v = pb;
        else {
          const double a = t + 1 < Tb ? line[cur ^ 1][u] + pb : -INFINITY;
          const double c = u < Ub ? line[cur ^ 1][u + 1] + lpy[(long)t * U1 + u] : -INFINITY;
          v = lse2(a, c);
        }
        line[cur][u] = v;
        out[(long)t * U1 + u] = v;
      }
      cur ^= 1;
      __syncthreads();
    }
  }
}

// One wave per cell, four per block: the logits row becomes its gradient in place.
__global__ __launch_bounds__(256) void rnnt_grad_kernel(float* __restrict__ x, const int64_t* __restrict__ ys, int Umax,
                                                        const int* __restrict__ hlens, const int* __restrict__ tlens,
                                                        int T, int U1, int V, long N, float gscale,
                                                        const float* __restrict__ gdev, const double* __restrict__ nll,
                                                        const double* __restrict__ work) {
  const int lane = threadIdx.x & 63;
  const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= N) return;
  const long bt = cell / U1;
  const int u = (int)(cell - bt * U1);
  const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
  const int Tb = clampi(hlens[b], 0, T), Ub = clampi(tlens[b], 0, Umax);
  float* xr = x + cell * V;
  const double nl = nll[b];
  if (t >= Tb || u > Ub || !(fabs(nl) < INFINITY)) {
    for (int c = lane; c < V; c += 64) xr[c] = 0.f;
    return;
  }
  const double* lse = work;
  const double* lpb = work + N;
  const double* lpy = work + 2 * N;
  const double* al = work + 3 * N;
  const double* be = work + 4 * N;
  const float gs = gdev ? gscale * gdev[0] : gscale;
  const double a = al[cell], lnP = -nl;
  const float occ = (float)exp(a + be[cell] - lnP);
  // the blank move (t, u) -> (t + 1, u); from the last frame only the final cell has one (to the end)
  float tb = 0.f;
  if (t + 1 < Tb) tb = (float)exp(a + lpb[cell] + be[cell + U1] - lnP);
  else if (u == Ub) tb = (float)exp(a + lpb[cell] - lnP);
  float ty = 0.f;
  int y = -1;
  if (u < Ub) {
    y = clampi((int)ys[(long)b * Umax + u], 0, V - 1);
    ty = (float)exp(a + lpy[cell] + be[cell + 1] - lnP);
  }
  const double l = lse[cell];
  for (int c = lane; c < V; c += 64) {
    float g = expf((float)((double)xr[c] - l)) * occ;
    if (c == 0) g -= tb;
    if (c == y) g -= ty;
    xr[c] = g * gs;
  }
}

}  // namespace

ESP_API int esp_rnnt_joint_fwd(const float* pe, const float* pd, float* z, int B, int T, int U1, int J, int act,
                               void* stream) {
  ESP_ARG_CHECK(B > 0 && T > 0 && U1 > 0 && J > 0, "esp_rnnt_joint_fwd: bad sizes B=%d T=%d U1=%d J=%d", B, T, U1, J);
  ESP_ARG_CHECK(act == ACT_TANH || act == ACT_RELU, "esp_rnnt_joint_fwd: activation %d (0 tanh, 1 relu)", act);
  const long n = (long)B * T * U1 * J;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(joint_fwd_kernel, dim3((unsigned)(blocks < 65536 * 8 ? blocks : 65536 * 8)), dim3(256), 0,
                     (hipStream_t)stream, pe, pd, z, T, U1, J, act, n);
  ESP_CHECK_LAUNCH("esp_rnnt_joint_fwd");
  return 0;
}

ESP_API long esp_rnnt_joint_bwd_workspace_bytes(int B, int T, int U1, int J) {
  if (B <= 0 || T <= 0 || U1 <= 0 || J <= 0) return 0;
  return 4L * B * ((T + JB_TT - 1) / JB_TT) * U1 * J;
}
ESP_API int esp_rnnt_joint_bwd(const float* dz, const float* z, const int* hlens, const int* tlens, float* dpe,
                               float* dpd, int B, int T, int U1, int J, int act, float* work, long work_bytes,
                               void* stream) {
  ESP_ARG_CHECK(B > 0 && T > 0 && U1 > 0 && J > 0, "esp_rnnt_joint_bwd: bad sizes B=%d T=%d U1=%d J=%d", B, T, U1, J);
  ESP_ARG_CHECK(act == ACT_TANH || act == ACT_RELU, "esp_rnnt_joint_bwd: activation %d (0 tanh, 1 relu)", act);
  ESP_ARG_CHECK(B <= 65535, "esp_rnnt_joint_bwd: B=%d > 65535", B);
  const long need__ = esp_rnnt_joint_bwd_workspace_bytes(B, T, U1, J);
  ESP_ARG_CHECK(work_bytes >= need__, "esp_rnnt_joint_bwd: workspace %ld B < %ld B required (esp_rnnt_joint_bwd_workspace_bytes)", work_bytes, need__);
  const int ntile = (T + JB_TT - 1) / JB_TT;
  ESP_ARG_CHECK(ntile <= 65535, "esp_rnnt_joint_bwd: T=%d too long", T);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(joint_bwd_kernel, dim3((J + JB_NT - 1) / JB_NT, ntile, B), dim3(JB_NT), 0, st, dz, z, hlens, tlens,
                     dpe, work, T, U1, J, act, ntile);
  const long n = (long)B * U1 * J;
  hipLaunchKernelGGL(joint_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, work, dpd, U1, J, ntile,
                     n);
  ESP_CHECK_LAUNCH("esp_rnnt_joint_bwd");
  return 0;
}

ESP_API long esp_rnnt_loss_workspace_bytes(int B, int T, int U1) {
  return B <= 0 || T <= 0 || U1 <= 0 ? 0 : 8L * 5 * B * T * U1;
}

#define RNNT_COMMON_CHECKS(name)                                                                                   \
  ESP_ARG_CHECK(B > 0 && T > 0 && U1 > 0, name ": bad sizes B=%d T=%d U1=%d", B, T, U1);                            \
  ESP_ARG_CHECK(U1 <= RNNT_NT * RNNT_SPT, name ": U1=%d > %d", U1, RNNT_NT * RNNT_SPT);                             \
  ESP_ARG_CHECK((long)B * T * U1 < (1L << 31), name ": B*T*U1 = %ld cells >= 2^31", (long)B * T * U1);               \
  {                                                                                                                \
    const long need__ = esp_rnnt_loss_workspace_bytes(B, T, U1);                                                   \
    ESP_ARG_CHECK(work_bytes >= need__, name ": workspace %ld B < %ld B required (esp_rnnt_loss_workspace_bytes)", \
                  work_bytes, need__);                                                                             \
  }

ESP_API int esp_rnnt_logprobs(const float* logits, const long long* ys, const int* hlens, const int* tlens, int B,
                              int T, int U1, int V, double* work, long work_bytes, void* stream) {
  RNNT_COMMON_CHECKS("esp_rnnt_logprobs");
  ESP_ARG_CHECK(V >= 1, "esp_rnnt_logprobs: V=%d", V);
  const long N = (long)B * T * U1;
  hipLaunchKernelGGL(rnnt_logprobs_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits,
                     (const int64_t*)ys, U1 - 1, hlens, tlens, T, U1, V, N, work);
  ESP_CHECK_LAUNCH("esp_rnnt_logprobs");
  return 0;
}

ESP_API int esp_rnnt_alpha_beta(const int* hlens, const int* tlens, int B, int T, int U1, double* work,
                                long work_bytes, double* nll, void* stream) {
  RNNT_COMMON_CHECKS("esp_rnnt_alpha_beta");
  const long N = (long)B * T * U1;
  hipLaunchKernelGGL(rnnt_alpha_beta_kernel, dim3(B, 2), dim3(RNNT_NT), 0, (hipStream_t)stream, hlens, tlens, T, U1, N,
                     work, nll);
  ESP_CHECK_LAUNCH("esp_rnnt_alpha_beta");
  return 0;
}

ESP_API int esp_rnnt_grad(float* logits, const long long* ys, const int* hlens, const int* tlens, int B, int T, int U1,
                          int V, float gscale, const float* gdev, const double* nll, const double* work,
                          long work_bytes, void* stream) {
  RNNT_COMMON_CHECKS("esp_rnnt_grad");
  ESP_ARG_CHECK(V >= 1, "esp_rnnt_grad: V=%d", V);
  const long N = (long)B * T * U1;
  hipLaunchKernelGGL(rnnt_grad_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits,
                     (const int64_t*)ys, U1 - 1, hlens, tlens, T, U1, V, N, gscale, gdev, nll, work);
  ESP_CHECK_LAUNCH("esp_rnnt_grad");
  return 0;
}
