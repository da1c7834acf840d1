// Query-side gradients of latest rel-pos attention straight from dS (attention.py:240-263 backward), d_k = 64:
//   dq_u[i] = sum_j dS[i][j] k[j]             (ac = q_u k^T)
//   dq_v[i] = sum_j dS[i][j] p[T-1-i+j]       (bd[i][j] = q_v[i] . p[T-1-i+j], the latest rel_shift)
// The rel_shift adjoint dbd[i][T-1-i+j] = dS[i][j] is dS re-indexed, so no dbd tensor is formed: one block per
// (z = h*nb + b, 32 query rows) stages its dS rows in LDS once and reads that image twice, straight for dq_u
// and with a per-row skew for dq_v,
//   A'[r][x] = dS[i0+r][x - 31 + r]   against   p rows kmin + x,  kmin = T - 32 - i0,  x < T + 31
// (elements outside [0, T) are zeroed by predicate, never read from the neighbouring row).  Arithmetic is the
// GEMM family's: both operands split into three bf16 parts in registers (esp::split3_pair), the six products
// smallest first on v_mfma_f32_32x32x16_bf16, fp32 accumulate.  Waves: (u | v) x (d half c); the v tiles pass
// through LDS and the u waves store dq_u + dq_v.  Per block the column sums of dq_u and dq_v go to
// bias_part (Z, ceil(T/32), 2, 64), the layout esp_relpos_dp reduces in fixed order into the pos_bias gradients.
#include <stdlib.h>

#include "common.h"

namespace {

constexpr int QR = 32, QDK = 64, QKS = 32;  // query rows per block, d_k, k per loop iteration (two MFMA k-steps)
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// accumulator register r of lane half hf -> tile row
__device__ __forceinline__ int il_of(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

__device__ __forceinline__ void split8(const float* v, bf16x8 (&o)[3]) {
  uint32_t H[4], M[4], L[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) esp::split3_pair(v[2 * p], v[2 * p + 1], H[p], M[p], L[p]);
  o[0] = __builtin_bit_cast(bf16x8, make_uint4(H[0], H[1], H[2], H[3]));
  o[1] = __builtin_bit_cast(bf16x8, make_uint4(M[0], M[1], M[2], M[3]));
  o[2] = __builtin_bit_cast(bf16x8, make_uint4(L[0], L[1], L[2], L[3]));
}
// mid.mid, lo.hi, hi.lo, mid.hi, hi.mid, hi.hi (gemm_kernels.h mma6)
__device__ __forceinline__ void mma6(f32x16& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
  constexpr int PA[6] = {1, 2, 0, 1, 0, 0}, PB[6] = {1, 0, 2, 0, 1, 0};
#pragma unroll
  for (int p = 0; p < 6; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA[p]], b[PB[p]], acc, 0, 0, 0);
}

// DSP: LDS row pitch, 32 ceil(T/32) + 4 floats: an odd number of quads (the straight 16-B reads of 16 rows hit
// 16 different quad banks) and DSP + 1 odd (the skewed 4-B reads of 32 rows hit 32 different banks)
__global__ __launch_bounds__(256) void relpos_dq_kernel(const float* __restrict__ dS, long lds,
                                                        const float* __restrict__ kmat, long ldk,
                                                        const float* __restrict__ pm, long ldpm,
                                                        float* __restrict__ dq, long ldq,
                                                        float* __restrict__ bias_part, int nb, int T, int DSP) {
  extern __shared__ float ds[];  // [32][DSP]; after the k-loops the dq_v tiles [2][32][33]
  const int nqb = (T + QR - 1) / QR;
  const int qb = blockIdx.x % nqb, z = blockIdx.x / nqb;
  const int i0 = qb * QR;
  const int head = z / nb, b = z - head * nb;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (wave-uniform)
  const int hf = lane >> 5, l32 = lane & 31;
  // u | v alternate with the block so each SIMD (one wave of every block) sees both kinds of wave
  const int job = ((wave >> 1) + blockIdx.x) & 1, c = wave & 1;

  // stage the block's dS rows: wave w rows w, w+4, .. (a row is <= 2 x 64 quads: DSP <= 512); columns >= T
  // and rows >= T as 0 (the pitch's pad columns in HBM are not trusted).  Four rows' loads are issued before
  // their LDS stores, so a wave keeps 8 x 16 B per lane in flight instead of one load per round trip.
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    float4 v[4][2];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int i = i0 + wave + 4 * (4 * rb + rr);
      const float* src = dS + ((long)z * T + i) * lds;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c4 = 4 * lane + 256 * u;
        v[rr][u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < T && c4 < T) v[rr][u] = *reinterpret_cast<const float4*>(src + c4);  // c4 + 3 < lds (lds % 4 == 0)
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = wave + 4 * (4 * rb + rr);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c4 = 4 * lane + 256 * u;
        float4 w = v[rr][u];
        if (c4 + 1 >= T) w.y = 0.f;
        if (c4 + 2 >= T) w.z = 0.f;
        if (c4 + 3 >= T) w.w = 0.f;
        if (c4 < DSP) *reinterpret_cast<float4*>(ds + r * DSP + c4) = w;
      }
    }
  }
  __syncthreads();

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // lane's k of a 32-k iteration at base x0: x0 + 16 t + 8 hf + s (t = MFMA k-step, s < 8), A and B alike
  if (job == 0) {
    // k rows through 32-bit byte offsets from one uniform base: row * 4 ldk (a 24-bit multiply) + the lane's column
    const char* kbase = reinterpret_cast<const char*>(kmat + (long)b * T * ldk + QDK * head + 32 * c);
    const uint32_t ldk4 = (uint32_t)ldk * 4u, l4 = 4u * (uint32_t)l32;
    auto kld = [&](int row) {
      return *reinterpret_cast<const float*>(kbase + (__umul24((uint32_t)min(row, T - 1), ldk4) + l4));
    };
    const int nit = (T + QKS - 1) / QKS;  // columns < 32 nit <= DSP - 4 are staged (0 beyond T)
    float bf[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) bf[s] = kld(16 * (s >> 3) + 8 * hf + (s & 7));
#pragma unroll 1
    for (int it = 0; it < nit; ++it) {
      const int x0 = it * QKS;
      float af[16], bn[16];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float4 v = *reinterpret_cast<const float4*>(ds + l32 * DSP + x0 + 16 * t + 8 * hf + 4 * u);
          af[8 * t + 4 * u] = v.x; af[8 * t + 4 * u + 1] = v.y; af[8 * t + 4 * u + 2] = v.z; af[8 * t + 4 * u + 3] = v.w;
        }
      if (it + 1 < nit) {
#pragma unroll
        for (int s = 0; s < 16; ++s) bn[s] = kld(x0 + QKS + 16 * (s >> 3) + 8 * hf + (s & 7));
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x8 ah[3], bh[3];
        split8(af + 8 * t, ah);
        split8(bf + 8 * t, bh);
        mma6(acc, ah, bh);
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) bf[s] = bn[s];
    }
  } else {
    const int kmin = T - QR - i0, pmax = 2 * T - 2;
    const char* pbase = reinterpret_cast<const char*>(pm + QDK * head + 32 * c);
    const uint32_t ldp4 = (uint32_t)ldpm * 4u, l4 = 4u * (uint32_t)l32;
    auto pld = [&](int x) {
      return *reinterpret_cast<const float*>(pbase + (__umul24((uint32_t)min(max(kmin + x, 0), pmax), ldp4) + l4));
    };
    const int nit = (T + QR - 1 + QKS - 1) / QKS;  // window columns x < T + 31
    float bf[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) bf[s] = pld(16 * (s >> 3) + 8 * hf + (s & 7));
    const float* arow = ds + l32 * DSP + l32 - (QR - 1);  // A'[l32][x] = arow[x]
#pragma unroll 1
    for (int it = 0; it < nit; ++it) {
      const int x0 = it * QKS;
      float af[16], bn[16];
      // every row's columns j = x + r - 31 of this iteration inside [0, DSP): no predicate (all but the
      // first and the last one or two iterations)
      if (x0 >= QR - 1 && x0 + QKS - 1 + QR - 1 < DSP) {
#pragma unroll
        for (int s = 0; s < 16; ++s) af[s] = arow[x0 + 16 * (s >> 3) + 8 * hf + (s & 7)];
      } else {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const int x = x0 + 16 * (s >> 3) + 8 * hf + (s & 7);
          const int j = x + l32 - (QR - 1);  // staged columns [0, DSP) of the lane's own row; 0 from T on
          af[s] = (j >= 0 && j < DSP) ? arow[x] : 0.f;
        }
      }
      if (it + 1 < nit) {
#pragma unroll
        for (int s = 0; s < 16; ++s) bn[s] = pld(x0 + QKS + 16 * (s >> 3) + 8 * hf + (s & 7));
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x8 ah[3], bh[3];
        split8(af + 8 * t, ah);
        split8(bf + 8 * t, bh);
        mma6(acc, ah, bh);
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) bf[s] = bn[s];
    }
  }
  // column sums over the block's rows (rows >= T are zero rows of A): the pos_bias_u / pos_bias_v partials
  {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[r];
    s += __shfl_xor(s, 32, 64);
    if (hf == 0) bias_part[(((long)z * nqb + qb) * 2 + job) * QDK + 32 * c + l32] = s;
  }
  __syncthreads();  // the dS image is dead
  constexpr int VP = 33;
  float* vt = ds;  // [2][32][VP] (the host sizes the LDS for it)
  if (job == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) vt[(c * QR + il_of(r, hf)) * VP + l32] = acc[r];
  }
  __syncthreads();
  if (job == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = il_of(r, hf);
      if (i0 + row < T)
        dq[((long)b * T + i0 + row) * ldq + QDK * head + 32 * c + l32] = acc[r] + vt[(c * QR + row) * VP + l32];
    }
  }
}

}  // namespace

static int relpos_dq_pitch(int T) { return (T + 31) / 32 * 32 + 4; }

// dq (rows b*T + i, pitch ldq, head h at column 64 h; overwritten) = dq_u + dq_v from dS ((nb*H*T) rows of pitch
// lds, lds % 4 == 0, 16-B aligned), k rows at kmat + (b*T + j)*ldk + 64 h, p (2T-1 rows of pitch ldpm, head h at
// column 64 h); bias_part (nb*H, ceil(T/32), 2, 64): per-block column sums of dq_u and dq_v.  T <= 480 (64 KB LDS).
ESP_API int esp_relpos_dq(const float* dS, long lds, const float* kmat, long ldk, const float* p, long ldpm, float* dq,
                          long ldq, float* bias_part, int nb, int H, int T, void* stream) {
  ESP_ARG_CHECK(T >= 1 && nb >= 1 && H >= 1 && lds >= T && lds % 4 == 0 && ((uintptr_t)dS & 15) == 0,
                "esp_relpos_dq: bad sizes T=%d lds=%ld (lds %% 4 == 0, dS 16-B aligned)", T, lds);
  const int DSP = relpos_dq_pitch(T);
  size_t shm = (size_t)QR * DSP * sizeof(float);
  if (shm < 2 * QR * 33 * sizeof(float)) shm = 2 * QR * 33 * sizeof(float);  // the dq_v tiles reuse the image
  ESP_ARG_CHECK(shm <= 65536 && DSP <= 512, "esp_relpos_dq: T=%d needs %zu B of LDS (T <= 480)", T, shm);
  ESP_ARG_CHECK(dq && bias_part && kmat && p, "esp_relpos_dq: null operand");
  ESP_ARG_CHECK(ldk >= 64 && ldpm >= 64 && ldk < (1L << 22) && ldpm < (1L << 22) && 4L * T * ldk < (1L << 31) &&
                    4L * (2 * T - 1) * ldpm < (1L << 31),
                "esp_relpos_dq: ldk / ldpm out of range (row byte offsets on 24-bit multiplies, < 2^31)");
  const int nqb = (T + QR - 1) / QR;
  hipLaunchKernelGGL(relpos_dq_kernel, dim3((unsigned)((long)nb * H * nqb)), dim3(256), shm, (hipStream_t)stream, dS, lds,
                     kmat, ldk, p, ldpm, dq, ldq, bias_part, nb, T, DSP);
  ESP_CHECK_LAUNCH("esp_relpos_dq");
  return 0;
}
