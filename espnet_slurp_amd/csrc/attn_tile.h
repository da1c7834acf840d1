// LDS tile helpers of the one-workgroup-per-(sequence, head) attention kernels (cbt.hip: esp_block_attn_*;
// causal_attn.hip: esp_causal_attn_*).  Sequences of at most 64 rows, 256 threads:
//   thread (ti, tj) = (tid / 16, tid % 16) owns rows ti + 16a and columns tj + 16b (a, b < NA = ceil(S / 16)) of an
//   S x S matrix, and rows ti + 16a, columns tj*CW .. tj*CW + CW - 1 (CW = DK / 16) of an S x DK result; a 16-lane
//   row group reduces a score row with four xor shuffles.
//   LDS tiles are row-major with pitch DK + 4 (S x S tiles: 16 NA + 4) floats.  The pitch / 4 is odd, so the 16
//   lanes of a row group that read 16 different rows with one ds_read_b128 hit 16 different 16-byte slots of the
//   256-byte bank row; the rows ti + 16a are shared by a whole row group (a broadcast).
//   Products are exact fp32 FMA chains in a fixed order: results repeat bit for bit.
#pragma once
#include "common.h"

namespace {

constexpr int kThreads = 256;

// rows [0, S) of src (pitch ld) -> dst (pitch DK + 4); rows [S, SP) are zero-filled
template <int DK>
__device__ __forceinline__ void stage_tile(float* __restrict__ dst, const float* __restrict__ src, long ld, int S,
                                           int SP) {
  constexpr int P = DK + 4, C4 = DK / 4;
  for (int i = threadIdx.x; i < SP * C4; i += kThreads) {
    const int r = i / C4, c = i - r * C4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < S) v = *reinterpret_cast<const float4*>(src + (long)r * ld + 4 * c);
    *reinterpret_cast<float4*>(dst + r * P + 4 * c) = v;
  }
}

// acc[a][b] = sum_k A[ti + 16a][k] * B[tj + 16b][k], both tiles of pitch DK + 4.  LOWER: the 16 x 16 tiles above
// the diagonal (b > a: every column beyond every row) are skipped and stay 0 -- a causal mask hides them anyway
template <int DK, int NA, bool LOWER = false>
__device__ __forceinline__ void mm_nt(const float* __restrict__ A, const float* __restrict__ B, int ti, int tj,
                                      float (&acc)[NA][NA]) {
  constexpr int P = DK + 4;
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NA; ++b) acc[a][b] = 0.f;
#pragma unroll 2
  for (int k = 0; k < DK; k += 4) {
    float4 av[NA], bv[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) av[a] = *reinterpret_cast<const float4*>(A + (ti + 16 * a) * P + k);
#pragma unroll
    for (int b = 0; b < NA; ++b) bv[b] = *reinterpret_cast<const float4*>(B + (tj + 16 * b) * P + k);
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NA; ++b) {
        if (LOWER && b > a) continue;
        float s = acc[a][b];
        s = fmaf(av[a].x, bv[b].x, s);
        s = fmaf(av[a].y, bv[b].y, s);
        s = fmaf(av[a].z, bv[b].z, s);
        s = fmaf(av[a].w, bv[b].w, s);
        acc[a][b] = s;
      }
  }
}

// acc[a][c] = sum_{j < nk} X[ti + 16a][j] * B[j][tj*CW + c]   (X of pitch PX, B of pitch DK + 4; nk % 4 == 0)
template <int DK, int NA>
__device__ __forceinline__ void mm_nn(const float* __restrict__ X, int PX, const float* __restrict__ B, int nk,
                                      int ti, int tj, float (&acc)[NA][DK / 16]) {
  constexpr int P = DK + 4, CW = DK / 16;
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int c = 0; c < CW; ++c) acc[a][c] = 0.f;
  for (int j = 0; j < nk; j += 4) {
    float xv[NA][4];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const float4 t = *reinterpret_cast<const float4*>(X + (ti + 16 * a) * PX + j);
      xv[a][0] = t.x, xv[a][1] = t.y, xv[a][2] = t.z, xv[a][3] = t.w;
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      float bv[CW];
#pragma unroll
      for (int c = 0; c < CW; ++c) bv[c] = B[(j + jj) * P + tj * CW + c];
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int c = 0; c < CW; ++c) acc[a][c] = fmaf(xv[a][jj], bv[c], acc[a][c]);
    }
  }
}

// acc[a][c] = sum_{i < ni} X[i][ti + 16a] * B[i][tj*CW + c]
template <int DK, int NA>
__device__ __forceinline__ void mm_tn(const float* __restrict__ X, int PX, const float* __restrict__ B, int ni,
                                      int ti, int tj, float (&acc)[NA][DK / 16]) {
  constexpr int P = DK + 4, CW = DK / 16;
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int c = 0; c < CW; ++c) acc[a][c] = 0.f;
#pragma unroll 2
  for (int i = 0; i < ni; ++i) {
    float xv[NA], bv[CW];
#pragma unroll
    for (int a = 0; a < NA; ++a) xv[a] = X[i * PX + ti + 16 * a];
#pragma unroll
    for (int c = 0; c < CW; ++c) bv[c] = B[i * P + tj * CW + c];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int c = 0; c < CW; ++c) acc[a][c] = fmaf(xv[a], bv[c], acc[a][c]);
  }
}

// reductions over the 16 lanes of a row group (lanes 16 ti .. 16 ti + 15 of the wave)
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// rows i = ti + 16a (< S) of an S x DK result -> global rows of pitch ld
template <int DK, int NA>
__device__ __forceinline__ void store_rows(float* __restrict__ dst, long ld, int S, int ti, int tj,
                                           const float (&acc)[NA][DK / 16]) {
  constexpr int CW = DK / 16;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = ti + 16 * a;
    if (i >= S) continue;
    float* p = dst + (long)i * ld + tj * CW;
    if constexpr (CW % 4 == 0) {
#pragma unroll
      for (int c = 0; c < CW; c += 4)
        *reinterpret_cast<float4*>(p + c) = make_float4(acc[a][c], acc[a][c + 1], acc[a][c + 2], acc[a][c + 3]);
    } else if constexpr (CW == 2) {
      *reinterpret_cast<float2*>(p) = make_float2(acc[a][0], acc[a][1]);
    } else {
      p[0] = acc[a][0];
    }
  }
}

template <int DK, int NA>
constexpr int region_a() {  // floats of a tile that holds an SP x DK operand first and an SP x SP matrix later
  return 16 * NA * ((DK + 4) > (16 * NA + 4) ? (DK + 4) : (16 * NA + 4));
}

// dynamic LDS above 64 KiB (of the CU's 160) has to be granted per kernel
template <typename Kern>
hipError_t grant_lds(Kern kern, size_t bytes) {
  if (bytes <= 65536) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes);
}

}  // namespace
