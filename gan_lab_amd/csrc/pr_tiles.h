// The tile walk of the row-set metrics (prdc.hip, kid.hip): dot products of 64 query rows with 64 key rows over the whole depth on
// the exact-fp32 MFMA, one definition so that both families form the same bits.
//   products as keys x queries on v_mfma_f32_32x32x2_f32: lane L supplies A[i = L & 31][kk = L >> 5] = key i,
//   B[kk][j = L & 31] = query j; the result sits at column j = L & 31, rows pr_row(r, L >> 5) of register r.
// A workgroup is 2 x 2 waves over 64 queries x 64 keys; the depth D is walked in chunks of 32 through [row][33] LDS tiles (both
// operands are read down a column at stride 33: conflict free).  An fp32 MFMA accumulator is one k-ordered fmaf chain, so every
// PR_DUMP chunks (64 terms) the running chain is added into a second accumulator and restarts: chains of 64 terms summed by a
// chain of D / 64 partials.  Tails in rows and depth are zero-filled on load.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PR_LD = 33;                     // LDS row stride of a 32-column tile
constexpr int PR_TILE = 64;                   // queries per workgroup and keys per tile (2 waves x 32 each)
constexpr int PR_DUMP = 2;                    // depth chunks (of 32) per accumulation chain
constexpr int PR_SMEM = 2 * PR_TILE * PR_LD;  // floats of the two operand tiles; reused by the final merge (256 x 16 floats)
constexpr int PR_MAX_ROWS = 1 << 30;

__device__ __forceinline__ int pr_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 pr_zero() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// LDS tile [64][PR_LD] <- src[r0 + row][c0 .. c0 + 32) of a (rows, D) row-major matrix; zero outside
__device__ __forceinline__ void pr_load_tile(float* lds, const float* __restrict__ src, int rows, int D, int r0, int c0) {
  for (int idx = threadIdx.x; idx < PR_TILE * 32; idx += 256) {
    const int r = idx >> 5, c = idx & 31;
    float v = 0.f;
    if (r0 + r < rows && c0 + c < D) v = src[(long long)(r0 + r) * D + c0 + c];
    lds[r * PR_LD + c] = v;
  }
}

// dot[r] = keys[k0 + kw * 32 + pr_row(r, h)] . q[q0 + qw * 32 + j] over the whole depth
__device__ __forceinline__ f32x16 pr_dots(float* qs, float* ks, const float* __restrict__ q, const float* __restrict__ keys,
                                          int M, int N, int D, int q0, int k0, int qw, int kw, int j, int h) {
  f32x16 run = pr_zero(), tot = pr_zero();
  int chunk = 0;
  for (int c0 = 0; c0 < D; c0 += 32) {
    __syncthreads();
    pr_load_tile(qs, q, M, D, q0, c0);
    pr_load_tile(ks, keys, N, D, k0, c0);
    __syncthreads();
    const float* a = ks + (kw * 32 + j) * PR_LD + h;
    const float* b = qs + (qw * 32 + j) * PR_LD + h;
#pragma unroll
    for (int st = 0; st < 16; ++st) run = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * st], b[2 * st], run, 0, 0, 0);
    if (++chunk == PR_DUMP) {
      chunk = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) tot[r] += run[r];
      run = pr_zero();
    }
  }
  if (chunk)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] += run[r];
  return tot;
}
