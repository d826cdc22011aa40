// Row sums of the cubic polynomial kernel between two sets of fp32 feature rows: the three passes of the unbiased MMD^2 behind
// the Kernel Inception Distance (Binkowski et al. 2018); composed in gan_lab_amd/kid.py, DESIGN.md 4.19.  Matrix-free: the M x N
// kernel matrix never exists.  The tile walk is prdc.hip's (pr_tiles.h): a workgroup owns 64 query rows, walks all key tiles and
// forms the dot products on the exact-fp32 MFMA; where prdc counts the keys under a radius, this kernel cubes and sums:
//   out[i] = sum_j (gamma q_i.k_j + coef0)^3,  t = fmaf(gamma, dot, coef0) one fp32 fma, its cube and every sum in float64.
// A lane owns ONE query and 16 keys of a tile and adds them in key order, tile after tile; the four lanes that share a query (2
// lane halves x 2 key waves) are joined through LDS at the end, by one lane in a fixed order.  No atomics, nothing depends on the
// launch geometry: bitwise reproducible.  Tails in rows and depth are zero-filled on load and masked by index; with
// exclude_diag the term j == i is left out by index (a duplicate row at another index counts).
#include "pr_tiles.h"

namespace {

template <bool EXCLUDE_DIAG>
__global__ __launch_bounds__(256) void kid_rowsums_kernel(const float* __restrict__ q, const float* __restrict__ keys,
                                                          double* __restrict__ out, int M, int N, int D, float gamma,
                                                          float coef0) {
  __shared__ __attribute__((aligned(16))) float smem[PR_SMEM];
  float* qs = smem;
  float* ks = smem + PR_TILE * PR_LD;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int qw = wave >> 1, kw = wave & 1;
  const int q0 = blockIdx.x * PR_TILE, qi = q0 + qw * 32 + j;
  double acc = 0.0;
  for (int k0 = 0; k0 < N; k0 += PR_TILE) {
    const f32x16 dot = pr_dots(qs, ks, q, keys, M, N, D, q0, k0, qw, kw, j, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {                           // keys ascending in r
      const int key = k0 + kw * 32 + pr_row(r, h);
      const double t = (double)fmaf(gamma, dot[r], coef0);
      if (key < N && !(EXCLUDE_DIAG && key == qi)) acc += t * t * t;
    }
  }
  __syncthreads();
  double* part = reinterpret_cast<double*>(smem);            // 256 doubles: within the two operand tiles
  part[threadIdx.x] = acc;
  __syncthreads();
  if (kw != 0 || h != 0 || qi >= M) return;
#pragma unroll
  for (int s = 1; s < 4; ++s) acc += part[((qw * 2 + (s >> 1)) * 64) + (s & 1) * 32 + j];   // (key wave, lane half) = (0,1) (1,0) (1,1)
  out[qi] = acc;
}

}  // namespace

extern "C" int ganlab_kid_rowsums_f32(const float* q, long long M, const float* keys, long long N, int D, float gamma, float coef0,
                                      int exclude_diag, double* out, void* stream) {
  if (!q || !keys || !out || M < 1 || N < 1 || D < 1) return GANLAB_EINVAL;
  if ((exclude_diag != 0 && exclude_diag != 1) || (exclude_diag && M != N)) return GANLAB_EINVAL;
  if (!(gamma == gamma) || !(coef0 == coef0)) return GANLAB_EINVAL;
  if (M > PR_MAX_ROWS || N > PR_MAX_ROWS) return GANLAB_EINVAL;
  const dim3 grid((unsigned)((M + PR_TILE - 1) / PR_TILE));
  hipStream_t st = gl_stream(stream);
  if (exclude_diag) GL_LAUNCH(kid_rowsums_kernel<true>, grid, dim3(256), 0, st, q, keys, out, (int)M, (int)N, D, gamma, coef0);
  else GL_LAUNCH(kid_rowsums_kernel<false>, grid, dim3(256), 0, st, q, keys, out, (int)M, (int)N, D, gamma, coef0);
  return GL_CHECK_LAUNCH();
}
