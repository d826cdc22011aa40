// Streaming first and second moments of fp32 feature rows about a pivot, into float64 accumulators: the statistics behind the
// Frechet distance between two feature sets (FID when the rows are Inception's); composed in gan_lab_amd/frechet.py, DESIGN.md 4.19.
//   sum[a] += sum_i (x_ia - c_a),  gram[a][b] += sum_i (x_ia - c_a)(x_ib - c_b)      (i over the n rows of this launch)
// The pivot c is subtracted on load, in fp32 (exact when x and c are within a factor of two of each other), so rows with a large
// common offset do not cancel catastrophically in cov = (gram - sum sum^T / n) / (n - 1).
// A workgroup owns one 64 x 64 tile of gram, on or above the diagonal, and walks the n rows in chunks of 32 through two
// [row][col] LDS tiles.  The contraction runs over rows, so on v_mfma_f32_32x32x2_f32 lane L supplies A[i = L & 31][kk = L >> 5] =
// x[row kk][column a0 + i] and B[kk][j = L & 31] = x[row kk][column b0 + j]: both operands are read ALONG a row of the tile, 32
// consecutive words per lane half, conflict free at any stride.  The result sits at column j, rows fm_row(r, L >> 5) of register r.
// An fp32 MFMA accumulator is one row-ordered fmaf chain: every FM_DUMP chunks (32 terms) it is added into the launch's float64
// partial and restarts.  At the end the partial is added to gram by its one owner, and to the mirrored element below the diagonal
// as well (fmaf(a, b, c) == fmaf(b, a, c), so a diagonal tile is symmetric by itself): gram stays full and exactly symmetric.  The
// workgroups of the diagonal tiles also add their 64 columns into sum, row after row in float64.  No atomics, the grid is a
// function of D alone, every sum in a fixed order: bitwise reproducible.  Tails in rows and columns are zero-filled on load and
// masked by index.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int FM_TILE = 64;       // side of a gram tile (2 waves x 32 each way)
constexpr int FM_ROWS = 32;       // rows per chunk
constexpr int FM_DUMP = 1;        // chunks per fp32 accumulation chain: 32 terms
constexpr int FM_MAX_D = 4096;
constexpr long long FM_MAX_ROWS = 1LL << 30;

__device__ __forceinline__ int fm_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__global__ __launch_bounds__(256) void moments_accum_kernel(const float* __restrict__ rows, const float* __restrict__ pivot,
                                                            double* __restrict__ sum, double* __restrict__ gram, int n, int D,
                                                            int T) {
  __shared__ float xa[FM_ROWS * FM_TILE];
  __shared__ float xb[FM_ROWS * FM_TILE];
  // tile (ti, tj), ti <= tj, of the upper triangle in row-major order
  int t = blockIdx.x, ti = 0;
  while (t >= T - ti) { t -= T - ti; ++ti; }
  const int tj = ti + t;
  const bool diag = ti == tj;
  const int a0 = ti * FM_TILE, b0 = tj * FM_TILE;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int aw = wave >> 1, bw = wave & 1;
  // this thread loads column `lane` of both tiles, rows wave, wave + 4, ... of every chunk
  const bool in_a = a0 + lane < D, in_b = b0 + lane < D;
  const float pa = in_a ? pivot[a0 + lane] : 0.f, pb = in_b ? pivot[b0 + lane] : 0.f;
  f32x16 run;
  double tot[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { run[r] = 0.f; tot[r] = 0.0; }
  double colsum = 0.0;
  int chunk = 0;
  for (int r0 = 0; r0 < n; r0 += FM_ROWS) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FM_ROWS / 4; ++k) {
      const int r = wave + 4 * k;
      const bool in_r = r0 + r < n;
      const float* src = rows + (long long)(r0 + r) * D;
      xa[r * FM_TILE + lane] = (in_r && in_a) ? src[a0 + lane] - pa : 0.f;
      xb[r * FM_TILE + lane] = (in_r && in_b) ? src[b0 + lane] - pb : 0.f;
    }
    __syncthreads();
    if (diag && wave == 0)
#pragma unroll 8
      for (int r = 0; r < FM_ROWS; ++r) colsum += (double)xa[r * FM_TILE + lane];
    const float* a = xa + h * FM_TILE + aw * 32 + j;
    const float* b = xb + h * FM_TILE + bw * 32 + j;
#pragma unroll
    for (int st = 0; st < FM_ROWS / 2; ++st)
      run = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * st * FM_TILE], b[2 * st * FM_TILE], run, 0, 0, 0);
    if (++chunk == FM_DUMP) {
      chunk = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) { tot[r] += (double)run[r]; run[r] = 0.f; }
    }
  }
  if (chunk)
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] += (double)run[r];
  const int gb = b0 + bw * 32 + j;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ga = a0 + aw * 32 + fm_row(r, h);
    if (ga < D && gb < D) {
      gram[(long long)ga * D + gb] += tot[r];
      if (!diag) gram[(long long)gb * D + ga] += tot[r];
    }
  }
  if (diag && wave == 0 && in_a) sum[a0 + lane] += colsum;
}

}  // namespace

extern "C" int ganlab_moments_accum_f32(const float* rows, long long n, int D, const float* pivot, double* sum, double* gram,
                                        void* stream) {
  if (!rows || !pivot || !sum || !gram || n < 1 || D < 1) return GANLAB_EINVAL;
  if (n > FM_MAX_ROWS || D > FM_MAX_D) return GANLAB_EINVAL;
  const int T = (D + FM_TILE - 1) / FM_TILE;
  GL_LAUNCH(moments_accum_kernel, dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, gl_stream(stream), rows, pivot, sum, gram,
            (int)n, D, T);
  return GL_CHECK_LAUNCH();
}
