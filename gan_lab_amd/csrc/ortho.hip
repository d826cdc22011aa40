// BigGAN's orthogonal regulariser (Brock et al. 2019, eq. 3) for ALL weights of a network in three launches.  For a parameter
// W viewed as Wm = (R, K) row-major and M = (Wm Wm^T) o (1 - I):
//   penalty = beta * sum(M^2) ;  gW += 4 * beta * M Wm                 (the derivative of the penalty; accumulated)
// A device-resident job table (ganlab_ortho_job, built and uploaded once per arena build by gan_lab_amd/ops.py, like
// spectral.hip's) names, per layer, the parameter, its gradient slot, the form and the scratch.  The (R, R) matrix is never
// formed when R > K: each layer takes the association with the smaller middle dimension m = min(R, K)
//   row form    (R <= K):  S = Wm Wm^T (R, R), diagonal zeroed at the store ;  G = S Wm ;           sum(M^2) = sum(S^2)
//   column form (K <  R):  S = Wm^T Wm (K, K), q[r] = |Wm[r,:]|^2 ;            G = Wm S - q o Wm ;  sum(M^2) = sum(S^2) - sum(q^2)
// Every pass is ONE launch over the blocks of all layers; a block finds its job by binary search over that pass's block offsets.
//   Gram    one 64 x 64 tile of S per block (+ in column form blocks of 4 rows of q, one wave per row); part[block] = the
//           block's sum of squares
//   apply   one 64 x 64 tile of G per block, gW += 4 beta (...)
//   tail    one block: per layer the partials in index order (fp64) -> penalty, and their running sum -> the total
// Both products run on v_mfma_f32_32x32x2_f32 (operand / result layout: attention.hip), a wave per 32 x 32 quarter of the tile,
// the contraction in chunks of 32 staged through LDS: A as [i][33] (read down a column of k: conflict free), B as [k][65]
// (read along a row).  Rows / columns / contraction indices past the matrix are zero-filled on load and masked on store.  An
// fp32 MFMA accumulator is one k-ordered chain: every 128 terms it is added into a second accumulator and restarts from zero
// (common.h "Accumulation chains").  Loads are 16 bytes wide where the source's row length is a multiple of 4 (every slot and
// scratch area is 16-byte aligned, so each row then is), scalar otherwise (K = 27, odd test shapes).
// Every sum runs in a fixed order and nothing is atomic: results are bitwise reproducible.  Nothing is read back by the host.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int OR_T = GANLAB_ORTHO_TILE;       // output tile edge
constexpr int OR_KC = 32;                     // contraction chunk
constexpr int OR_LDA = OR_KC + 1;             // LDS row stride of the A tile [i][k]
constexpr int OR_LDB = OR_T + 1;              // LDS row stride of the B tile [k][j]
constexpr int OR_DUMP = 4;                    // chunks per accumulation chain (128 terms)
constexpr int OR_QR = GANLAB_ORTHO_QROWS;     // rows of q per block (one wave each)
static_assert(OR_T == 64 && OR_QR == 4, "a 256-thread block is 2 x 2 waves of 32 x 32 results, or 4 waves of one row");

enum { BLK_G = 0, BLK_A = 1 };

// last job whose first block of pass WHICH is <= b
template <int WHICH>
__device__ __forceinline__ int or_find(const ganlab_ortho_job* __restrict__ jobs, int n, long long b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((WHICH == BLK_G ? jobs[mid].blk_g0 : jobs[mid].blk_a0) <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// row of result register r in lane half h (v_mfma_f32_32x32x2_f32)
__device__ __forceinline__ int or_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 or_zero() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// LDS tile <- rows [p0, p0 + P) x columns [q0, q0 + Q) of the row-major (nrows, ld) matrix src, zero outside;
// TR ? lds[q][p] : lds[p][q] with row stride LD.  p0, q0 are multiples of 32.
template <int P, int Q, bool TR, int LD>
__device__ __forceinline__ void or_load(float* lds, const float* __restrict__ src, int nrows, int ld, int p0, int q0) {
  if ((ld & 3) == 0) {
    for (int idx = threadIdx.x; idx < P * Q / 4; idx += 256) {
      const int p = idx / (Q / 4), q = (idx - p * (Q / 4)) * 4;
      float4 v = float4{0.f, 0.f, 0.f, 0.f};
      if (p0 + p < nrows && q0 + q < ld)       // ld % 4 == 0: the four columns are in or out together
        v = *reinterpret_cast<const float4*>(src + (long long)(p0 + p) * ld + q0 + q);
      if (TR) {
        lds[(q + 0) * LD + p] = v.x; lds[(q + 1) * LD + p] = v.y; lds[(q + 2) * LD + p] = v.z; lds[(q + 3) * LD + p] = v.w;
      } else {
        lds[p * LD + q + 0] = v.x; lds[p * LD + q + 1] = v.y; lds[p * LD + q + 2] = v.z; lds[p * LD + q + 3] = v.w;
      }
    }
  } else {
    for (int idx = threadIdx.x; idx < P * Q; idx += 256) {
      const int p = idx / Q, q = idx - p * Q;
      float v = 0.f;
      if (p0 + p < nrows && q0 + q < ld) v = src[(long long)(p0 + p) * ld + q0 + q];
      lds[TR ? q * LD + p : p * LD + q] = v;
    }
  }
}

// This wave's 32 x 32 quarter of C[i0 + i][j0 + j] = sum_{k < klen} A(i, k) B(k, j), i, j in [0, 64).
//   TA ? A(i, k) = a[k * a_ld + i] : a[i * a_ld + k] ;  TB ? B(k, j) = b[j * b_ld + k] : b[k * b_ld + j]
// a, b are row-major with a_rows / b_rows rows of a_ld / b_ld floats.  Called by all 256 threads of the block.
template <bool TA, bool TB>
__device__ __forceinline__ f32x16 or_tile(float* as, float* bs, const float* __restrict__ a, int a_rows, int a_ld,
                                          const float* __restrict__ b, int b_rows, int b_ld, int i0, int j0, int klen) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, jl = lane & 31, h = lane >> 5;
  const float* ar = as + ((wave >> 1) * 32 + jl) * OR_LDA + h;
  const float* br = bs + h * OR_LDB + (wave & 1) * 32 + jl;
  f32x16 acc = or_zero(), tot = or_zero();
  int chunk = 0;
  for (int k0 = 0; k0 < klen; k0 += OR_KC) {
    __syncthreads();
    if (TA) or_load<OR_KC, OR_T, true, OR_LDA>(as, a, a_rows, a_ld, k0, i0);
    else    or_load<OR_T, OR_KC, false, OR_LDA>(as, a, a_rows, a_ld, i0, k0);
    if (TB) or_load<OR_T, OR_KC, true, OR_LDB>(bs, b, b_rows, b_ld, j0, k0);
    else    or_load<OR_KC, OR_T, false, OR_LDB>(bs, b, b_rows, b_ld, k0, j0);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < OR_KC / 2; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[2 * kk], br[2 * kk * OR_LDB], acc, 0, 0, 0);
    if (++chunk == OR_DUMP) {
      chunk = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) tot[r] += acc[r];
      acc = or_zero();
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) tot[r] += acc[r];
  return tot;
}

__device__ __forceinline__ int or_m(const ganlab_ortho_job& j) { return j.form == GANLAB_ORTHO_ROW ? j.R : j.K; }

// ---- Gram: a tile of S (+ the diagonal mask / q) and the block's sum of squares ------------------------------------------------
__global__ __launch_bounds__(256) void ortho_gram_kernel(const ganlab_ortho_job* __restrict__ jobs, int n_jobs) {
  __shared__ float as[OR_T * OR_LDA];
  __shared__ float bs[OR_KC * OR_LDB];
  __shared__ float red[4];
  const ganlab_ortho_job j = jobs[or_find<BLK_G>(jobs, n_jobs, blockIdx.x)];
  const int lb = (int)(blockIdx.x - j.blk_g0);
  if (lb >= j.n_part) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, jl = lane & 31, h = lane >> 5;
  const int m = or_m(j), tm = (m + OR_T - 1) / OR_T;
  if (lb >= tm * tm) {                        // column form: q of OR_QR rows, one wave per row
    const int r = (lb - tm * tm) * OR_QR + wave;
    float a = 0.f;
    if (r < j.R) {
      const float* row = j.w + (long long)r * j.K;
      for (int k = lane; k < j.K; k += 64) a += row[k] * row[k];
    }
    a = gl_wave_sum(a);
    if (lane == 0) {
      if (r < j.R) j.q[r] = a;
      red[wave] = a * a;                       // rows past R: 0
    }
    __syncthreads();
    if (threadIdx.x == 0) j.part[lb] = ((red[0] + red[1]) + red[2]) + red[3];
    return;
  }
  const int ti = lb / tm, tj = lb - ti * tm;
  const int i0 = ti * OR_T, j0 = tj * OR_T;
  const bool rowf = j.form == GANLAB_ORTHO_ROW;
  const f32x16 c = rowf ? or_tile<false, true>(as, bs, j.w, j.R, j.K, j.w, j.R, j.K, i0, j0, j.K)
                        : or_tile<true, false>(as, bs, j.w, j.R, j.K, j.w, j.R, j.K, i0, j0, j.R);
  const int col = j0 + (wave & 1) * 32 + jl;
  float ss = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = i0 + (wave >> 1) * 32 + or_row(r, h);
    if (row < m && col < m) {
      const float v = (rowf && row == col) ? 0.f : c[r];
      j.s[(long long)row * m + col] = v;
      ss += v * v;
    }
  }
  ss = gl_block_sum_256(ss, red);
  if (threadIdx.x == 0) j.part[lb] = ss;
}

// ---- apply: gW += scale * (S Wm)  |  scale * (Wm S - q o Wm) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void ortho_apply_kernel(const ganlab_ortho_job* __restrict__ jobs, int n_jobs, float scale) {
  __shared__ float as[OR_T * OR_LDA];
  __shared__ float bs[OR_KC * OR_LDB];
  const ganlab_ortho_job j = jobs[or_find<BLK_A>(jobs, n_jobs, blockIdx.x)];
  const int lb = (int)(blockIdx.x - j.blk_a0);
  const int tk = (j.K + OR_T - 1) / OR_T, tr = (j.R + OR_T - 1) / OR_T;
  if (lb >= tr * tk) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, jl = lane & 31, h = lane >> 5;
  const int ti = lb / tk, tj = lb - ti * tk;
  const int i0 = ti * OR_T, j0 = tj * OR_T;
  const bool rowf = j.form == GANLAB_ORTHO_ROW;
  const f32x16 c = rowf ? or_tile<false, false>(as, bs, j.s, j.R, j.R, j.w, j.R, j.K, i0, j0, j.R)
                        : or_tile<false, false>(as, bs, j.w, j.R, j.K, j.s, j.K, j.K, i0, j0, j.K);
  const int col = j0 + (wave & 1) * 32 + jl;
  if (col >= j.K) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = i0 + (wave >> 1) * 32 + or_row(r, h);
    if (row < j.R) {
      const long long e = (long long)row * j.K + col;
      float v = c[r];
      if (!rowf) v -= j.q[row] * j.w[e];
      j.gw[e] += scale * v;
    }
  }
}

// ---- tail: the partials of every layer, in index order, into its penalty and into the total ----------------------------------------
__global__ __launch_bounds__(256) void ortho_tail_kernel(const ganlab_ortho_job* __restrict__ jobs, int n_jobs, float beta,
                                                         float* __restrict__ total_out) {
  __shared__ double red[4];
  double total = 0.0;
  for (int l = 0; l < n_jobs; ++l) {
    const ganlab_ortho_job j = jobs[l];
    const int m = or_m(j), tm = (m + OR_T - 1) / OR_T, ng = tm * tm;
    double a = 0.0;
    for (int i = threadIdx.x; i < j.n_part; i += 256) a += i < ng ? (double)j.part[i] : -(double)j.part[i];
    a = gl_block_sum_256d(a, red);
    if (threadIdx.x == 0) j.penalty[0] = (float)((double)beta * a);
    total += a;
  }
  if (threadIdx.x == 0) total_out[0] = (float)((double)beta * total);
}

bool or_grid_ok(long long b) { return b > 0 && b <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int ganlab_ortho_job_size(void) { return (int)sizeof(ganlab_ortho_job); }

int ganlab_ortho_apply(const ganlab_ortho_job* jobs_device, int n_layers, long long blocks_gram, long long blocks_apply,
                       float beta, float* total_out, void* stream) {
  if (!jobs_device || !total_out || n_layers <= 0 || !or_grid_ok(blocks_gram) || !or_grid_ok(blocks_apply) || !(beta >= 0.f) ||
      !(beta <= 3.0e38f))
    return GANLAB_EINVAL;
  hipStream_t st = gl_stream(stream);
  GL_LAUNCH(ortho_gram_kernel, dim3((unsigned)blocks_gram), dim3(256), 0, st, jobs_device, n_layers);
  GL_LAUNCH(ortho_apply_kernel, dim3((unsigned)blocks_apply), dim3(256), 0, st, jobs_device, n_layers, 4.f * beta);
  GL_LAUNCH(ortho_tail_kernel, dim3(1), dim3(256), 0, st, jobs_device, n_layers, beta, total_out);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
