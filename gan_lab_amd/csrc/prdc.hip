// k-nearest-neighbour statistics between two sets of fp32 feature rows: improved precision / recall (Kynkaanniemi et al. 2019)
// and density / coverage (Naeem et al. 2020); composed in gan_lab_amd/prdc.py, DESIGN.md 4.16.  The N x M matrix of squared
// distances is never in memory: like attention.hip's forward, a workgroup owns a tile of query rows, walks all key tiles, forms
// the products on the exact-fp32 MFMA and reduces every tile per query row while it sits in the result registers - with "keep
// the k smallest" (knn) or "count those under a radius, keep the smallest and where it was" (cross) in the softmax's place.
//   d2[key][query] = max(|q|^2 + |k|^2 - 2 q.k, 0), the product as keys x queries on v_mfma_f32_32x32x2_f32: lane L supplies
//   A[i = L & 31][kk = L >> 5] = key i, B[kk][j = L & 31] = query j; the result sits at column j = L & 31, rows pr_row(r, L >> 5)
//   of register r.  A lane therefore owns ONE query and 16 keys of the tile: its k-list / count / minimum are per-lane scalars.
// The tile walk (pr_tiles.h) is shared with kid.hip.
// A workgroup is 2 x 2 waves over 64 queries x 64 keys; the depth D is walked in chunks of 32 through [row][33] LDS tiles (both
// operands are read down a column at stride 33: conflict free).  An fp32 MFMA accumulator is one k-ordered fmaf chain, so every
// PR_DUMP chunks (64 terms) the running chain is added into a second accumulator and restarts: chains of 64 terms summed by a
// chain of D / 64 partials.  The four lanes that share a query (2 lane halves x 2 key waves) are joined through LDS at the end, by
// one lane in a fixed order.  No atomics, nothing depends on the launch geometry: bitwise reproducible.  Tails in rows and depth
// are zero-filled on load and masked by index; the squared norms come from a kernel in front (fp64 sums in a fixed order).
#include "pr_tiles.h"
#include <math.h>

namespace {

__device__ __forceinline__ float pr_dist(float qn, float kn, float dot) { return fmaxf(fmaf(-2.f, dot, qn + kn), 0.f); }

// sorted insert into an ascending list: the largest value falls off the end
template <int KC>
__device__ __forceinline__ void pr_insert(float (&list)[KC], float v) {
#pragma unroll
  for (int i = 0; i < KC; ++i) {
    const float lo = fminf(list[i], v);
    v = fmaxf(list[i], v);
    list[i] = lo;
  }
}

// ---- |x_row|^2: one wave per row, fp64 partial per lane (columns lane, lane + 64, ...), fixed xor tree -------------------------
__global__ __launch_bounds__(256) void prdc_norms_kernel(const float* __restrict__ x, float* __restrict__ out, int rows, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* p = x + (long long)row * D;
  double acc = 0.0;
  for (int c = lane; c < D; c += 64) acc += (double)p[c] * (double)p[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) out[row] = (float)acc;
}

// ---- the k smallest squared distances of every row to the OTHER rows of its set, ascending ------------------------------------
// KC: the list's capacity in registers (>= k); the first k entries of the KC smallest are the k smallest
template <int KC>
__global__ __launch_bounds__(256) void prdc_knn_kernel(const float* __restrict__ x, const float* __restrict__ nrm,
                                                       float* __restrict__ out, int N, int D, int k) {
  __shared__ float smem[PR_SMEM];
  __shared__ float kn[PR_TILE];
  float* qs = smem;
  float* ks = smem + PR_TILE * PR_LD;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int qw = wave >> 1, kw = wave & 1;
  const int q0 = blockIdx.x * PR_TILE, qi = q0 + qw * 32 + j;
  const float qn = qi < N ? nrm[qi] : 0.f;
  float list[KC];
#pragma unroll
  for (int i = 0; i < KC; ++i) list[i] = INFINITY;
  for (int k0 = 0; k0 < N; k0 += PR_TILE) {
    __syncthreads();
    if (threadIdx.x < PR_TILE) kn[threadIdx.x] = k0 + (int)threadIdx.x < N ? nrm[k0 + threadIdx.x] : 0.f;
    const f32x16 dot = pr_dots(qs, ks, x, x, N, N, D, q0, k0, qw, kw, j, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kl = kw * 32 + pr_row(r, h), key = k0 + kl;
      float d = pr_dist(qn, kn[kl], dot[r]);
      if (key >= N || key == qi) d = INFINITY;               // the row itself is excluded by index, a duplicate elsewhere counts
      if (d < list[KC - 1]) pr_insert(list, d);
    }
  }
  __syncthreads();
  float* mine = smem + threadIdx.x * KC;
#pragma unroll
  for (int i = 0; i < KC; ++i) mine[i] = list[i];
  __syncthreads();
  if (kw != 0 || h != 0 || qi >= N) return;
#pragma unroll
  for (int s = 1; s < 4; ++s) {                              // (key wave, lane half) = (0, 1), (1, 0), (1, 1)
    const float* other = smem + (((qw * 2 + (s >> 1)) * 64) + (s & 1) * 32 + j) * KC;
#pragma unroll
    for (int i = 0; i < KC; ++i) pr_insert(list, other[i]);
  }
#pragma unroll
  for (int i = 0; i < KC; ++i)
    if (i < k) out[(long long)qi * k + i] = list[i];
}

// ---- queries (M, D) against keys (N, D): keys inside a radius, the nearest key and its squared distance ------------------------
// KEY_RAD: the radius belongs to the key (rad[i], N of them), else to the query (rad[j], M of them); <= counts as inside
template <bool KEY_RAD>
__global__ __launch_bounds__(256) void prdc_cross_kernel(const float* __restrict__ q, const float* __restrict__ qnrm,
                                                         const float* __restrict__ keys, const float* __restrict__ knrm,
                                                         const float* __restrict__ rad, int* __restrict__ count,
                                                         float* __restrict__ dmin, int* __restrict__ imin, int M, int N, int D) {
  __shared__ float smem[PR_SMEM];
  __shared__ float kn[PR_TILE];
  __shared__ float krad[PR_TILE];
  float* qs = smem;
  float* ks = smem + PR_TILE * PR_LD;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int qw = wave >> 1, kw = wave & 1;
  const int q0 = blockIdx.x * PR_TILE, qi = q0 + qw * 32 + j;
  const float qn = qi < M ? qnrm[qi] : 0.f;
  const float qrad = (!KEY_RAD && qi < M) ? rad[qi] : 0.f;
  int cnt = 0, bi = 0x7fffffff;
  float best = INFINITY;
  for (int k0 = 0; k0 < N; k0 += PR_TILE) {
    __syncthreads();
    if (threadIdx.x < PR_TILE) {
      const bool in = k0 + (int)threadIdx.x < N;
      kn[threadIdx.x] = in ? knrm[k0 + threadIdx.x] : 0.f;
      krad[threadIdx.x] = (KEY_RAD && in) ? rad[k0 + threadIdx.x] : 0.f;
    }
    const f32x16 dot = pr_dots(qs, ks, q, keys, M, N, D, q0, k0, qw, kw, j, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {                           // keys ascending in r: a strict < keeps the lowest index of a tie
      const int kl = kw * 32 + pr_row(r, h), key = k0 + kl;
      const float d = pr_dist(qn, kn[kl], dot[r]);
      if (key < N) {
        cnt += d <= (KEY_RAD ? krad[kl] : qrad) ? 1 : 0;
        if (d < best) { best = d; bi = key; }
      }
    }
  }
  __syncthreads();
  float* mbest = smem;
  int* mcnt = reinterpret_cast<int*>(smem + 256);
  int* midx = reinterpret_cast<int*>(smem + 512);
  mbest[threadIdx.x] = best;
  mcnt[threadIdx.x] = cnt;
  midx[threadIdx.x] = bi;
  __syncthreads();
  if (kw != 0 || h != 0 || qi >= M) return;
#pragma unroll
  for (int s = 1; s < 4; ++s) {
    const int t = ((qw * 2 + (s >> 1)) * 64) + (s & 1) * 32 + j;
    cnt += mcnt[t];
    if (mbest[t] < best || (mbest[t] == best && midx[t] < bi)) { best = mbest[t]; bi = midx[t]; }
  }
  count[qi] = cnt;
  dmin[qi] = best;
  imin[qi] = bi;
}

bool pr_shape_ok(long long rows, int D) { return rows >= 1 && rows <= PR_MAX_ROWS && D >= 1; }

}  // namespace

extern "C" {

int ganlab_prdc_norms_f32(const float* x, float* out, long long rows, int D, void* stream) {
  if (!x || !out || rows < 1 || D < 1) return GANLAB_EINVAL;
  if (!pr_shape_ok(rows, D)) return GANLAB_EUNSUPPORTED;
  GL_LAUNCH(prdc_norms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, gl_stream(stream), x, out, (int)rows, D);
  return GL_CHECK_LAUNCH();
}

int ganlab_prdc_knn_f32(const float* x, const float* norms, float* out, long long N, int D, int k, void* stream) {
  if (!x || !norms || !out || N < 1 || D < 1) return GANLAB_EINVAL;
  if (k < 1 || k > GANLAB_PRDC_MAX_K || k >= N) return GANLAB_EINVAL;
  if (!pr_shape_ok(N, D)) return GANLAB_EUNSUPPORTED;
  const dim3 grid((unsigned)((N + PR_TILE - 1) / PR_TILE));
  hipStream_t st = gl_stream(stream);
  if (k <= 4) GL_LAUNCH(prdc_knn_kernel<4>, grid, dim3(256), 0, st, x, norms, out, (int)N, D, k);
  else if (k <= 8) GL_LAUNCH(prdc_knn_kernel<8>, grid, dim3(256), 0, st, x, norms, out, (int)N, D, k);
  else GL_LAUNCH(prdc_knn_kernel<16>, grid, dim3(256), 0, st, x, norms, out, (int)N, D, k);
  return GL_CHECK_LAUNCH();
}

int ganlab_prdc_cross_f32(const float* queries, const float* query_norms, const float* keys, const float* key_norms,
                          const float* radii, int radius_of_query, int* count, float* dmin, int* imin, long long M, long long N,
                          int D, void* stream) {
  if (!queries || !query_norms || !keys || !key_norms || !radii || !count || !dmin || !imin) return GANLAB_EINVAL;
  if (M < 1 || N < 1 || D < 1 || (radius_of_query != 0 && radius_of_query != 1)) return GANLAB_EINVAL;
  if (!pr_shape_ok(M, D) || !pr_shape_ok(N, D)) return GANLAB_EUNSUPPORTED;
  const dim3 grid((unsigned)((M + PR_TILE - 1) / PR_TILE));
  hipStream_t st = gl_stream(stream);
  if (radius_of_query)
    GL_LAUNCH(prdc_cross_kernel<false>, grid, dim3(256), 0, st, queries, query_norms, keys, key_norms, radii, count, dmin, imin,
              (int)M, (int)N, D);
  else
    GL_LAUNCH(prdc_cross_kernel<true>, grid, dim3(256), 0, st, queries, query_norms, keys, key_norms, radii, count, dmin, imin,
              (int)M, (int)N, D);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
