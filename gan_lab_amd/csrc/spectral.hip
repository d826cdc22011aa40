// Spectral normalisation of ALL weights of a critic in a handful of launches (Miyato et al. 2018; the arithmetic of
// torch.nn.utils.spectral_norm with one power iteration).  A device-resident job table (ganlab_sn_job, built and uploaded
// once per arena build by gan_lab_amd/ops.py, like pack.hip's descriptor table) names, per layer, the parameter W viewed
// as Wm = (R, K) row-major, the normalised copy W_sn the convolutions read, its gradient, the parameter's gradient, the
// stored u (R) / v (K) / sigma and three scratch areas.  Every pass is ONE launch over the blocks of all layers: a block
// finds its job by binary search over that pass's block offsets.
//   refresh, iterate:   T   tpart[c][k] = sum_{r in row chunk c} u[r] Wm[r][k]            (SN_RC rows per chunk)
//                       V   t = sum_c tpart[c] ; v = t / max(|t|, eps)                    (one block per layer)
//                       S   s[r] = sum_k Wm[r][k] v[k]                                    (one wave per row)
//                       N   u = s / max(|s|, eps) ; sigma = sum_r u[r] s[r] ; W_sn = W / sigma
//   refresh, no iterate: S with the stored v, then N with the stored u (sigma and W_sn follow the moved weights)
//   backward:           D   dpart[b] = sum over elementwise block b of g_sn * W_sn
//                       G   d = sum_b dpart[b] ; gW += (g_sn - d u v^T) / sigma
// All sums run in a fixed order (thread-serial chains, xor-shuffle trees, block partials added in index order, every block
// of a layer re-deriving the layer's scalars from the same partials with the same code): no floating-point atomics, results
// are bitwise reproducible.  Nothing is read back by the host.  Rows are read with 16-byte loads where K % 4 == 0 (every
// slot is 16-byte aligned, so each row is); other K (27: the first conv; odd test shapes) take the scalar path.
#include "common.h"

namespace {

constexpr int SN_RC = GANLAB_SN_ROW_CHUNK;      // rows per partial of pass T
constexpr int SN_TC = GANLAB_SN_COL_TILE;       // columns per block of pass T (256 threads x 4)
constexpr int SN_EB = GANLAB_SN_ELEM_BLOCK;     // elements per block of the elementwise passes (256 threads x 2 x 4)

enum { BLK_T = 0, BLK_S = 1, BLK_E = 2 };

template <int WHICH>
__device__ __forceinline__ long long sn_block0(const ganlab_sn_job& j) {
  return WHICH == BLK_T ? j.blk_t0 : (WHICH == BLK_S ? j.blk_s0 : j.blk_e0);
}

// last job whose first block of pass WHICH is <= b
template <int WHICH>
__device__ __forceinline__ int sn_find(const ganlab_sn_job* __restrict__ jobs, int n, long long b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sn_block0<WHICH>(jobs[mid]) <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- T: partial column sums of u^T Wm over SN_RC rows -----------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_t_kernel(const ganlab_sn_job* __restrict__ jobs, int n_jobs) {
  const ganlab_sn_job j = jobs[sn_find<BLK_T>(jobs, n_jobs, blockIdx.x)];
  const int lb = (int)(blockIdx.x - j.blk_t0);
  const int nct = (j.K + SN_TC - 1) / SN_TC;
  const int rc = lb / nct, ct = lb - rc * nct;
  const int r0 = rc * SN_RC, r1 = min(r0 + SN_RC, j.R);
  if (r0 >= j.R) return;
  float* out = j.tpart + (long long)rc * j.K;
  if ((j.K & 3) == 0) {
    const int k = ct * SN_TC + threadIdx.x * 4;
    if (k >= j.K) return;
    float4 a = float4{0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; ++r) {
      const float ur = j.u[r];
      const float4 w = *reinterpret_cast<const float4*>(j.w + (long long)r * j.K + k);
      a.x += ur * w.x; a.y += ur * w.y; a.z += ur * w.z; a.w += ur * w.w;
    }
    *reinterpret_cast<float4*>(out + k) = a;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = ct * SN_TC + q * 256 + threadIdx.x;
      if (k >= j.K) continue;
      float a = 0.f;
      for (int r = r0; r < r1; ++r) a += j.u[r] * j.w[(long long)r * j.K + k];
      out[k] = a;
    }
  }
}

// ---- V: t = sum of the partials, v = t / max(|t|, eps); one block per layer ---------------------------------------------
__global__ __launch_bounds__(256) void sn_v_kernel(const ganlab_sn_job* __restrict__ jobs, int n_jobs, float eps) {
  __shared__ float red[4];
  if ((int)blockIdx.x >= n_jobs) return;
  const ganlab_sn_job j = jobs[blockIdx.x];
  const int nrc = (j.R + SN_RC - 1) / SN_RC;
  float sq = 0.f;
  for (int k = threadIdx.x; k < j.K; k += 256) {
    float t = 0.f;
    for (int c = 0; c < nrc; ++c) t += j.tpart[(long long)c * j.K + k];
    j.v[k] = t;                      // re-read below by the thread that wrote it
    sq += t * t;
  }
  sq = gl_block_sum_256(sq, red);
  const float den = fmaxf(sqrtf(sq), eps);
  for (int k = threadIdx.x; k < j.K; k += 256) j.v[k] = j.v[k] / den;
}

// ---- S: s = Wm v, one wave per row ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_s_kernel(const ganlab_sn_job* __restrict__ jobs, int n_jobs) {
  const ganlab_sn_job j = jobs[sn_find<BLK_S>(jobs, n_jobs, blockIdx.x)];
  const int r = (int)(blockIdx.x - j.blk_s0) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= j.R) return;
  const float* row = j.w + (long long)r * j.K;
  float a = 0.f;
  if ((j.K & 3) == 0) {
    for (int k = lane * 4; k < j.K; k += 256) {
      const float4 w = *reinterpret_cast<const float4*>(row + k);
      const float4 v = *reinterpret_cast<const float4*>(j.v + k);
      a += (w.x * v.x + w.y * v.y) + (w.z * v.z + w.w * v.w);
    }
  } else {
    for (int k = lane; k < j.K; k += 64) a += row[k] * j.v[k];
  }
  a = gl_wave_sum(a);
  if (lane == 0) j.s[r] = a;
}

// ---- N: (u, sigma) from s, then W_sn = W / sigma over this block's elements --------------------------------------------------
__global__ __launch_bounds__(256) void sn_n_kernel(const ganlab_sn_job* __restrict__ jobs, int n_jobs, int iterate, float eps) {
  __shared__ float red[4];
  const ganlab_sn_job j = jobs[sn_find<BLK_E>(jobs, n_jobs, blockIdx.x)];
  const long long lb = blockIdx.x - j.blk_e0;
  // every block of the layer derives the same scalars from the same s with the same code: bit-identical, no hand-off
  float den = 1.f;
  if (iterate) {
    float sq = 0.f;
    for (int r = threadIdx.x; r < j.R; r += 256) sq += j.s[r] * j.s[r];
    den = fmaxf(sqrtf(gl_block_sum_256(sq, red)), eps);
  }
  float dot = 0.f;
  for (int r = threadIdx.x; r < j.R; r += 256) {
    const float sr = j.s[r];
    const float ur = iterate ? sr / den : j.u[r];
    dot += ur * sr;
  }
  const float sigma = gl_block_sum_256(dot, red);
  if (lb == 0) {                     // (the other blocks read s, never u: no ordering needed)
    if (iterate)
      for (int r = threadIdx.x; r < j.R; r += 256) j.u[r] = j.s[r] / den;
    if (threadIdx.x == 0) j.sigma[0] = sigma;
  }
  const long long total = (long long)j.R * j.K;
  if ((j.K & 3) == 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const long long e = lb * SN_EB + (q * 256 + threadIdx.x) * 4;
      if (e >= total) continue;
      float4 w = *reinterpret_cast<const float4*>(j.w + e);
      w.x /= sigma; w.y /= sigma; w.z /= sigma; w.w /= sigma;
      *reinterpret_cast<float4*>(j.w_sn + e) = w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long e = lb * SN_EB + q * 256 + threadIdx.x;
      if (e < total) j.w_sn[e] = j.w[e] / sigma;
    }
  }
}

// ---- D: per-block partial of <g_sn, W_sn> -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_d_kernel(const ganlab_sn_job* __restrict__ jobs, int n_jobs) {
  __shared__ float red[4];
  const ganlab_sn_job j = jobs[sn_find<BLK_E>(jobs, n_jobs, blockIdx.x)];
  const long long lb = blockIdx.x - j.blk_e0;
  const long long total = (long long)j.R * j.K;
  float a = 0.f;
  if ((j.K & 3) == 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const long long e = lb * SN_EB + (q * 256 + threadIdx.x) * 4;
      if (e >= total) continue;
      const float4 g = *reinterpret_cast<const float4*>(j.g_sn + e);
      const float4 w = *reinterpret_cast<const float4*>(j.w_sn + e);
      a += (g.x * w.x + g.y * w.y) + (g.z * w.z + g.w * w.w);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long e = lb * SN_EB + q * 256 + threadIdx.x;
      if (e < total) a += j.g_sn[e] * j.w_sn[e];
    }
  }
  a = gl_block_sum_256(a, red);
  if (threadIdx.x == 0) j.dpart[lb] = a;
}

// ---- G: gW += (g_sn - <g_sn, W_sn> u v^T) / sigma ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_g_kernel(const ganlab_sn_job* __restrict__ jobs, int n_jobs) {
  __shared__ float red[4];
  const ganlab_sn_job j = jobs[sn_find<BLK_E>(jobs, n_jobs, blockIdx.x)];
  const long long lb = blockIdx.x - j.blk_e0;
  const long long total = (long long)j.R * j.K;
  const int nb = (int)((total + SN_EB - 1) / SN_EB);
  float a = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) a += j.dpart[i];
  const float d = gl_block_sum_256(a, red);
  const float sigma = j.sigma[0];
  if ((j.K & 3) == 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const long long e = lb * SN_EB + (q * 256 + threadIdx.x) * 4;
      if (e >= total) continue;
      const int r = (int)(e / j.K), k = (int)(e - (long long)r * j.K);
      const float du = d * j.u[r];
      const float4 g = *reinterpret_cast<const float4*>(j.g_sn + e);
      const float4 v = *reinterpret_cast<const float4*>(j.v + k);
      float4 o = *reinterpret_cast<const float4*>(j.gw + e);
      o.x += (g.x - du * v.x) / sigma; o.y += (g.y - du * v.y) / sigma;
      o.z += (g.z - du * v.z) / sigma; o.w += (g.w - du * v.w) / sigma;
      *reinterpret_cast<float4*>(j.gw + e) = o;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long e = lb * SN_EB + q * 256 + threadIdx.x;
      if (e >= total) continue;
      const int r = (int)(e / j.K), k = (int)(e - (long long)r * j.K);
      j.gw[e] += (j.g_sn[e] - d * j.u[r] * j.v[k]) / sigma;
    }
  }
}

bool sn_grid_ok(long long b) { return b > 0 && b <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int ganlab_sn_job_size(void) { return (int)sizeof(ganlab_sn_job); }

int ganlab_sn_refresh(const ganlab_sn_job* jobs_device, int n_layers, long long blocks_t, long long blocks_s,
                      long long blocks_e, int iterate, float eps, void* stream) {
  if (!jobs_device || n_layers <= 0 || !sn_grid_ok(blocks_t) || !sn_grid_ok(blocks_s) || !sn_grid_ok(blocks_e))
    return GANLAB_EINVAL;
  hipStream_t st = gl_stream(stream);
  if (iterate) {
    GL_LAUNCH(sn_t_kernel, dim3((unsigned)blocks_t), dim3(256), 0, st, jobs_device, n_layers);
    GL_LAUNCH(sn_v_kernel, dim3((unsigned)n_layers), dim3(256), 0, st, jobs_device, n_layers, eps);
  }
  GL_LAUNCH(sn_s_kernel, dim3((unsigned)blocks_s), dim3(256), 0, st, jobs_device, n_layers);
  GL_LAUNCH(sn_n_kernel, dim3((unsigned)blocks_e), dim3(256), 0, st, jobs_device, n_layers, iterate ? 1 : 0, eps);
  return GL_CHECK_LAUNCH();
}

int ganlab_sn_backward(const ganlab_sn_job* jobs_device, int n_layers, long long blocks_e, void* stream) {
  if (!jobs_device || n_layers <= 0 || !sn_grid_ok(blocks_e)) return GANLAB_EINVAL;
  hipStream_t st = gl_stream(stream);
  GL_LAUNCH(sn_d_kernel, dim3((unsigned)blocks_e), dim3(256), 0, st, jobs_device, n_layers);
  GL_LAUNCH(sn_g_kernel, dim3((unsigned)blocks_e), dim3(256), 0, st, jobs_device, n_layers);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
