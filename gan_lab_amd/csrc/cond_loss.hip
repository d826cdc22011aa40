// Classifier-based class conditioning of the ResNet GAN critic (config.cgan = 'acgan' | 'contra' | 'reacgan'):
// AC-GAN's cross-entropy (Odena et al. 2017), ContraGAN's conditional contrastive loss "2C" (Kang & Park 2020) and ReACGAN's
// data-to-data cross-entropy "D2D-CE" (Kang et al. 2021).  labels: int32 (N,), clamped into [0, K) as in cond.hip.
//
// Cross-entropy on logits z (N, K):  l_i = LSE_k z_ik - z_{i,y_i};  dz_ik = g/N (softmax_ik - [k = y_i]).  One wave per row; the
// forward is ONE workgroup of 16 waves (rows wave-strided, fp64 partial per wave, the 16 partials added in index order), so the
// mean needs no second launch and no atomic; the backward is one wave per row over the whole device.
//
// Contrastive, h (N, E) the embeddings, P (K, E) the proxies; hh_i = h_i / max(|h_i|, 1e-12), ph_k likewise,
// s_i = hh_i . ph_{y_i}, S_ij = hh_i . hh_j, t = temperature:
//   2C      u_i = s_i/t, A_ij = S_ij/t (j != i);  D_i = LSE({u_i} u {A_ij}), M_i = LSE({u_i} u {A_ij: y_j = y_i});  l_i = D_i - M_i
//   D2D-CE  u_i = min(s_i - m_p, 0)/t, A_ij = max(S_ij - m_n, 0)/t over y_j != y_i;  D_i = LSE({u_i} u {A_ij});  l_i = D_i - u_i
// forward   cl_fwd_kernel: a workgroup of two waves owns 64 query rows (a wave 32 of them) and walks the N key rows in tiles of
//           64.  Rows are normalised as they are staged: a wave computes the inverse norm of each row it stages (lanes stride the
//           row, xor-shuffle tree - cl_inv_norm, the one routine every kernel here uses, so hh has the same bits everywhere) and
//           the tile is written to LDS as h * inv, E in chunks of 32, zero-padded.  The 64 x 64 tile of S^T is two 32 x 32
//           products per wave on v_mfma_f32_32x32x2_f32 with the QUERY in the result column (attention.hip's orientation), so a
//           query's running maxima and sums are per-lane scalars, joined across the lane halves by one xor-32 shuffle; masks,
//           clamps and both online log-sum-exps run in the result registers, S never reaches memory.  Both LSEs start from
//           (max = u_i, sum = 1), so they are finite for any row and a row without negatives gives l_i = 0 exactly.
//           Writes rows (4, N) = l, D, M, s.  cl_mean_kernel (one workgroup, fp64, fixed order) writes the mean.  2 launches.
// backward  cl_norm_kernel writes hh (N, E), 1/|h_i| and 1/|p_k| into the workspace; cl_bwd_kernel has the forward's ownership
//           and recomputes the tile of S from hh (the same bits as the forward's), forms
//             c_ij = a_ij + a_ji,   a_ij = dl_i/dS_ij from the row's saved D, M, a_ji from the key rows' (loaded per tile)
//           in the result registers and feeds them back as the B operand of a second product dhh^T[e][i] += hh[j][e] c[j][i]
//           (register r of the two lane halves holds keys at_row(r, 0) and at_row(r, 1): exactly the pair one MFMA contracts).
//           E is walked in blocks of 128 columns (4 accumulators); S is recomputed per block.  The rows of dhh are parked in dh,
//           then each wave finishes its rows: + b_i ph_{y_i}, the normalisation derivative (dhh - hh (hh . dhh)) / |h_i|, g/N.
//           cl_dproxy_kernel: one workgroup per class, dph_k = sum_{i: y_i = k} b_i hh_i with i ascending, every row written
//           (exact zeros for an absent class), then the same derivative.  3 launches.
// No atomics anywhere, every sum in a fixed order: two runs are bitwise equal.  Stream-ordered, nothing is read back.
#include "common.h"
#include <math.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int CL_LD = 33;            // LDS row stride of a 32-column chunk: rows at stride 33 and columns are both conflict free
constexpr int CL_TILE = 64;          // query rows per workgroup, key rows per tile
constexpr int CL_EBLOCK = 128;       // embedding columns per backward pass (4 accumulators of 32)
constexpr int CL_2C = 0, CL_D2D = 1;
constexpr float CL_EPS = 1e-12f;

__device__ __forceinline__ int cl_label(int l, int K) { return l < 0 ? 0 : (l >= K ? K - 1 : l); }
__device__ __forceinline__ f32x16 cl_mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of result register r in lane half h
__device__ __forceinline__ int cl_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ f32x16 cl_zero() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}
__device__ __forceinline__ float cl_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// 1 / max(|row|, eps) by one wave, the same value in every lane: lanes stride the row, fmaf chains, xor tree
__device__ __forceinline__ float cl_inv_norm(const float* __restrict__ row, int E, int lane) {
  float a = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float v = row[e];
    a = fmaf(v, v, a);
  }
  a = gl_wave_sum(a);
  return 1.0f / fmaxf(sqrtf(a), CL_EPS);
}

// LDS chunk [64][CL_LD] <- src[r0 + r][e0 .. e0 + 32) * inv[r] (inv == nullptr: as it is) for r0 + r < rows, zero outside
__device__ __forceinline__ void cl_stage(float* lds, const float* __restrict__ src, const float* inv, int r0, int rows, int E,
                                         int e0) {
  for (int idx = threadIdx.x; idx < CL_TILE * 32; idx += 128) {
    const int r = idx >> 5, c = idx & 31;
    float v = 0.f;
    if (r0 + r < rows && e0 + c < E) {
      v = src[(long long)(r0 + r) * E + e0 + c];
      if (inv != nullptr) v *= inv[r];
    }
    lds[r * CL_LD + c] = v;
  }
}

// S^T[key = kh * 32 + cl_row(r, h)][query = wave * 32 + j] += sum over the staged chunk
__device__ __forceinline__ void cl_tile_dot(f32x16 (&acc)[2], const float* qs, const float* ks, int wave, int j, int h) {
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    const float b = qs[(wave * 32 + j) * CL_LD + 2 * st + h];
    acc[0] = cl_mfma(ks[j * CL_LD + 2 * st + h], b, acc[0]);
    acc[1] = cl_mfma(ks[(32 + j) * CL_LD + 2 * st + h], b, acc[1]);
  }
}

// dl_i/ds_i from the row's saved statistics
template <int MODE>
__device__ __forceinline__ float cl_b(float s, float D, float M, float inv_tau, float mp) {
  if (MODE == CL_2C) {
    const float u = s * inv_tau;
    return (expf(u - D) - expf(u - M)) * inv_tau;
  }
  return s < mp ? (expf((s - mp) * inv_tau - D) - 1.0f) * inv_tau : 0.f;
}

// ---- cross-entropy -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ce_fwd_kernel(const float* __restrict__ z, const int* __restrict__ labels,
                                                      float* __restrict__ loss, float* __restrict__ lse, int N, int K) {
  __shared__ double part[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc = 0.0;
  for (int i = wave; i < N; i += 16) {
    const float* row = z + (long long)i * K;
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, row[k]);
    m = cl_wave_max(m);
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += expf(row[k] - m);
    s = gl_wave_sum(s);
    const float l = m + logf(s);
    if (lane == 0) lse[i] = l;
    acc += (double)(l - row[cl_label(labels[i], K)]);
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += part[w];
    loss[0] = (float)(t / (double)N);
  }
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ z, const int* __restrict__ labels,
                                                     const float* __restrict__ lse, const float* __restrict__ gout,
                                                     float* __restrict__ dz, int N, int K) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N) return;
  const float g = gout[0] / (float)N, l = lse[i];
  const int y = cl_label(labels[i], K);
  const float* row = z + (long long)i * K;
  float* out = dz + (long long)i * K;
  for (int k = lane; k < K; k += 64) out[k] = g * (expf(row[k] - l) - (k == y ? 1.0f : 0.f));
}

// ---- contrastive forward -------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(128) void cl_fwd_kernel(const float* __restrict__ hmat, const float* __restrict__ proxy,
                                                     const int* __restrict__ labels, float* __restrict__ rows, int N, int E, int K,
                                                     float inv_tau, float mp, float mn) {
  __shared__ float qs[CL_TILE * CL_LD];
  __shared__ float ks[CL_TILE * CL_LD];
  __shared__ float qinv[CL_TILE], kinv[CL_TILE], qsim[CL_TILE];
  __shared__ int klab[CL_TILE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int i0 = blockIdx.x * CL_TILE;
  // the wave's 32 query rows: 1/|h_i| and s_i = (h_i . p_y) / (|h_i| |p_y|)
  for (int rr = 0; rr < 32; ++rr) {
    const int slot = wave * 32 + rr, row = i0 + slot;
    float inv = 0.f, s = 0.f;
    if (row < N) {
      const float* hr = hmat + (long long)row * E;
      const float* pr = proxy + (long long)cl_label(labels[row], K) * E;
      inv = cl_inv_norm(hr, E, lane);
      const float pinv = cl_inv_norm(pr, E, lane);
      float d = 0.f;
      for (int e = lane; e < E; e += 64) d = fmaf(hr[e] * inv, pr[e] * pinv, d);
      s = gl_wave_sum(d);
    }
    if (lane == 0) {
      qinv[slot] = inv;
      qsim[slot] = s;
    }
  }
  __syncthreads();
  const int q = i0 + wave * 32 + j;
  const int yq = q < N ? cl_label(labels[q], K) : -1;
  const float sq = qsim[wave * 32 + j];
  const float u = MODE == CL_2C ? sq * inv_tau : fminf(sq - mp, 0.f) * inv_tau;
  float mD = u, sD = 1.f, mM = u, sM = 1.f;
  for (int k0 = 0; k0 < N; k0 += CL_TILE) {
    __syncthreads();                                   // the last tile's readers of kinv / klab / ks are done
    for (int rr = 0; rr < 32; ++rr) {
      const int slot = wave * 32 + rr, row = k0 + slot;
      const float inv = row < N ? cl_inv_norm(hmat + (long long)row * E, E, lane) : 0.f;
      if (lane == 0) {
        kinv[slot] = inv;
        klab[slot] = row < N ? cl_label(labels[row], K) : -2;
      }
    }
    f32x16 acc[2] = {cl_zero(), cl_zero()};
    for (int e0 = 0; e0 < E; e0 += 32) {
      __syncthreads();
      cl_stage(qs, hmat, qinv, i0, N, E, e0);
      cl_stage(ks, hmat, kinv, k0, N, E, e0);
      __syncthreads();
      cl_tile_dot(acc, qs, ks, wave, j, h);
    }
    // A (or -inf where the pair does not count) in place; the tile's maxima
    float tD = -INFINITY, tM = -INFINITY;
    bool same[2][16];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = kh * 32 + cl_row(r, h), key = k0 + kk;
        const int ky = klab[kk];
        float a = -INFINITY;
        same[kh][r] = false;
        if (MODE == CL_2C) {
          if (key < N && key != q) {
            a = acc[kh][r] * inv_tau;
            same[kh][r] = ky == yq;
            if (same[kh][r]) tM = fmaxf(tM, a);
          }
        } else {
          if (key < N && ky != yq) a = fmaxf(acc[kh][r] - mn, 0.f) * inv_tau;
        }
        acc[kh][r] = a;
        tD = fmaxf(tD, a);
      }
    tD = fmaxf(tD, __shfl_xor(tD, 32, 64));
    const float nD = fmaxf(mD, tD);                      // finite: mD starts at u
    float rD = 0.f;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int r = 0; r < 16; ++r) rD += acc[kh][r] == -INFINITY ? 0.f : expf(acc[kh][r] - nD);
    rD += __shfl_xor(rD, 32, 64);
    sD = sD * expf(mD - nD) + rD;
    mD = nD;
    if (MODE == CL_2C) {
      tM = fmaxf(tM, __shfl_xor(tM, 32, 64));
      const float nM = fmaxf(mM, tM);
      float rM = 0.f;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int r = 0; r < 16; ++r) rM += same[kh][r] ? expf(acc[kh][r] - nM) : 0.f;
      rM += __shfl_xor(rM, 32, 64);
      sM = sM * expf(mM - nM) + rM;
      mM = nM;
    }
  }
  if (h == 0 && q < N) {
    const float D = mD + logf(sD), M = MODE == CL_2C ? mM + logf(sM) : u;
    rows[q] = D - M;
    rows[(long long)N + q] = D;
    rows[2LL * N + q] = M;
    rows[3LL * N + q] = sq;
  }
}

__global__ __launch_bounds__(256) void cl_mean_kernel(const float* __restrict__ v, float* __restrict__ out, int N) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) acc += (double)v[i];
  acc = gl_block_sum_256d(acc, red);
  if (threadIdx.x == 0) out[0] = (float)(acc / (double)N);
}

// ---- contrastive backward ------------------------------------------------------------------------------------------------------
// one wave per row of [h; proxy]: hh and 1/|h_i| for the N rows of h, 1/|p_k| for the K proxies
__global__ __launch_bounds__(256) void cl_norm_kernel(const float* __restrict__ hmat, const float* __restrict__ proxy,
                                                      float* __restrict__ hhat, float* __restrict__ hinv,
                                                      float* __restrict__ pinv, int N, int E, int K) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (long long)N + K) return;
  if (row < N) {
    const float* hr = hmat + row * E;
    const float inv = cl_inv_norm(hr, E, lane);
    for (int e = lane; e < E; e += 64) hhat[row * E + e] = hr[e] * inv;
    if (lane == 0) hinv[row] = inv;
  } else {
    const float inv = cl_inv_norm(proxy + (row - N) * E, E, lane);
    if (lane == 0) pinv[row - N] = inv;
  }
}

template <int MODE>
__global__ __launch_bounds__(128) void cl_bwd_kernel(const float* __restrict__ hhat, const float* __restrict__ hinv,
                                                     const float* __restrict__ proxy, const float* __restrict__ pinv,
                                                     const int* __restrict__ labels, const float* __restrict__ rows,
                                                     const float* __restrict__ gout, float* __restrict__ dh, int N, int E, int K,
                                                     float inv_tau, float mp, float mn) {
  __shared__ float qs[CL_TILE * CL_LD];
  __shared__ float ks[CL_TILE * CL_LD];
  __shared__ float kD[CL_TILE], kM[CL_TILE];
  __shared__ int klab[CL_TILE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int i0 = blockIdx.x * CL_TILE;
  const float* Dst = rows + N;
  const float* Mst = rows + 2LL * N;
  const float* sst = rows + 3LL * N;
  const int q = i0 + wave * 32 + j;
  const int yq = q < N ? cl_label(labels[q], K) : -1;
  const float Dq = q < N ? Dst[q] : INFINITY, Mq = q < N ? Mst[q] : INFINITY;      // exp(A - inf) = 0
  for (int eb0 = 0; eb0 < E; eb0 += CL_EBLOCK) {
    f32x16 dacc[4] = {cl_zero(), cl_zero(), cl_zero(), cl_zero()};
    for (int k0 = 0; k0 < N; k0 += CL_TILE) {
      __syncthreads();                                 // the last tile's readers of kD / kM / klab / ks are done
      if (threadIdx.x < CL_TILE) {
        const int key = k0 + threadIdx.x;
        kD[threadIdx.x] = key < N ? Dst[key] : INFINITY;
        kM[threadIdx.x] = key < N ? Mst[key] : INFINITY;
        klab[threadIdx.x] = key < N ? cl_label(labels[key], K) : -2;
      }
      f32x16 acc[2] = {cl_zero(), cl_zero()};
      for (int e0 = 0; e0 < E; e0 += 32) {
        __syncthreads();
        cl_stage(qs, hhat, nullptr, i0, N, E, e0);
        cl_stage(ks, hhat, nullptr, k0, N, E, e0);
        __syncthreads();
        cl_tile_dot(acc, qs, ks, wave, j, h);
      }
      // c[key][query] = a_ij + a_ji in place
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kk = kh * 32 + cl_row(r, h), key = k0 + kk;
          const int ky = klab[kk];
          const float S = acc[kh][r];
          float c = 0.f;
          if (MODE == CL_2C) {
            if (key < N && q < N && key != q) {
              const float a = S * inv_tau;
              c = expf(a - Dq) + expf(a - kD[kk]);
              if (ky == yq) c -= expf(a - Mq) + expf(a - kM[kk]);
              c *= inv_tau;
            }
          } else {
            if (key < N && q < N && ky != yq && S > mn) {
              const float a = (S - mn) * inv_tau;
              c = (expf(a - Dq) + expf(a - kD[kk])) * inv_tau;
            }
          }
          acc[kh][r] = c;
        }
      // dhh^T[e][query] += sum_key hh[key][e] c[key][query]
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (eb0 + t * 32 < E) {                          // workgroup-uniform
          __syncthreads();
          cl_stage(ks, hhat, nullptr, k0, N, E, eb0 + t * 32);
          __syncthreads();
#pragma unroll
          for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              dacc[t] = cl_mfma(ks[(kh * 32 + cl_row(r, h)) * CL_LD + j], acc[kh][r], dacc[t]);
        }
      }
    }
    if (q < N) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int e = eb0 + t * 32 + cl_row(r, h);
          if (e < E) dh[(long long)q * E + e] = dacc[t][r];
        }
    }
  }
  __syncthreads();                                     // the parked rows of dhh are visible to the workgroup
  const float gN = gout[0] / (float)N;
  for (int rr = 0; rr < 32; ++rr) {
    const int row = i0 + wave * 32 + rr;
    if (row >= N) break;                               // wave-uniform; no barrier follows
    const int y = cl_label(labels[row], K);
    const float b = cl_b<MODE>(sst[row], Dst[row], Mst[row], inv_tau, mp);
    const float pin = pinv[y];
    const float* hr = hhat + (long long)row * E;
    const float* pr = proxy + (long long)y * E;
    float* dr = dh + (long long)row * E;
    float d = 0.f;
    for (int e = lane; e < E; e += 64) d = fmaf(hr[e], dr[e] + b * (pr[e] * pin), d);
    d = gl_wave_sum(d);
    const float sc = hinv[row] * gN;
    for (int e = lane; e < E; e += 64) dr[e] = ((dr[e] + b * (pr[e] * pin)) - hr[e] * d) * sc;
  }
}

// one workgroup per class; thread t owns columns t, t + 256, ...
template <int MODE>
__global__ __launch_bounds__(256) void cl_dproxy_kernel(const float* __restrict__ hhat, const float* __restrict__ proxy,
                                                        const float* __restrict__ pinv, const int* __restrict__ labels,
                                                        const float* __restrict__ rows, const float* __restrict__ gout,
                                                        float* __restrict__ dproxy, int N, int E, int K, float inv_tau, float mp) {
  __shared__ float red[4];
  const int k = blockIdx.x;
  const float* Dst = rows + N;
  const float* Mst = rows + 2LL * N;
  const float* sst = rows + 3LL * N;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < N; ++i) {
    if (cl_label(labels[i], K) != k) continue;         // workgroup-uniform
    const float b = cl_b<MODE>(sst[i], Dst[i], Mst[i], inv_tau, mp);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int e = threadIdx.x + c * 256;
      if (e < E) acc[c] = fmaf(b, hhat[(long long)i * E + e], acc[c]);
    }
  }
  const float pin = pinv[k];
  const float* pr = proxy + (long long)k * E;
  float d = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int e = threadIdx.x + c * 256;
    if (e < E) d = fmaf(pr[e] * pin, acc[c], d);
  }
  d = gl_block_sum_256(d, red);
  const float sc = pin * (gout[0] / (float)N);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int e = threadIdx.x + c * 256;
    if (e < E) dproxy[(long long)k * E + e] = (acc[c] - (pr[e] * pin) * d) * sc;
  }
}

bool cl_supported(int N, int E, int K) { return N >= 1 && N <= 8192 && E >= 1 && E <= 1024 && K >= 2 && K <= 65536; }
bool cl_params_ok(int mode, float tau, float mp, float mn) {
  return (mode == CL_2C || mode == CL_D2D) && tau > 0.f && isfinite(tau) && isfinite(mp) && isfinite(mn);
}

}  // namespace

#define ST gl_stream(stream)

extern "C" {

int ganlab_class_ce_fwd_f32(const float* z, const int* labels, float* loss, float* lse, int N, int K, void* stream) {
  if (!z || !labels || !loss || !lse) return GANLAB_EINVAL;
  if (N < 1 || N > 8192 || K < 2 || K > 65536) return GANLAB_EUNSUPPORTED;
  GL_LAUNCH(ce_fwd_kernel, dim3(1), dim3(1024), 0, ST, z, labels, loss, lse, N, K);
  return GL_CHECK_LAUNCH();
}

int ganlab_class_ce_bwd_f32(const float* z, const int* labels, const float* lse, const float* gout, float* dz, int N, int K,
                            void* stream) {
  if (!z || !labels || !lse || !gout || !dz) return GANLAB_EINVAL;
  if (N < 1 || N > 8192 || K < 2 || K > 65536) return GANLAB_EUNSUPPORTED;
  GL_LAUNCH(ce_bwd_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ST, z, labels, lse, gout, dz, N, K);
  return GL_CHECK_LAUNCH();
}

int ganlab_cl_supported(int N, int E, int K) { return cl_supported(N, E, K) ? 1 : 0; }

int ganlab_cl_fwd_f32(const float* h, const float* proxy, const int* labels, float* loss, float* rows, int N, int E, int K,
                      int mode, float temperature, float margin_pos, float margin_neg, void* stream) {
  if (!h || !proxy || !labels || !loss || !rows || !cl_params_ok(mode, temperature, margin_pos, margin_neg)) return GANLAB_EINVAL;
  if (!cl_supported(N, E, K)) return GANLAB_EUNSUPPORTED;
  const unsigned grid = (unsigned)((N + CL_TILE - 1) / CL_TILE);
  const float inv_tau = 1.0f / temperature;
  if (mode == CL_2C)
    GL_LAUNCH(cl_fwd_kernel<CL_2C>, dim3(grid), dim3(128), 0, ST, h, proxy, labels, rows, N, E, K, inv_tau, margin_pos,
              margin_neg);
  else
    GL_LAUNCH(cl_fwd_kernel<CL_D2D>, dim3(grid), dim3(128), 0, ST, h, proxy, labels, rows, N, E, K, inv_tau, margin_pos,
              margin_neg);
  GL_LAUNCH(cl_mean_kernel, dim3(1), dim3(256), 0, ST, (const float*)rows, loss, N);
  return GL_CHECK_LAUNCH();
}

size_t ganlab_cl_bwd_workspace(int N, int E, int K) {
  if (!cl_supported(N, E, K)) return 0;
  return ((size_t)N * E + (size_t)N + (size_t)K) * sizeof(float);
}

int ganlab_cl_bwd_f32(const float* h, const float* proxy, const int* labels, const float* rows, const float* gout, float* dh,
                      float* dproxy, int N, int E, int K, int mode, float temperature, float margin_pos, float margin_neg,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !proxy || !labels || !rows || !gout || !dh || !dproxy ||
      !cl_params_ok(mode, temperature, margin_pos, margin_neg))
    return GANLAB_EINVAL;
  if (!cl_supported(N, E, K)) return GANLAB_EUNSUPPORTED;
  if (!workspace || workspace_bytes < ganlab_cl_bwd_workspace(N, E, K)) return GANLAB_EWORKSPACE;
  float* hhat = reinterpret_cast<float*>(workspace);
  float* hinv = hhat + (size_t)N * E;
  float* pinv = hinv + N;
  const float inv_tau = 1.0f / temperature;
  const unsigned grid = (unsigned)((N + CL_TILE - 1) / CL_TILE);
  GL_LAUNCH(cl_norm_kernel, dim3((unsigned)(((long long)N + K + 3) / 4)), dim3(256), 0, ST, h, proxy, hhat, hinv, pinv, N, E, K);
  if (mode == CL_2C) {
    GL_LAUNCH(cl_bwd_kernel<CL_2C>, dim3(grid), dim3(128), 0, ST, (const float*)hhat, (const float*)hinv, proxy,
              (const float*)pinv, labels, rows, gout, dh, N, E, K, inv_tau, margin_pos, margin_neg);
    GL_LAUNCH(cl_dproxy_kernel<CL_2C>, dim3((unsigned)K), dim3(256), 0, ST, (const float*)hhat, proxy, (const float*)pinv,
              labels, rows, gout, dproxy, N, E, K, inv_tau, margin_pos);
  } else {
    GL_LAUNCH(cl_bwd_kernel<CL_D2D>, dim3(grid), dim3(128), 0, ST, (const float*)hhat, (const float*)hinv, proxy,
              (const float*)pinv, labels, rows, gout, dh, N, E, K, inv_tau, margin_pos, margin_neg);
    GL_LAUNCH(cl_dproxy_kernel<CL_D2D>, dim3((unsigned)K), dim3(256), 0, ST, (const float*)hhat, proxy, (const float*)pinv,
              labels, rows, gout, dproxy, N, E, K, inv_tau, margin_pos);
  }
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
