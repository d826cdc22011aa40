// Projection of images into StyleGAN's latent space (gan_lab_amd/project.py): what an iteration needs beyond the
// generator's own forward and backward - a multi-scale reconstruction loss with its gradient, and the update of the latent rows.
// No atomics, every sum in a fixed order: two runs are bitwise equal.  Nothing is read back by the host; the iteration count lives
// on the device.
//
// pyramid_mse   d_0 = x - t, d_{l+1} = the 2x2 mean of d_l; loss[n] = sum_l w_l mean_{c,h,w} d_l[n]^2.  A workgroup owns a 32x32 tile
//               of one (n, c) plane (the whole plane below 32x32): it forms every level of d inside the tile in LDS (fp32 differences
//               and means), squares and sums per level in fp64, writes the gradient tile (summed in fp64, rounded once)
//                   g = 2 / (C R^2) * sum_l w_l up_l(d_l)          (R_l^2 4^l = R^2: every level has the same normaliser)
//               and one fp64 partial per (tile, level).  x and t are read once, g is written once.  A second launch, one workgroup
//               per sample, adds the partials in index order into terms[n, l] = mean d_l[n]^2 and loss[n].
// scale_rows    out[n, :] = g[n, :] * s[n]: the backward of pyramid_mse under a per-sample cotangent.
// w_moments     w_avg = the column means of (M, D) rows, w_std = sqrt(sum (w - w_avg)^2 / M) over ALL entries (the StyleGAN2
//               projector's definition): two passes in fp64, a workgroup owns 64 columns and reads them twice; the partials of the
//               second pass are added in index order by a one-workgroup launch.
// project_step  ONE workgroup: reads the device-resident iteration count k, reduces the per-layer gradients (W space: in layer
//               order), applies Adam's update k + 1 with the learning rate of the schedule at t = k / num_steps, writes k + 1, and
//               writes the next forward's input w_in = w_opt + scale((k + 1) / num_steps) * noise.  The schedule and the bias
//               corrections are computed once, in fp64; every element's update in fp64 from fp32 state, rounded once per stored
//               value.  One workgroup because every thread reads k before one of them replaces it.
#include "common.h"

namespace {

constexpr int PM_TILE = 32;
constexpr int PM_LDS = 1024 + 256 + 64 + 16 + 4 + 1;      // every level of a 32x32 tile

struct PmWeights {
  float w[GANLAB_PYRAMID_MAX_LEVELS];
};

__device__ __forceinline__ double pj_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid: planes * tiles_per_plane workgroups; T = min(R, 32) is the tile edge, a power of two >= 4
__global__ __launch_bounds__(256) void pyramid_mse_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                          float* __restrict__ g, double* __restrict__ part, int R, int T, int Lv,
                                                          PmWeights wt, double gscale) {
  __shared__ __attribute__((aligned(16))) float lv[PM_LDS];
  __shared__ double red[4][GANLAB_PYRAMID_MAX_LEVELS];
  const int tid = threadIdx.x;
  const int tiles_x = R / T, tiles = tiles_x * tiles_x;
  const long long blk = blockIdx.x;
  const long long plane = blk / tiles;
  const int tile = (int)(blk - plane * tiles);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int q = T >> 2;                                     // float4 groups per tile row
  const bool active = tid < T * q;
  const int row = tid / q, c4 = (tid - row * q) * 4;
  const long long at = plane * ((long long)R * R) + (long long)(ty * T + row) * R + tx * T + c4;

  double acc[GANLAB_PYRAMID_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < GANLAB_PYRAMID_MAX_LEVELS; ++l) acc[l] = 0.0;

  if (active) {
    const float4 xv = *reinterpret_cast<const float4*>(x + at), tv = *reinterpret_cast<const float4*>(t + at);
    const float4 d = float4{xv.x - tv.x, xv.y - tv.y, xv.z - tv.z, xv.w - tv.w};
    *reinterpret_cast<float4*>(lv + row * T + c4) = d;
    acc[0] = (double)d.x * (double)d.x;
    acc[0] += (double)d.y * (double)d.y;
    acc[0] += (double)d.z * (double)d.z;
    acc[0] += (double)d.w * (double)d.w;
  }
  __syncthreads();
  int off = 0;
#pragma unroll
  for (int l = 1; l < GANLAB_PYRAMID_MAX_LEVELS; ++l) {
    if (l < Lv) {                                           // Lv is uniform: every thread reaches the barrier
      const int sp = T >> (l - 1), s = T >> l, noff = off + sp * sp;
      if (tid < s * s) {                                    // s * s <= 256
        const int i = tid / s, j = tid - i * s;
        const float* p = lv + off + (2 * i) * sp + 2 * j;
        const float m = ((p[0] + p[1]) + (p[sp] + p[sp + 1])) * 0.25f;
        lv[noff + tid] = m;
        acc[l] = (double)m * (double)m;
      }
      off = noff;
      __syncthreads();
    }
  }

  if (active) {
    double o[4] = {0.0, 0.0, 0.0, 0.0};                     // six terms per output: fp64 costs nothing next to the loads
    int base = 0;
#pragma unroll
    for (int l = 0; l < GANLAB_PYRAMID_MAX_LEVELS; ++l) {
      if (l < Lv) {
        const int s = T >> l;
        const float* p = lv + base + (row >> l) * s;
        const double w = (double)wt.w[l];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fma(w, (double)p[(c4 + k) >> l], o[k]);
        base += s * s;
      }
    }
    *reinterpret_cast<float4*>(g + at) =
        float4{(float)(o[0] * gscale), (float)(o[1] * gscale), (float)(o[2] * gscale), (float)(o[3] * gscale)};
  }

#pragma unroll
  for (int l = 0; l < GANLAB_PYRAMID_MAX_LEVELS; ++l) {
    const double s = pj_wave_sum_d(acc[l]);
    if ((tid & 63) == 0) red[tid >> 6][l] = s;
  }
  __syncthreads();
  if (tid < Lv) part[blk * Lv + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// one workgroup per sample: per_sample = C * tiles partial rows of Lv doubles each
__global__ __launch_bounds__(256) void pyramid_mse_finish_kernel(const double* __restrict__ part, float* __restrict__ loss,
                                                                 float* __restrict__ terms, int per_sample, int Lv, int C, int R,
                                                                 PmWeights wt) {
  __shared__ double red[4];
  __shared__ double total[GANLAB_PYRAMID_MAX_LEVELS];
  const long long n = blockIdx.x;
  const double* rows = part + n * (long long)per_sample * Lv;
  for (int l = 0; l < Lv; ++l) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < per_sample; i += 256) acc += rows[(long long)i * Lv + l];
    acc = gl_block_sum_256d(acc, red);
    if (threadIdx.x == 0) total[l] = acc;
  }
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int l = 0; l < Lv; ++l) {
      const double rl = (double)(R >> l);
      const double term = total[l] / ((double)C * rl * rl);
      terms[n * Lv + l] = (float)term;
      sum += (double)wt.w[l] * term;
    }
    loss[n] = (float)sum;
  }
}

__global__ __launch_bounds__(256) void scale_rows_kernel(const float* __restrict__ g, const float* __restrict__ s,
                                                         float* __restrict__ out, long long per4, long long total4) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    const float k = s[i / per4];
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    reinterpret_cast<float4*>(out)[i] = float4{v.x * k, v.y * k, v.z * k, v.w * k};
  }
}

// workgroup b owns columns [64 b, 64 b + 64): thread (r = tid / 64, c = tid % 64) walks rows r, r + 4, ...
__global__ __launch_bounds__(256) void w_moments_kernel(const float* __restrict__ ws, float* __restrict__ w_avg,
                                                        double* __restrict__ part, long long M, int D) {
  __shared__ double red[4][64];
  const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + c;
  const bool active = col < D;
  double acc = 0.0;
  if (active)
    for (long long i = r; i < M; i += 4) acc += (double)ws[i * D + col];
  red[r][c] = acc;
  __syncthreads();
  const double mean = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) / (double)M;
  __syncthreads();
  if (active && r == 0) w_avg[col] = (float)mean;
  acc = 0.0;
  if (active)
    for (long long i = r; i < M; i += 4) {
      const double d = (double)ws[i * D + col] - mean;
      acc += d * d;
    }
  red[r][c] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int k = 0; k < 64; ++k) sum += (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    part[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(64) void w_moments_finish_kernel(const double* __restrict__ part, float* __restrict__ w_std, int blocks,
                                                              long long M) {
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int i = 0; i < blocks; ++i) sum += part[i];
    w_std[0] = (float)sqrt(sum / (double)M);
  }
}

struct PjHyper {
  double lr0, noise_factor, rampdown, rampup, noise_ramp, num_steps;
};

__device__ __forceinline__ double pj_noise_scale(const PjHyper& h, double t, double w_std) {
  const double a = fmax(0.0, 1.0 - t / h.noise_ramp);
  return w_std * h.noise_factor * a * a;
}

__device__ __forceinline__ double pj_lr(const PjHyper& h, double t) {
  const double r = fmin(1.0, (1.0 - t) / h.rampdown);
  return h.lr0 * (0.5 - 0.5 * cos(3.14159265358979323846 * r)) * fmin(1.0, t / h.rampup);
}

// Lw = 1: W space (w_opt, m, v, noise are (N, D), the gradient is summed over the L layers and w_in broadcast over them);
// Lw = L: W+ space.  grad == nullptr: no update - only w_in at the current iteration count (the first forward's input).
__global__ __launch_bounds__(1024) void project_step_kernel(float* __restrict__ w_opt, const float* __restrict__ grad,
                                                            float* __restrict__ m, float* __restrict__ v, int* __restrict__ step,
                                                            const float* __restrict__ noise, const float* __restrict__ w_std,
                                                            float* __restrict__ w_in, int N, int L, int Lw, int D, PjHyper h) {
  __shared__ double sc[5];
  const int k = step[0];
  __syncthreads();                                          // every thread holds k before thread 0 replaces it
  if (threadIdx.x == 0) {
    const int k1 = grad != nullptr ? k + 1 : k;
    const double t = (double)k / h.num_steps;
    sc[0] = pj_lr(h, t);
    sc[1] = 1.0 - pow(0.9, (double)(k + 1));
    sc[2] = sqrt(1.0 - pow(0.999, (double)(k + 1)));
    sc[3] = pj_noise_scale(h, (double)k1 / h.num_steps, (double)w_std[0]);
    if (grad != nullptr) step[0] = k1;
  }
  __syncthreads();
  const double lr = sc[0], bc1 = sc[1], bc2s = sc[2], nscale = sc[3];
  const long long rows = (long long)N * Lw * D;
  for (long long i = threadIdx.x; i < rows; i += blockDim.x) {
    const long long n = i / ((long long)Lw * D);
    const int rem = (int)(i - n * ((long long)Lw * D));     // l * D + d (W+), d (W)
    double w = (double)w_opt[i];
    if (grad != nullptr) {
      double gd;
      if (Lw == 1) {
        const float* gp = grad + n * ((long long)L * D) + rem;
        gd = (double)gp[0];
        for (int l = 1; l < L; ++l) gd += (double)gp[(long long)l * D];
      } else {
        gd = (double)grad[i];
      }
      const float mf = (float)((double)m[i] + (gd - (double)m[i]) * (1.0 - 0.9));
      const float vf = (float)((double)v[i] * 0.999 + (1.0 - 0.999) * gd * gd);
      m[i] = mf;
      v[i] = vf;
      const float wf = (float)(w - (lr / bc1) * (double)mf / (sqrt((double)vf) / bc2s + 1e-8));
      w_opt[i] = wf;
      w = (double)wf;
    }
    const float wi = (float)(w + nscale * (double)noise[i]);
    if (Lw == 1) {
      float* o = w_in + n * ((long long)L * D) + rem;
      for (int l = 0; l < L; ++l) o[(long long)l * D] = wi;
    } else {
      w_in[i] = wi;
    }
  }
}

inline bool pj_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool pj_pow2(int r) { return r > 0 && (r & (r - 1)) == 0; }

// workgroups of pyramid_mse's first launch, or 0 for a geometry outside the kernel's range
inline long long pm_blocks(int N, int C, int R, int Lv) {
  if (N <= 0 || C <= 0 || !pj_pow2(R) || R < 4 || R > 1024 || Lv < 1 || Lv > GANLAB_PYRAMID_MAX_LEVELS) return 0;
  int log2r = 0;
  while ((1 << log2r) < R) ++log2r;
  if (Lv > log2r + 1) return 0;
  const int tx = R < PM_TILE ? 1 : R / PM_TILE;
  const long long b = (long long)N * C * tx * tx;
  return b <= 0x7fffffffLL ? b : 0;
}

}  // namespace

extern "C" {

size_t ganlab_pyramid_mse_workspace(int N, int C, int R, int levels) {
  return (size_t)pm_blocks(N, C, R, levels) * (size_t)levels * sizeof(double);
}

int ganlab_pyramid_mse_f32(const float* x, const float* t, const float* weights, int levels, float* g, float* loss, float* terms,
                           int N, int C, int R, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !t || !weights || !g || !loss || !terms) return GANLAB_EINVAL;
  const long long blocks = pm_blocks(N, C, R, levels);
  if (blocks == 0) return GANLAB_EUNSUPPORTED;
  if (!pj_aligned16(x) || !pj_aligned16(t) || !pj_aligned16(g)) return GANLAB_EINVAL;
  PmWeights wt;
  for (int l = 0; l < GANLAB_PYRAMID_MAX_LEVELS; ++l) {
    wt.w[l] = l < levels ? weights[l] : 0.f;
    if (!(wt.w[l] >= 0.f) || wt.w[l] > 3.0e38f) return GANLAB_EINVAL;
  }
  if (!workspace || workspace_bytes < (size_t)blocks * levels * sizeof(double) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return GANLAB_EWORKSPACE;
  double* part = reinterpret_cast<double*>(workspace);
  const int T = R < PM_TILE ? R : PM_TILE;
  const double gscale = 2.0 / ((double)C * (double)R * (double)R);
  GL_LAUNCH(pyramid_mse_kernel, dim3((unsigned)blocks), dim3(256), 0, gl_stream(stream), x, t, g, part, R, T, levels, wt, gscale);
  GL_LAUNCH(pyramid_mse_finish_kernel, dim3(N), dim3(256), 0, gl_stream(stream), (const double*)part, loss, terms,
            (int)(blocks / N), levels, C, R, wt);
  return GL_CHECK_LAUNCH();
}

int ganlab_scale_rows_f32(const float* g, const float* s, float* out, int N, long long per, void* stream) {
  if (!g || !s || !out || N <= 0 || per <= 0 || (per & 3) || !pj_aligned16(g) || !pj_aligned16(out)) return GANLAB_EINVAL;
  const long long total4 = (long long)N * (per >> 2);
  long long blocks = (total4 + 255) / 256;
  blocks = blocks > 256 * 8 ? 256 * 8 : blocks;
  GL_LAUNCH(scale_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, gl_stream(stream), g, s, out, per >> 2, total4);
  return GL_CHECK_LAUNCH();
}

size_t ganlab_w_moments_workspace(int D) { return D > 0 ? (size_t)((D + 63) / 64) * sizeof(double) : 0; }

int ganlab_w_moments_f32(const float* ws, float* w_avg, float* w_std, long long M, int D, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (!ws || !w_avg || !w_std || M <= 0 || D <= 0 || M > (1LL << 40) / D) return GANLAB_EINVAL;
  const int blocks = (D + 63) / 64;
  if (!workspace || workspace_bytes < (size_t)blocks * sizeof(double) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return GANLAB_EWORKSPACE;
  double* part = reinterpret_cast<double*>(workspace);
  GL_LAUNCH(w_moments_kernel, dim3(blocks), dim3(256), 0, gl_stream(stream), ws, w_avg, part, M, D);
  GL_LAUNCH(w_moments_finish_kernel, dim3(1), dim3(64), 0, gl_stream(stream), (const double*)part, w_std, blocks, M);
  return GL_CHECK_LAUNCH();
}

int ganlab_project_step_f32(float* w_opt, const float* grad_ws, float* m, float* v, int* step, const float* noise,
                            const float* w_std, float* w_in, int N, int L, int w_plus, int D, const double* hyper, void* stream) {
  if (!w_opt || !m || !v || !step || !noise || !w_std || !w_in || !hyper || N <= 0 || L <= 0 || D <= 0) return GANLAB_EINVAL;
  if ((long long)N * L * D > (1LL << 31)) return GANLAB_EINVAL;
  const PjHyper h = {hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5]};
  if (!(h.lr0 >= 0.0) || !(h.noise_factor >= 0.0) || !(h.rampdown > 0.0) || !(h.rampup > 0.0) || !(h.noise_ramp > 0.0) ||
      !(h.num_steps >= 1.0))
    return GANLAB_EINVAL;
  GL_LAUNCH(project_step_kernel, dim3(1), dim3(1024), 0, gl_stream(stream), w_opt, grad_ws, m, v, step, noise, w_std, w_in, N, L,
            w_plus ? L : 1, D, h);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
