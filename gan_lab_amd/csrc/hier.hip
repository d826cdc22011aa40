// BigGAN's generator conditioning for the ResNet GAN (config.hier_latent / config.shared_embed): hierarchical
// latents ("skip-z") and a shared class embedding (Brock et al. 2019, section 3 and appendix B); without labels the same
// mechanism is self-modulation (Chen et al. 2019).  Two kernel families, no atomics anywhere: two runs are bitwise equal.
//
// Modulation, batched over every linear of every norm.  z (N, Lz), shared (K, E) (E = 0: none), labels int32 (N,) clamped into
// [0, K) as in cond.hip.  Job j is one bias-free linear W_j (C_j, D_j) of a norm, D_j = z_len_j + E, reading
//   cond_j[n,:] = [ z[n, z_off_j : z_off_j + z_len_j], shared[l_n, :] ]                          never materialised
//   fwd      out[n, col_j + c] = one_j + s_j <W_j[c,:], cond_j[n,:]>          one launch; out (N, T), one_j = 1 (gain) or 0 (shift)
//   dweight  dW_j[c,d] = s_j sum_n g[n, col_j + c] cond_j[n,d]                 n ascending, WRITTEN to the job's gradient slot
//   dcond    dz[n,i] = sum_{j: i in chunk j} s_j sum_c g[n, col_j + c] W_j[c, i - z_off_j]       0 where no job reads z[:, i]
//            de[n,e] = sum_j s_j sum_c g[n, col_j + c] W_j[c, z_len_j + e]      one wave per output, fixed-order reduction
//   dshared  dshared[k,e] = sum_{n: l_n = k} de[n,e]                            n ascending, every row written
// The backward is these three launches (two without an embedding, dcond left out when neither dz nor dshared is wanted) whatever
// the number of jobs.  Sums run in fp64 from the lane accumulator on.
//
// Modulated BatchNorm: gain / shift are (N, C) with a row stride (views into the (N, T) buffer above), the statistics are
// norm.hip's (ganlab_bn_stats_f32 / ganlab_bn_finalize_f32 with weight = NULL) as for cond.hip's conditional norm:
//   apply      y[n,c,:] = act((x - mean[c]) * (rstd[c] * gain[n,c]) + shift[n,c])     cbn_apply_kernel's arithmetic: equal rows
//              reproduce the unconditional kernel bit for bit
//   backward   (first order; gz = gy * act'(y), ghat = gz * gain[n,c], L = N*HW)
//     planes   p0[n,c] = sum_hw gz, p1[n,c] = sum_hw gz * xhat                         bn_planes.h, shared with cond.hip
//     finish   dshift[n,c] = p0[n,c], dgain[n,c] = p1[n,c] written with the destination's own row stride (straight into the
//              (N, T) gradient buffer);  s0[c] = sum_n gain[n,c] p0[n,c], s1[c] likewise from p1
//     apply    gx = rstd[c] * (ghat - s0[c]/L - xhat * s1[c]/L);  without batch statistics (eval mode) gx = rstd[c] * ghat
#include "common.h"
#include "bn_planes.h"      // cbn_bwd_planes_kernel

namespace {

constexpr int EW_MAX_BLOCKS = 256 * 8;
inline unsigned ew_blocks(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > EW_MAX_BLOCKS ? EW_MAX_BLOCKS : b));
}

__device__ __forceinline__ int clamp_label(int l, int K) { return l < 0 ? 0 : (l >= K ? K - 1 : l); }

// ---- modulation ----------------------------------------------------------------------------------------------------------------
// the job that owns block b of a pass: jobs are sorted by their first block, the last one that starts at or before b
template <bool WPASS>
__device__ __forceinline__ int job_of_block(const ganlab_hier_job* __restrict__ jobs, int J, long long b) {
  int j = 0;
  for (int i = 1; i < J; ++i)
    if ((WPASS ? jobs[i].blk_w0 : jobs[i].blk_f0) <= b) j = i;
  return j;
}

// block (x: job and 64-channel tile, y: four samples): lane = channel, wave = sample
__global__ __launch_bounds__(256) void hier_fwd_kernel(const ganlab_hier_job* __restrict__ jobs, int J,
                                                       const float* __restrict__ z, const float* __restrict__ shared,
                                                       const int* __restrict__ labels, float* __restrict__ out, int N,
                                                       long long T, int Lz, int E, int K) {
  const int j = job_of_block<false>(jobs, J, blockIdx.x);
  const ganlab_hier_job job = jobs[j];
  const int c = (int)(blockIdx.x - job.blk_f0) * 64 + (threadIdx.x & 63);
  const int n = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (c >= job.C || n >= N) return;
  const int D = job.z_len + E;
  const float* wr = job.w + (long long)c * D;
  const float* zr = z != nullptr ? z + (long long)n * Lz + job.z_off : nullptr;
  double acc = 0.0;
  for (int d = 0; d < job.z_len; ++d) acc += (double)wr[d] * (double)zr[d];
  if (E > 0) {
    const float* er = shared + (long long)clamp_label(labels[n], K) * E;
    for (int e = 0; e < E; ++e) acc += (double)wr[job.z_len + e] * (double)er[e];
  }
  out[(long long)n * T + job.col + c] = job.one + job.scale * (float)acc;
}

// thread = one element (c, d) of one job's weight gradient
__global__ __launch_bounds__(256) void hier_dweight_kernel(const ganlab_hier_job* __restrict__ jobs, int J,
                                                           const float* __restrict__ g, const float* __restrict__ z,
                                                           const float* __restrict__ shared, const int* __restrict__ labels,
                                                           int N, long long T, int Lz, int E, int K, int which) {
  const int j = job_of_block<true>(jobs, J, blockIdx.x);
  const ganlab_hier_job job = jobs[j];
  const int D = job.z_len + E;
  const long long e = (long long)(blockIdx.x - job.blk_w0) * 256 + threadIdx.x;
  if (e >= (long long)job.C * D) return;
  const int c = (int)(e / D), d = (int)(e - (long long)c * D);
  const float* gc = g + job.col + c;
  double acc = 0.0;
  if (d < job.z_len) {
    const float* zc = z + job.z_off + d;
    for (int n = 0; n < N; ++n) acc += (double)gc[(long long)n * T] * (double)zc[(long long)n * Lz];
  } else {
    const float* sc = shared + (d - job.z_len);
    for (int n = 0; n < N; ++n)
      acc += (double)gc[(long long)n * T] * (double)sc[(long long)clamp_label(labels[n], K) * E];
  }
  float* gw = which ? job.gw_own : job.gw;
  gw[e] = job.scale * (float)acc;
}

// one wave per output (n, i), i in [i0, i1): i < Lz an entry of dz, else entry i - Lz of de
__global__ __launch_bounds__(256) void hier_dcond_kernel(const ganlab_hier_job* __restrict__ jobs, int J,
                                                         const float* __restrict__ g, float* __restrict__ dz,
                                                         float* __restrict__ de, int N, long long T, int Lz, int E, int i0,
                                                         int i1) {
  const int per = i1 - i0;
  const long long o = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (o >= (long long)N * per) return;
  const int lane = threadIdx.x & 63;
  const int n = (int)(o / per), i = i0 + (int)(o - (long long)n * per);
  const float* gr = g + (long long)n * T;
  double acc = 0.0;
  for (int j = 0; j < J; ++j) {
    const int C = jobs[j].C, z_off = jobs[j].z_off, z_len = jobs[j].z_len;
    int d;
    if (i < Lz) {
      if (i < z_off || i >= z_off + z_len) continue;
      d = i - z_off;
    } else {
      d = z_len + (i - Lz);
    }
    const int D = z_len + E;
    const float* w = jobs[j].w + d;
    const float* gj = gr + jobs[j].col;
    double a = 0.0;
    for (int c = lane; c < C; c += 64) a += (double)gj[c] * (double)w[(long long)c * D];
    acc += (double)jobs[j].scale * a;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  if (lane == 0) {
    if (i < Lz)
      dz[(long long)n * Lz + i] = (float)acc;
    else
      de[(long long)n * E + (i - Lz)] = (float)acc;
  }
}

__global__ void hier_dshared_kernel(const float* __restrict__ de, const int* __restrict__ labels, float* __restrict__ out,
                                    int N, int E, int K) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)K * E) return;
  const int k = (int)(t / E), e = (int)(t - (long long)k * E);
  double s = 0.0;
  for (int n = 0; n < N; ++n)
    if (clamp_label(labels[n], K) == k) s += (double)de[(long long)n * E + e];
  out[t] = (float)s;
}

// ---- modulated BatchNorm -------------------------------------------------------------------------------------------------------
__global__ void mbn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                 const float* __restrict__ gain, const float* __restrict__ shift, float* __restrict__ y,
                                 long long total4, int C, long long hw4, long long gstride, long long sstride, int act,
                                 float slope) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    const long long plane = i / hw4;
    const int c = (int)(plane % C);
    const long long n = plane / C;
    const float mu = mean[c], sc = rstd[c] * gain[n * gstride + c], sh = shift[n * sstride + c];
    float4 v = reinterpret_cast<const float4*>(x)[i];
    v.x = (v.x - mu) * sc + sh;
    v.y = (v.y - mu) * sc + sh;
    v.z = (v.z - mu) * sc + sh;
    v.w = (v.w - mu) * sc + sh;
    if (act == GANLAB_ACT_LRELU) {
      v.x = gl_lrelu(v.x, slope); v.y = gl_lrelu(v.y, slope);
      v.z = gl_lrelu(v.z, slope); v.w = gl_lrelu(v.w, slope);
    }
    reinterpret_cast<float4*>(y)[i] = v;
  }
}
__global__ void mbn_apply1_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                  const float* __restrict__ gain, const float* __restrict__ shift, float* __restrict__ y,
                                  long long total, int C, long long HW, long long gstride, long long sstride, int act,
                                  float slope) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long plane = i / HW;
    const int c = (int)(plane % C);
    const long long n = plane / C;
    const float sc = rstd[c] * gain[n * gstride + c];
    const float v = (x[i] - mean[c]) * sc + shift[n * sstride + c];
    y[i] = act == GANLAB_ACT_LRELU ? gl_lrelu(v, slope) : v;
  }
}

// thread t = n * C + c: n < N the two per-sample gradients of (n, c), n == N the two weighted channel sums of channel c
__global__ void mbn_bwd_finish_kernel(const double* __restrict__ part, const float* __restrict__ gain, long long gstride,
                                      float* __restrict__ sums, float* __restrict__ dgain, float* __restrict__ dshift,
                                      long long dstride, int N, int C) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)(N + 1) * C) return;
  const int n = (int)(t / C), c = (int)(t - (long long)n * C);
  if (n == N) {
    double a0 = 0.0, a1 = 0.0;
    for (int m = 0; m < N; ++m) {
      const double w = (double)gain[(long long)m * gstride + c];
      a0 += w * part[((long long)m * C + c) * 2];
      a1 += w * part[((long long)m * C + c) * 2 + 1];
    }
    sums[c * 2] = (float)a0;
    sums[c * 2 + 1] = (float)a1;
  } else if (dgain != nullptr) {
    dshift[(long long)n * dstride + c] = (float)part[t * 2];
    dgain[(long long)n * dstride + c] = (float)part[t * 2 + 1];
  }
}

// sums == NULL: no batch statistics behind mean / rstd (eval mode), gx = rstd * ghat
__global__ void mbn_bwd_apply_kernel(const float* __restrict__ gz, const float* __restrict__ x, const float* __restrict__ mean,
                                     const float* __restrict__ rstd, const float* __restrict__ gain, long long gstride,
                                     const float* __restrict__ sums, float* __restrict__ gx, long long total4, int C,
                                     long long hw4, float inv_len) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    const long long plane = i / hw4;
    const int c = (int)(plane % C);
    const float mu = mean[c], rs = rstd[c], w = gain[(plane / C) * gstride + c];
    const float a = sums != nullptr ? sums[c * 2] * inv_len : 0.f, b = sums != nullptr ? sums[c * 2 + 1] * inv_len : 0.f;
    const float4 g = reinterpret_cast<const float4*>(gz)[i], xv = reinterpret_cast<const float4*>(x)[i];
    float4 o;
    o.x = rs * (g.x * w - a - (xv.x - mu) * rs * b);
    o.y = rs * (g.y * w - a - (xv.y - mu) * rs * b);
    o.z = rs * (g.z * w - a - (xv.z - mu) * rs * b);
    o.w = rs * (g.w * w - a - (xv.w - mu) * rs * b);
    reinterpret_cast<float4*>(gx)[i] = o;
  }
}
__global__ void mbn_bwd_apply1_kernel(const float* __restrict__ gz, const float* __restrict__ x, const float* __restrict__ mean,
                                      const float* __restrict__ rstd, const float* __restrict__ gain, long long gstride,
                                      const float* __restrict__ sums, float* __restrict__ gx, long long total, int C,
                                      long long HW, float inv_len) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long plane = i / HW;
    const int c = (int)(plane % C);
    const float mu = mean[c], rs = rstd[c], w = gain[(plane / C) * gstride + c];
    const float a = sums != nullptr ? sums[c * 2] * inv_len : 0.f, b = sums != nullptr ? sums[c * 2 + 1] * inv_len : 0.f;
    gx[i] = rs * (gz[i] * w - a - (x[i] - mu) * rs * b);
  }
}

inline bool aligned16(const void* a, const void* b, const void* c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

inline bool hier_args_ok(const ganlab_hier_job* jobs, int J, long long blocks, int N, long long T, int Lz, int E, int K,
                         const float* z, const float* shared, const int* labels) {
  return jobs && J > 0 && blocks > 0 && blocks <= 0x7fffffffLL && N > 0 && N <= 4 * 65535 && T > 0 && Lz >= 0 && E >= 0 && (Lz > 0 || E > 0) &&
         (Lz == 0 || z) && (E == 0 || (shared && labels && K > 0));
}

}  // namespace

#define ST gl_stream(stream)

extern "C" {

int ganlab_hier_job_size(void) { return (int)sizeof(ganlab_hier_job); }

int ganlab_hier_fwd_f32(const ganlab_hier_job* jobs_device, int n_jobs, long long blocks_fwd, const float* z,
                        const float* shared, const int* labels, float* out, int N, long long T, int Lz, int E, int K,
                        void* stream) {
  if (!hier_args_ok(jobs_device, n_jobs, blocks_fwd, N, T, Lz, E, K, z, shared, labels) || !out) return GANLAB_EINVAL;
  GL_LAUNCH(hier_fwd_kernel, dim3((unsigned)blocks_fwd, (unsigned)((N + 3) / 4)), dim3(256), 0, ST, jobs_device, n_jobs, z,
            shared, labels, out, N, T, Lz, E, K);
  return GL_CHECK_LAUNCH();
}

int ganlab_hier_bwd_f32(const ganlab_hier_job* jobs_device, int n_jobs, long long blocks_dw, const float* g, const float* z,
                        const float* shared, const int* labels, float* dz, float* de, float* dshared, int N, long long T,
                        int Lz, int E, int K, int own_slots, void* stream) {
  if (!hier_args_ok(jobs_device, n_jobs, blocks_dw, N, T, Lz, E, K, z, shared, labels) || !g || (dshared != nullptr && !de) ||
      (E == 0 && dshared != nullptr))
    return GANLAB_EINVAL;
  GL_LAUNCH(hier_dweight_kernel, dim3((unsigned)blocks_dw), dim3(256), 0, ST, jobs_device, n_jobs, g, z, shared, labels, N, T,
            Lz, E, K, own_slots);
  const int i0 = dz != nullptr ? 0 : Lz, i1 = dshared != nullptr ? Lz + E : Lz;
  if (i1 > i0) {
    const long long waves = (long long)N * (i1 - i0);
    GL_LAUNCH(hier_dcond_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ST, jobs_device, n_jobs, g, dz, de, N, T, Lz,
              E, i0, i1);
  }
  if (dshared != nullptr)
    GL_LAUNCH(hier_dshared_kernel, dim3((unsigned)(((long long)K * E + 255) / 256)), dim3(256), 0, ST, de, labels, dshared, N,
              E, K);
  return GL_CHECK_LAUNCH();
}

int ganlab_mbn_apply_f32(const float* x, const float* mean, const float* rstd, const float* gain, long long gain_stride,
                         const float* shift, long long shift_stride, float* y, int N, int C, long long HW, int act,
                         float slope, void* stream) {
  if (!x || !mean || !rstd || !gain || !shift || !y || N <= 0 || C <= 0 || HW <= 0 || gain_stride < C || shift_stride < C)
    return GANLAB_EINVAL;
  const long long total = (long long)N * C * HW;
  if ((HW & 3) == 0 && aligned16(x, y))
    GL_LAUNCH(mbn_apply_kernel, dim3(ew_blocks(total / 4)), dim3(256), 0, ST, x, mean, rstd, gain, shift, y, total / 4, C,
              HW / 4, gain_stride, shift_stride, act, slope);
  else
    GL_LAUNCH(mbn_apply1_kernel, dim3(ew_blocks(total)), dim3(256), 0, ST, x, mean, rstd, gain, shift, y, total, C, HW,
              gain_stride, shift_stride, act, slope);
  return GL_CHECK_LAUNCH();
}

size_t ganlab_mbn_bwd_workspace(int N, int C) {
  if (N <= 0 || C <= 0) return 0;
  return (size_t)N * C * 2 * sizeof(double);
}

int ganlab_mbn_bwd_f32(const float* gy, const float* x, const float* mean, const float* rstd, const float* gain,
                       long long gain_stride, const float* yact, float* gz, float* gx, float* dgain, float* dshift,
                       long long grad_stride, float* sums, int N, int C, long long HW, int batch_stats, float slope,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (!gy || !x || !mean || !rstd || !gain || !sums || N <= 0 || C <= 0 || HW <= 0 || gain_stride < C ||
      (yact != nullptr) != (gz != nullptr) || (dgain != nullptr) != (dshift != nullptr) || (dgain != nullptr && grad_stride < C))
    return GANLAB_EINVAL;
  if (!workspace || workspace_bytes < ganlab_mbn_bwd_workspace(N, C)) return GANLAB_EWORKSPACE;
  double* part = reinterpret_cast<double*>(workspace);
  const long long planes = (long long)N * C, total = planes * HW;
  const unsigned pgrid = (unsigned)((planes + 3) / 4);
  if ((HW & 3) == 0 && aligned16(gy, x) && aligned16(yact, gz))
    GL_LAUNCH(cbn_bwd_planes_kernel<true>, dim3(pgrid), dim3(256), 0, ST, gy, x, mean, rstd, yact, gz, part, planes, C, HW,
              slope);
  else
    GL_LAUNCH(cbn_bwd_planes_kernel<false>, dim3(pgrid), dim3(256), 0, ST, gy, x, mean, rstd, yact, gz, part, planes, C, HW,
              slope);
  const long long fin = (long long)(N + 1) * C;
  GL_LAUNCH(mbn_bwd_finish_kernel, dim3((unsigned)((fin + 255) / 256)), dim3(256), 0, ST, part, gain, gain_stride, sums, dgain,
            dshift, grad_stride, N, C);
  if (gx != nullptr) {
    const float* g = gz != nullptr ? gz : gy;
    const float* s = batch_stats ? sums : nullptr;
    const float inv_len = 1.0f / (float)((long long)N * HW);
    if ((HW & 3) == 0 && aligned16(g, x, gx))
      GL_LAUNCH(mbn_bwd_apply_kernel, dim3(ew_blocks(total / 4)), dim3(256), 0, ST, g, x, mean, rstd, gain, gain_stride, s, gx,
                total / 4, C, HW / 4, inv_len);
    else
      GL_LAUNCH(mbn_bwd_apply1_kernel, dim3(ew_blocks(total)), dim3(256), 0, ST, g, x, mean, rstd, gain, gain_stride, s, gx,
                total, C, HW, inv_len);
  }
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
