// Class conditioning of the ResNet GAN (config.cgan = 'projection'): class-conditional BatchNorm for the
// generator (de Vries et al. 2017; Miyato & Koyama 2018) and the projection term of the critic (Miyato & Koyama 2018).
// labels: int32 (N,), clamped into [0, K) by every kernel that indexes a (K, .) table with one.
//
// Conditional BatchNorm, weight / bias tables (K, C), l_n the label of sample n.  The batch statistics and the running-estimate
// bookkeeping are norm.hip's (ganlab_bn_stats_f32 / ganlab_bn_finalize_f32 with weight = NULL); new here:
//   apply      y[n,c,:] = act((x - mean[c]) * (rstd[c] * weight[l_n,c]) + bias[l_n,c])    the centred form and the product
//              rstd * weight of bn_apply_kernel: a table of equal rows reproduces the unconditional kernel bit for bit
//   backward   (first order; gz = gy * act'(y), ghat = gz * weight[l_n,c], L = N*HW)
//     planes   gz and the plane sums p0[n,c] = sum_hw gz, p1[n,c] = sum_hw gz * xhat      one wave per plane, fp64
//     finish   s0[c] = sum_n weight[l_n,c] p0[n,c], s1[c] likewise from p1;  d bias[k,c] = sum_{n: l_n = k} p0[n,c],
//              d weight[k,c] likewise from p1 - n ascending, every row written (zeros for an absent class)
//     apply    gx = rstd[c] * (ghat - s0[c]/L - xhat * s1[c]/L);  without batch statistics (eval mode) gx = rstd[c] * ghat
// Projection, weight (K, F):
//   P(f, W, l, base)[n] = base[n] + sum_j W[l_n,j] f[n,j]        one workgroup per sample, fixed-order wave / LDS reduction
//   G(g, W, l)[n,j]     = g[n] W[l_n,j]                           = dP/df
//   S(g, f, l)[k,j]     = sum_{n: l_n = k} g[n] f[n,j]            = dP/dW, n ascending, every row written
// Each is bilinear in its float arguments and the derivatives of each are the other two: the family is closed, autograd
// composes any order from it.  No atomics anywhere: two runs are bitwise equal.
#include "common.h"
#include "bn_planes.h"      // cbn_bwd_planes_kernel

namespace {

constexpr int EW_MAX_BLOCKS = 256 * 8;
inline unsigned ew_blocks(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > EW_MAX_BLOCKS ? EW_MAX_BLOCKS : b));
}

__device__ __forceinline__ int clamp_label(int l, int K) { return l < 0 ? 0 : (l >= K ? K - 1 : l); }

// ---- conditional BatchNorm ---------------------------------------------------------------------------------------------------
__global__ void cbn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                 const float* __restrict__ weight, const float* __restrict__ bias,
                                 const int* __restrict__ labels, float* __restrict__ y, long long total4, int C, int K,
                                 long long hw4, int act, float slope) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    const long long plane = i / hw4;
    const int c = (int)(plane % C);
    const long long row = (long long)clamp_label(labels[plane / C], K) * C + c;
    const float mu = mean[c], sc = rstd[c] * weight[row], sh = bias[row];
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
__global__ void cbn_apply1_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                  const float* __restrict__ weight, const float* __restrict__ bias,
                                  const int* __restrict__ labels, float* __restrict__ y, long long total, int C, int K,
                                  long long HW, int act, float slope) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long plane = i / HW;
    const int c = (int)(plane % C);
    const long long row = (long long)clamp_label(labels[plane / C], K) * C + c;
    const float sc = rstd[c] * weight[row];
    const float v = (x[i] - mean[c]) * sc + bias[row];
    y[i] = act == GANLAB_ACT_LRELU ? gl_lrelu(v, slope) : v;
  }
}

// thread t = k * C + c: k < K the table row (k, c) of both gradients, k == K the two weighted channel sums of channel c
__global__ void cbn_bwd_finish_kernel(const double* __restrict__ part, const float* __restrict__ weight,
                                      const int* __restrict__ labels, float* __restrict__ sums, float* __restrict__ gw,
                                      float* __restrict__ gb, int N, int C, int K) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)(K + 1) * C) return;
  const int k = (int)(t / C), c = (int)(t - (long long)k * C);
  double a0 = 0.0, a1 = 0.0;
  if (k == K) {
    for (int n = 0; n < N; ++n) {
      const double w = (double)weight[(long long)clamp_label(labels[n], K) * C + c];
      a0 += w * part[((long long)n * C + c) * 2];
      a1 += w * part[((long long)n * C + c) * 2 + 1];
    }
    sums[c * 2] = (float)a0;
    sums[c * 2 + 1] = (float)a1;
  } else {
    for (int n = 0; n < N; ++n)
      if (clamp_label(labels[n], K) == k) {
        a0 += part[((long long)n * C + c) * 2];
        a1 += part[((long long)n * C + c) * 2 + 1];
      }
    gb[t] = (float)a0;
    gw[t] = (float)a1;
  }
}

// sums == NULL: no batch statistics behind mean / rstd (eval mode), gx = rstd * ghat
__global__ void cbn_bwd_apply_kernel(const float* __restrict__ gz, const float* __restrict__ x, const float* __restrict__ mean,
                                     const float* __restrict__ rstd, const float* __restrict__ weight,
                                     const int* __restrict__ labels, const float* __restrict__ sums, float* __restrict__ gx,
                                     long long total4, int C, int K, long long hw4, float inv_len) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    const long long plane = i / hw4;
    const int c = (int)(plane % C);
    const float mu = mean[c], rs = rstd[c], w = weight[(long long)clamp_label(labels[plane / C], K) * C + c];
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
__global__ void cbn_bwd_apply1_kernel(const float* __restrict__ gz, const float* __restrict__ x, const float* __restrict__ mean,
                                      const float* __restrict__ rstd, const float* __restrict__ weight,
                                      const int* __restrict__ labels, const float* __restrict__ sums, float* __restrict__ gx,
                                      long long total, int C, int K, long long HW, float inv_len) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long plane = i / HW;
    const int c = (int)(plane % C);
    const float mu = mean[c], rs = rstd[c], w = weight[(long long)clamp_label(labels[plane / C], K) * C + c];
    const float a = sums != nullptr ? sums[c * 2] * inv_len : 0.f, b = sums != nullptr ? sums[c * 2 + 1] * inv_len : 0.f;
    gx[i] = rs * (gz[i] * w - a - (x[i] - mu) * rs * b);
  }
}

// ---- projection --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void proj_fwd_kernel(const float* __restrict__ f, const float* __restrict__ weight,
                                                       const int* __restrict__ labels, const float* __restrict__ base,
                                                       float* __restrict__ out, long long F, int K) {
  __shared__ float red[4];
  const int n = blockIdx.x;
  const float* fr = f + (long long)n * F;
  const float* wr = weight + (long long)clamp_label(labels[n], K) * F;
  float s = 0.f;
  for (long long j = threadIdx.x; j < F; j += 256) s += wr[j] * fr[j];
  s = gl_block_sum_256(s, red);
  if (threadIdx.x == 0) out[n] = (base != nullptr ? base[n] : 0.f) + s;
}

__global__ void proj_dfeat_kernel(const float* __restrict__ g, const float* __restrict__ weight,
                                  const int* __restrict__ labels, float* __restrict__ out, long long total, long long F, int K) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / F, j = i - n * F;
    out[i] = g[n] * weight[(long long)clamp_label(labels[n], K) * F + j];
  }
}

__global__ void proj_dweight_kernel(const float* __restrict__ g, const float* __restrict__ f, const int* __restrict__ labels,
                                    float* __restrict__ out, int N, long long F, int K) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)K * F) return;
  const int k = (int)(t / F);
  const long long j = t - (long long)k * F;
  float s = 0.f;
  for (int n = 0; n < N; ++n)
    if (clamp_label(labels[n], K) == k) s += g[n] * f[(long long)n * F + j];
  out[t] = s;
}

// ---- uniform integers from the Philox stream: element e is word e % 4 of counter offset + e / 4, scaled into [0, high) ------
__global__ void randint_kernel(int* __restrict__ out, long long n, int high, uint64_t seed, uint64_t offset) {
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g * 4 >= n) return;
  const uint64_t ctr = offset + (uint64_t)g;
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (g * 4 + k < n) out[g * 4 + k] = (int)(((uint64_t)(c[k] >> 8) * (uint64_t)high) >> 24);
}

inline bool aligned16(const void* a, const void* b, const void* c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

}  // namespace

#define ST gl_stream(stream)

extern "C" {

int ganlab_cbn_apply_f32(const float* x, const float* mean, const float* rstd, const float* weight, const float* bias,
                         const int* labels, float* y, int N, int C, long long HW, int K, int act, float slope, void* stream) {
  if (!x || !mean || !rstd || !weight || !bias || !labels || !y || N <= 0 || C <= 0 || HW <= 0 || K <= 0) return GANLAB_EINVAL;
  const long long total = (long long)N * C * HW;
  if ((HW & 3) == 0 && aligned16(x, y))
    GL_LAUNCH(cbn_apply_kernel, dim3(ew_blocks(total / 4)), dim3(256), 0, ST, x, mean, rstd, weight, bias, labels, y, total / 4,
              C, K, HW / 4, act, slope);
  else
    GL_LAUNCH(cbn_apply1_kernel, dim3(ew_blocks(total)), dim3(256), 0, ST, x, mean, rstd, weight, bias, labels, y, total, C, K,
              HW, act, slope);
  return GL_CHECK_LAUNCH();
}

size_t ganlab_cbn_bwd_workspace(int N, int C) {
  if (N <= 0 || C <= 0) return 0;
  return (size_t)N * C * 2 * sizeof(double);
}

int ganlab_cbn_bwd_f32(const float* gy, const float* x, const float* mean, const float* rstd, const float* weight,
                       const int* labels, const float* yact, float* gz, float* gx, float* gw, float* gb, float* sums, int N,
                       int C, long long HW, int K, int batch_stats, float slope, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (!gy || !x || !mean || !rstd || !weight || !labels || !gw || !gb || !sums || N <= 0 || C <= 0 || HW <= 0 || K <= 0 ||
      (yact != nullptr) != (gz != nullptr))
    return GANLAB_EINVAL;
  if (!workspace || workspace_bytes < ganlab_cbn_bwd_workspace(N, C)) return GANLAB_EWORKSPACE;
  double* part = reinterpret_cast<double*>(workspace);
  const long long planes = (long long)N * C, total = planes * HW;
  const unsigned pgrid = (unsigned)((planes + 3) / 4);
  if ((HW & 3) == 0 && aligned16(gy, x) && aligned16(yact, gz))
    GL_LAUNCH(cbn_bwd_planes_kernel<true>, dim3(pgrid), dim3(256), 0, ST, gy, x, mean, rstd, yact, gz, part, planes, C, HW,
              slope);
  else
    GL_LAUNCH(cbn_bwd_planes_kernel<false>, dim3(pgrid), dim3(256), 0, ST, gy, x, mean, rstd, yact, gz, part, planes, C, HW,
              slope);
  const long long fin = (long long)(K + 1) * C;
  GL_LAUNCH(cbn_bwd_finish_kernel, dim3((unsigned)((fin + 255) / 256)), dim3(256), 0, ST, part, weight, labels, sums, gw, gb, N,
            C, K);
  if (gx != nullptr) {
    const float* g = gz != nullptr ? gz : gy;
    const float* s = batch_stats ? sums : nullptr;
    const float inv_len = 1.0f / (float)((long long)N * HW);
    if ((HW & 3) == 0 && aligned16(g, x, gx))
      GL_LAUNCH(cbn_bwd_apply_kernel, dim3(ew_blocks(total / 4)), dim3(256), 0, ST, g, x, mean, rstd, weight, labels, s, gx,
                total / 4, C, K, HW / 4, inv_len);
    else
      GL_LAUNCH(cbn_bwd_apply1_kernel, dim3(ew_blocks(total)), dim3(256), 0, ST, g, x, mean, rstd, weight, labels, s, gx, total,
                C, K, HW, inv_len);
  }
  return GL_CHECK_LAUNCH();
}

int ganlab_proj_fwd_f32(const float* f, const float* weight, const int* labels, const float* base, float* out, int N,
                        long long F, int K, void* stream) {
  if (!f || !weight || !labels || !out || N <= 0 || F <= 0 || K <= 0) return GANLAB_EINVAL;
  GL_LAUNCH(proj_fwd_kernel, dim3((unsigned)N), dim3(256), 0, ST, f, weight, labels, base, out, F, K);
  return GL_CHECK_LAUNCH();
}

int ganlab_proj_dfeat_f32(const float* g, const float* weight, const int* labels, float* out, int N, long long F, int K,
                          void* stream) {
  if (!g || !weight || !labels || !out || N <= 0 || F <= 0 || K <= 0) return GANLAB_EINVAL;
  GL_LAUNCH(proj_dfeat_kernel, dim3(ew_blocks((long long)N * F)), dim3(256), 0, ST, g, weight, labels, out, (long long)N * F,
            F, K);
  return GL_CHECK_LAUNCH();
}

int ganlab_proj_dweight_f32(const float* g, const float* f, const int* labels, float* out, int N, long long F, int K,
                            void* stream) {
  if (!g || !f || !labels || !out || N <= 0 || F <= 0 || K <= 0) return GANLAB_EINVAL;
  GL_LAUNCH(proj_dweight_kernel, dim3((unsigned)(((long long)K * F + 255) / 256)), dim3(256), 0, ST, g, f, labels, out, N, F,
            K);
  return GL_CHECK_LAUNCH();
}

int ganlab_randint_i32(int* out, long long n, int high, uint64_t seed, uint64_t offset, void* stream) {
  if (!out || n <= 0 || high <= 0 || high > (1 << 24)) return GANLAB_EINVAL;
  const long long groups = (n + 3) / 4;
  GL_LAUNCH(randint_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, ST, out, n, high, seed, offset);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
