// Perceptual path length (Karras et al. 2019, the StyleGAN paper's metric): the three kernels behind gan_lab_amd/ppl.py,
// DESIGN.md 4.22.
//   ppl_endpoints   t (N,) and out (2, N, D) from a, b (N, D): out[0] the point of the path a -> b at t, out[1] at t + eps, in ONE
//                   launch, one 256-thread workgroup per row (D <= 4096: a row lives in 16 registers per thread).
//                     t        sampling 'full': word 0 of Philox4x32-10 on counter offset + n under the key, (word >> 8) 2^-24 in
//                              [0, 1) - one counter per row, so a short draw is the prefix of a long one; 'end': 0.
//                     lerp     a + (b - a) t, formed per entry in double from the fp32 operands and rounded ONCE; t + eps is a
//                              double sum, so both ends are within half an ulp of the exact value.
//                     slerp    StyleGAN's: ah = a / |a|, bh = b / |b|, d = clamp(<ah, bh>, -1, 1), c = bh - d ah, ch = c / |c|,
//                              r = ah cos p + ch sin p at p = t acos(d), out = r sqrt(D / |r|^2).  The five row reductions (|a|^2,
//                              |b|^2, <ah, bh>, |c|^2, |r|^2 per end) are fp32 sums over the workgroup in a fixed order; the
//                              per-row scalars behind them (acos, the two angles, their sines and cosines, the final scale) are
//                              formed in double from the fp32 sums and rounded once - 256 lanes repeat them, which costs nothing
//                              beside the generator passes the points feed.  |c|^2 < 2^-30 (rows within 3e-5 rad of parallel or
//                              antipodal: fp32 cannot resolve the direction of c there), |a| = 0 or |b| = 0: both ends are
//                              ah sqrt(D), ah = a itself where |a| = 0.  Finite whenever a and b are.
//   row_sqdist      out[n] = sum_j (x[n, j] - y[n, j])^2: differences, squares and sums in double, rounded once; one workgroup per
//                   row, any D.
//   trimmed_mean    rocPRIM radix sort of the n values, then one workgroup: lo = sorted[i_lo], hi = sorted[i_hi], the count and the
//                   fp64 sum of the values with lo <= v <= hi (decided by comparison: ties at either bound are all kept), each of
//                   1024 threads adding every 1024th value of the SORTED array in ascending index order, the partials joined by a
//                   fixed tree.
// No atomics anywhere, nothing depends on timing: bitwise reproducible.
#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace {

constexpr int kMaxD = GANLAB_PPL_MAX_DIM;
constexpr int kPerThread = kMaxD / 256;
constexpr float kParallel = 9.313225746154785e-10f;          // 2^-30

__device__ __forceinline__ float ppl_uniform(uint64_t seed, uint64_t ctr) {
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (float)(c[0] >> 8) * 5.9604644775390625e-08f;         // 2^-24: exact
}

template <bool SLERP>
__global__ __launch_bounds__(256) void ppl_endpoints_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ t_out, float* __restrict__ out, long long N, int D,
                                                            double eps, int full, uint64_t seed, uint64_t offset) {
  __shared__ float red[4];
  const long long n = blockIdx.x;
  const int tid = threadIdx.x;
  const float t = full ? ppl_uniform(seed, offset + (uint64_t)n) : 0.f;
  if (tid == 0) t_out[n] = t;
  const double t0 = (double)t, t1 = (double)t + eps;
  const float* ar = a + n * D;
  const float* br = b + n * D;
  float* o0 = out + n * D;
  float* o1 = out + (N + n) * D;
  float av[kPerThread], bv[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int j = tid + 256 * k;
    av[k] = j < D ? ar[j] : 0.f;
    bv[k] = j < D ? br[j] : 0.f;
  }
  if (!SLERP) {
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int j = tid + 256 * k;
      if (j < D) {
        const double x = (double)av[k], dlt = (double)bv[k] - (double)av[k];
        o0[j] = (float)(x + dlt * t0);
        o1[j] = (float)(x + dlt * t1);
      }
    }
    return;
  }
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    sa += av[k] * av[k];
    sb += bv[k] * bv[k];
  }
  const float na = sqrtf(gl_block_sum_256(sa, red)), nb = sqrtf(gl_block_sum_256(sb, red));
  const float sqrt_d = (float)sqrt((double)D);
  const bool a_zero = !(na > 0.f);
  float sd = 0.f;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    av[k] = a_zero ? av[k] : av[k] / na;                   // padding entries stay 0
    bv[k] = nb > 0.f ? bv[k] / nb : 0.f;
    sd += av[k] * bv[k];
  }
  const float d = fminf(fmaxf(gl_block_sum_256(sd, red), -1.f), 1.f);
  float sc = 0.f;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    bv[k] = bv[k] - d * av[k];                             // c
    sc += bv[k] * bv[k];
  }
  const float nc2 = gl_block_sum_256(sc, red);
  if (a_zero || !(nb > 0.f) || !(nc2 >= kParallel)) {      // uniform over the workgroup: every lane holds the same sums
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int j = tid + 256 * k;
      if (j < D) o0[j] = o1[j] = av[k] * sqrt_d;
    }
    return;
  }
  const float nc = sqrtf(nc2);
  const double omega = acos((double)d);
  const float c0 = (float)cos(t0 * omega), s0 = (float)sin(t0 * omega);
  const float c1 = (float)cos(t1 * omega), s1 = (float)sin(t1 * omega);
  float r0[kPerThread], r1[kPerThread];
  float q0 = 0.f, q1 = 0.f;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const float ch = bv[k] / nc;
    r0[k] = av[k] * c0 + ch * s0;
    r1[k] = av[k] * c1 + ch * s1;
    q0 += r0[k] * r0[k];
    q1 += r1[k] * r1[k];
  }
  const float scale0 = (float)sqrt((double)D / (double)gl_block_sum_256(q0, red));
  const float scale1 = (float)sqrt((double)D / (double)gl_block_sum_256(q1, red));
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int j = tid + 256 * k;
    if (j < D) {
      o0[j] = r0[k] * scale0;
      o1[j] = r1[k] * scale1;
    }
  }
}

__global__ __launch_bounds__(256) void row_sqdist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         float* __restrict__ out, long long D) {
  __shared__ double red[4];
  const float* xr = x + (long long)blockIdx.x * D;
  const float* yr = y + (long long)blockIdx.x * D;
  double acc = 0.0;
  for (long long j = threadIdx.x; j < D; j += 256) {
    const double df = (double)xr[j] - (double)yr[j];
    acc += df * df;
  }
  acc = gl_block_sum_256d(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)acc;
}

constexpr int kTrimThreads = 1024;

// record: mean, lo, hi, kept, nonfinite
__global__ __launch_bounds__(kTrimThreads) void trimmed_mean_kernel(const float* __restrict__ sorted, long long n, long long i_lo,
                                                                     long long i_hi, double* __restrict__ record) {
  __shared__ double ssum[kTrimThreads];
  __shared__ long long skept[kTrimThreads];
  __shared__ long long sbad[kTrimThreads];
  const int tid = threadIdx.x;
  const float lo = sorted[i_lo], hi = sorted[i_hi];
  double sum = 0.0;
  long long kept = 0, bad = 0;
  for (long long i = tid; i < n; i += kTrimThreads) {
    const float v = sorted[i];
    if (!isfinite(v)) ++bad;
    if (v >= lo && v <= hi) {
      sum += (double)v;
      ++kept;
    }
  }
  ssum[tid] = sum;
  skept[tid] = kept;
  sbad[tid] = bad;
  __syncthreads();
  for (int s = kTrimThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      ssum[tid] += ssum[tid + s];
      skept[tid] += skept[tid + s];
      sbad[tid] += sbad[tid + s];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const bool ok = sbad[0] == 0;
  record[0] = ok ? ssum[0] / (double)skept[0] : nan;
  record[1] = ok ? (double)lo : nan;
  record[2] = ok ? (double)hi : nan;
  record[3] = ok ? (double)skept[0] : 0.0;
  record[4] = (double)sbad[0];
}

size_t ppl_align(size_t v) { return (v + 255) & ~(size_t)255; }

size_t trim_sort_temp(long long n) {
  size_t bytes = 0;
  float* none = nullptr;
  if (rocprim::radix_sort_keys(nullptr, bytes, none, none, (size_t)n) != hipSuccess) return 0;
  return ppl_align(bytes ? bytes : 1);
}

// numpy.percentile's position of quantile q among n sorted values: the double product (n - 1) q, ONE rounding - floor / ceil of
// it agree with numpy's 'lower' / 'higher' also at the n where the exact product is an integer
double trim_virtual_index(long long n, double q) { return (double)(n - 1) * q; }

}  // namespace

extern "C" int ganlab_ppl_endpoints_f32(const float* a, const float* b, float* t, float* out, long long N, int D, double eps,
                                        int mode, int sampling, uint64_t seed, uint64_t offset, void* stream) {
  if (!a || !b || !t || !out || N < 1 || N > 0x7fffffffLL || D < 1 || D > kMaxD) return GANLAB_EINVAL;
  if (!(eps > 0.0) || !(eps < 1.0)) return GANLAB_EINVAL;
  if ((mode != GANLAB_PPL_LERP && mode != GANLAB_PPL_SLERP) || (sampling != GANLAB_PPL_FULL && sampling != GANLAB_PPL_END))
    return GANLAB_EINVAL;
  hipStream_t st = gl_stream(stream);
  const dim3 grid((unsigned)N);
  if (mode == GANLAB_PPL_SLERP)
    GL_LAUNCH(ppl_endpoints_kernel<true>, grid, dim3(256), 0, st, a, b, t, out, N, D, eps, sampling == GANLAB_PPL_FULL, seed, offset);
  else
    GL_LAUNCH(ppl_endpoints_kernel<false>, grid, dim3(256), 0, st, a, b, t, out, N, D, eps, sampling == GANLAB_PPL_FULL, seed, offset);
  return GL_CHECK_LAUNCH();
}

extern "C" int ganlab_row_sqdist_f32(const float* x, const float* y, float* out, long long N, long long D, void* stream) {
  if (!x || !y || !out || N < 1 || N > 0x7fffffffLL || D < 1) return GANLAB_EINVAL;
  GL_LAUNCH(row_sqdist_kernel, dim3((unsigned)N), dim3(256), 0, gl_stream(stream), x, y, out, D);
  return GL_CHECK_LAUNCH();
}

extern "C" size_t ganlab_trimmed_mean_workspace(long long n) {
  if (n < 1 || n > 0x7fffffffLL) return 0;
  const size_t temp = trim_sort_temp(n);
  return temp ? temp + ppl_align((size_t)n * sizeof(float)) : 0;
}

extern "C" int ganlab_trimmed_mean_f32(const float* v, long long n, double q_lo, double q_hi, double* record, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  if (!v || !record || !workspace || n < 1 || n > 0x7fffffffLL) return GANLAB_EINVAL;
  if (!(q_lo >= 0.0) || !(q_hi <= 1.0) || !(q_lo <= q_hi)) return GANLAB_EINVAL;
  const size_t temp = trim_sort_temp(n);
  if (!temp) return GANLAB_EINVAL;
  if (workspace_bytes < temp + ppl_align((size_t)n * sizeof(float))) return GANLAB_EWORKSPACE;
  long long i_lo = (long long)floor(trim_virtual_index(n, q_lo)), i_hi = (long long)ceil(trim_virtual_index(n, q_hi));
  i_lo = i_lo < 0 ? 0 : (i_lo > n - 1 ? n - 1 : i_lo);
  i_hi = i_hi < 0 ? 0 : (i_hi > n - 1 ? n - 1 : i_hi);
  hipStream_t st = gl_stream(stream);
  float* sorted = reinterpret_cast<float*>(static_cast<char*>(workspace) + temp);
  size_t bytes = temp;
  if (rocprim::radix_sort_keys(workspace, bytes, v, sorted, (size_t)n, 0, 32, st) != hipSuccess) return GANLAB_ELAUNCH;
  GL_LAUNCH(trimmed_mean_kernel, dim3(1), dim3(kTrimThreads), 0, st, sorted, n, i_lo, i_hi, record);
  return GL_CHECK_LAUNCH();
}
