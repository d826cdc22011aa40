// The sampling side of the ResNet GAN (sampling.py): truncated-normal latents and the moving average of the
// BatchNorm buffers of the averaged generator.  Two streaming kernels, no atomics, no reductions: every output element is a pure
// function of its own inputs, so two runs are bitwise equal whatever the launch geometry.
//
// trunc_randn   the standard normal truncated to [-t, t] by inverse CDF (BigGAN's truncation trick without its rejection loop: no
//               data-dependent trip count, and the stream advances exactly as ganlab_randn_f32's does).  Element i takes word i % 4
//               of Philox counter offset + i / 4 (randn_kernel's counters):
//                 k = word >> 9                 23 bits
//                 u = (k + 1/2) 2^-23           uniform on the open interval (0, 1)
//                 v = 2u - 1 = (2k + 1 - 2^23) 2^-23      an odd multiple of 2^-23 in (-1, 1): exact in fp32, symmetric, never 0
//                 x = sqrt(2) erfinv(v p),  p = erf(t / sqrt(2))  (formed in double on the host, rounded once)
//               clamped to [-t, t] (erfinvf may overshoot by an ulp).  One thread per counter: a 16-byte store of its four values,
//               scalar stores for the last partial group (or an unaligned destination).
// ewma_many     lagged = decay * lagged + (1 - decay) * src over a device-resident table of (dst, src, count) segments in one
//               launch: grid.y = the segment, grid.x strides over its elements, four per thread where both pointers are 16-byte
//               aligned.  The arithmetic is fp64 (the kernel is bound by its loads), rounded once to fp32.  decay = 0 copies and
//               never reads `lagged`: an uninitialised (NaN / inf) average cannot leak through 0 * lagged.
#include "common.h"

namespace {

constexpr int EW_MAX_BLOCKS = 256 * 8;
inline unsigned ew_blocks(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > EW_MAX_BLOCKS ? EW_MAX_BLOCKS : b));
}

__device__ __forceinline__ float trunc_normal_of_word(uint32_t word, float t, float p) {
  const int s = (int)((word >> 9) << 1) + 1 - (1 << 23);      // 2k + 1 - 2^23
  const float v = (float)s * (1.0f / 8388608.0f);
  const float x = 1.41421356237309504880f * erfinvf(v * p);
  return fminf(fmaxf(x, -t), t);
}

__global__ __launch_bounds__(256) void trunc_randn_kernel(float* __restrict__ out, long long n, float t, float p, uint64_t seed,
                                                          uint64_t offset, int vec) {
  const long long n4 = (n + 3) >> 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const uint64_t ctr = offset + (uint64_t)i;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    float4 r;
    r.x = trunc_normal_of_word(c[0], t, p);
    r.y = trunc_normal_of_word(c[1], t, p);
    r.z = trunc_normal_of_word(c[2], t, p);
    r.w = trunc_normal_of_word(c[3], t, p);
    const long long e = i * 4;
    if (vec && e + 4 <= n) {
      reinterpret_cast<float4*>(out)[i] = r;
    } else {
      if (e < n) out[e] = r.x;
      if (e + 1 < n) out[e + 1] = r.y;
      if (e + 2 < n) out[e + 2] = r.z;
      if (e + 3 < n) out[e + 3] = r.w;
    }
  }
}

__device__ __forceinline__ float ewma_one(float lag, float src, double d) {
  return (float)(d * (double)lag + (1.0 - d) * (double)src);
}

constexpr int EWMA_GX = 8;      // blocks per segment: 8 * 256 threads * 4 elements per pass

__global__ __launch_bounds__(256) void ewma_many_kernel(const ganlab_ewma_job* __restrict__ jobs, float decay) {
  const ganlab_ewma_job job = jobs[blockIdx.y];
  float* __restrict__ dst = job.dst;
  const float* __restrict__ src = job.src;
  const long long n = job.count;
  const double d = (double)decay;
  const bool copy = decay == 0.f;
  const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
  const long long n4 = vec ? (n >> 2) : 0;
  for (long long i = tid; i < n4; i += nth) {
    const float4 s = reinterpret_cast<const float4*>(src)[i];
    float4 o = s;
    if (!copy) {
      const float4 l = reinterpret_cast<const float4*>(dst)[i];
      o.x = ewma_one(l.x, s.x, d);
      o.y = ewma_one(l.y, s.y, d);
      o.z = ewma_one(l.z, s.z, d);
      o.w = ewma_one(l.w, s.w, d);
    }
    reinterpret_cast<float4*>(dst)[i] = o;
  }
  for (long long i = n4 * 4 + tid; i < n; i += nth) dst[i] = copy ? src[i] : ewma_one(dst[i], src[i], d);
}

}  // namespace

#define ST gl_stream(stream)

extern "C" {

int ganlab_trunc_randn_f32(float* out, long long n, float threshold, uint64_t seed, uint64_t offset, void* stream) {
  if (!out || n <= 0 || !(threshold > 0.f) || !(threshold <= 3.0e38f)) return GANLAB_EINVAL;
  const float p = (float)erf((double)threshold * 0.70710678118654752440);
  const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  GL_LAUNCH(trunc_randn_kernel, dim3(ew_blocks((n + 3) / 4)), dim3(256), 0, ST, out, n, threshold, p, seed, offset, vec);
  return GL_CHECK_LAUNCH();
}

int ganlab_ewma_job_size(void) { return (int)sizeof(ganlab_ewma_job); }

int ganlab_ewma_many_f32(const ganlab_ewma_job* jobs_device, int n_jobs, float decay, void* stream) {
  if (!jobs_device || n_jobs <= 0 || n_jobs > 65535 || !(decay >= 0.f) || !(decay < 1.f)) return GANLAB_EINVAL;
  GL_LAUNCH(ewma_many_kernel, dim3(EWMA_GX, (unsigned)n_jobs), dim3(256), 0, ST, jobs_device, decay);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
