// Consistency regularisation of the ResNet GAN (consistency.py): bCR (Zhang et al. 2020) compares the critic on an
// image and on its flipped / shifted copy, zCR (Zhao et al. 2020) the critic and the generator on a latent and on its perturbed copy.
// What the terms need beyond the kernels already there: one integer image transform and two mean-squared-difference reductions with
// their gradients.  No atomics, every sum in a fixed order: two runs are bitwise equal.  Nothing is read back by the host.
//
// cr_params     one thread per image, ONE Philox counter (offset + n): word 0 -> the flip bit, words 1, 2 -> dx, dy uniform in
//               [-s, s] (the integer pick of diffaug_params_kernel: lo + floor(u * count) on the 24-bit u, exact).  Row n of the
//               (N, 4) int32 table is (flip, dx, dy, 0); a short draw is a prefix of a long one.
// cr_transform  y[n,c,i,j] = x[n,c,i-dy, f(j-dx)], f the mirror when the row's flip is set, 0 where (i-dy, j-dx) leaves the image.
//               One launch over the batch; four outputs of a row per thread and a 16-byte store where W % 4 == 0 and y is aligned
//               (the gather side stays scalar: a shift or a mirror breaks its alignment anyway), else one output per thread.
//               Values are moved or zeroed, never computed with: bit-exact.
// cr_msd        mean_n (a_n - b_n)^2 of two score vectors: one workgroup, fp32 differences squared in fp32, summed in fp64 (thread
//               t takes n = t, t + 256, ...; then the block tree), rounded once.  Backward: ga = (2/N)(a - b) gout, gb = -ga.
// cr_imsd       the same mean over every element of two image batches.  Forward: thread t of the grid takes the groups of four
//               elements t, t + threads, ... - the SAME groups whether they are loaded as one float4 or as four floats, so the sum
//               does not depend on the operands' alignment - keeps an fp64 partial, the block tree leaves one fp64 partial per
//               workgroup, and a second one-workgroup launch adds the partials in index order.  Backward: one launch reads both
//               images and writes both gradients; the two may be the halves of one tensor.
#include "common.h"

namespace {

constexpr int CR_MAX_BLOCKS = 1024;       // imsd partials: 4 workgroups per CU at most

__global__ __launch_bounds__(256) void cr_params_kernel(int* __restrict__ out, int N, int shift, int flip, uint64_t seed,
                                                        uint64_t offset, const uint64_t* __restrict__ base) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  if (base != nullptr) offset += *base;
  const uint64_t ctr = offset + (uint64_t)n;
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  auto pick = [](uint32_t word, int lo, int count) { return lo + (int)(((uint64_t)(word >> 8) * (uint64_t)count) >> 24); };
  int4 r;
  r.x = flip ? pick(c[0], 0, 2) : 0;
  r.y = pick(c[1], -shift, 2 * shift + 1);
  r.z = pick(c[2], -shift, 2 * shift + 1);
  r.w = 0;
  reinterpret_cast<int4*>(out)[n] = r;
}

// source element of output (i, j) of one plane, or 0
__device__ __forceinline__ float cr_fetch(const float* __restrict__ plane, int i, int j, int H, int W, int flip, int dx, int dy) {
  const int si = i - dy, k = j - dx;
  if (si < 0 || si >= H || k < 0 || k >= W) return 0.f;
  return plane[(long long)si * W + (flip ? W - 1 - k : k)];
}

template <bool VEC>
__global__ __launch_bounds__(256) void cr_transform_kernel(const float* __restrict__ x, const int* __restrict__ params,
                                                           float* __restrict__ y, long long items, int C, int H, int W) {
  const int wq = VEC ? W >> 2 : W;        // items per row
  for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < items; it += (long long)gridDim.x * blockDim.x) {
    const long long row = it / wq;
    const int q = (int)(it - row * wq);
    const long long plane = row / H;
    const int i = (int)(row - plane * H);
    const long long n = plane / C;
    const int4 p = reinterpret_cast<const int4*>(params)[n];
    const float* __restrict__ src = x + plane * ((long long)H * W);
    if (VEC) {
      float4 o;
      o.x = cr_fetch(src, i, 4 * q, H, W, p.x, p.y, p.z);
      o.y = cr_fetch(src, i, 4 * q + 1, H, W, p.x, p.y, p.z);
      o.z = cr_fetch(src, i, 4 * q + 2, H, W, p.x, p.y, p.z);
      o.w = cr_fetch(src, i, 4 * q + 3, H, W, p.x, p.y, p.z);
      reinterpret_cast<float4*>(y)[it] = o;
    } else {
      y[it] = cr_fetch(src, i, q, H, W, p.x, p.y, p.z);
    }
  }
}

__device__ __forceinline__ double cr_sq(float a, float b) {
  const float d = a - b;
  return (double)(d * d);
}

__global__ __launch_bounds__(256) void cr_msd_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ out, int N) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) acc += cr_sq(a[n], b[n]);
  acc = gl_block_sum_256d(acc, red);
  if (threadIdx.x == 0) out[0] = (float)(acc / (double)N);
}

// ga = ((a - b) * (2 / count)) * gout, gb = -ga; four elements per thread where every pointer is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void cr_sqdiff_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ gout, float* __restrict__ ga,
                                                            float* __restrict__ gb, long long n, float two_over_n) {
  const float g = gout[0];
  const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
  const long long n4 = VEC ? (n >> 2) : 0;
  for (long long i = tid; i < n4; i += nth) {
    const float4 va = reinterpret_cast<const float4*>(a)[i], vb = reinterpret_cast<const float4*>(b)[i];
    float4 o;
    o.x = ((va.x - vb.x) * two_over_n) * g;
    o.y = ((va.y - vb.y) * two_over_n) * g;
    o.z = ((va.z - vb.z) * two_over_n) * g;
    o.w = ((va.w - vb.w) * two_over_n) * g;
    reinterpret_cast<float4*>(ga)[i] = o;
    reinterpret_cast<float4*>(gb)[i] = float4{-o.x, -o.y, -o.z, -o.w};
  }
  for (long long i = n4 * 4 + tid; i < n; i += nth) {
    const float o = ((a[i] - b[i]) * two_over_n) * g;
    ga[i] = o;
    gb[i] = -o;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void cr_imsd_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              double* __restrict__ part, long long n) {
  __shared__ double red[4];
  const long long groups = (n + 3) >> 2;
  double acc = 0.0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < groups; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 4;
    if (VEC && e + 4 <= n) {
      const float4 va = reinterpret_cast<const float4*>(a)[i], vb = reinterpret_cast<const float4*>(b)[i];
      acc += cr_sq(va.x, vb.x);
      acc += cr_sq(va.y, vb.y);
      acc += cr_sq(va.z, vb.z);
      acc += cr_sq(va.w, vb.w);
    } else {
      const long long end = e + 4 < n ? e + 4 : n;
      for (long long k = e; k < end; ++k) acc += cr_sq(a[k], b[k]);
    }
  }
  acc = gl_block_sum_256d(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void cr_imsd_finish_kernel(const double* __restrict__ part, float* __restrict__ out, int blocks,
                                                             long long n) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < blocks; i += 256) acc += part[i];
  acc = gl_block_sum_256d(acc, red);
  if (threadIdx.x == 0) out[0] = (float)(acc / (double)n);
}

// workgroups of the imsd forward: a function of the element count alone (the summation order must not depend on anything else)
inline int cr_imsd_blocks(long long n) {
  const long long b = ((n + 3) / 4 + 1023) / 1024;       // four groups of four per thread before a second workgroup is worth it
  return (int)(b < 1 ? 1 : (b > CR_MAX_BLOCKS ? CR_MAX_BLOCKS : b));
}

inline unsigned cr_stream_blocks(long long items) {
  const long long b = (items + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 256 * 8 ? 256 * 8 : b));
}

inline bool cr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int cr_sqdiff_bwd(const float* a, const float* b, const float* gout, float* ga, float* gb, long long n, void* stream) {
  if (!a || !b || !gout || !ga || !gb || n <= 0) return GANLAB_EINVAL;
  const float c = (float)(2.0 / (double)n);
  const bool vec = cr_aligned16(a) && cr_aligned16(b) && cr_aligned16(ga) && cr_aligned16(gb);
  const unsigned blocks = cr_stream_blocks(vec ? (n + 3) / 4 : n);
  if (vec)
    GL_LAUNCH(cr_sqdiff_bwd_kernel<true>, dim3(blocks), dim3(256), 0, gl_stream(stream), a, b, gout, ga, gb, n, c);
  else
    GL_LAUNCH(cr_sqdiff_bwd_kernel<false>, dim3(blocks), dim3(256), 0, gl_stream(stream), a, b, gout, ga, gb, n, c);
  return GL_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

int ganlab_cr_params_i32(int* out, int N, int shift, int flip, uint64_t seed, uint64_t offset, const void* base, void* stream) {
  if (!out || N <= 0 || shift < 0 || shift > (1 << 20) || !cr_aligned16(out)) return GANLAB_EINVAL;
  GL_LAUNCH(cr_params_kernel, dim3((N + 255) / 256), dim3(256), 0, gl_stream(stream), out, N, shift, flip ? 1 : 0, seed, offset,
            reinterpret_cast<const uint64_t*>(base));
  return GL_CHECK_LAUNCH();
}

int ganlab_cr_transform_f32(const float* x, const int* params, float* y, int N, int C, int H, int W, void* stream) {
  if (!x || !params || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || !cr_aligned16(params)) return GANLAB_EINVAL;
  const long long total = (long long)N * C * H * W;
  if ((W & 3) == 0 && cr_aligned16(y)) {
    GL_LAUNCH(cr_transform_kernel<true>, dim3(cr_stream_blocks(total / 4)), dim3(256), 0, gl_stream(stream), x, params, y,
              total / 4, C, H, W);
  } else {
    GL_LAUNCH(cr_transform_kernel<false>, dim3(cr_stream_blocks(total)), dim3(256), 0, gl_stream(stream), x, params, y, total, C,
              H, W);
  }
  return GL_CHECK_LAUNCH();
}

int ganlab_cr_msd_fwd_f32(const float* a, const float* b, float* out, int N, void* stream) {
  if (!a || !b || !out || N <= 0) return GANLAB_EINVAL;
  GL_LAUNCH(cr_msd_fwd_kernel, dim3(1), dim3(256), 0, gl_stream(stream), a, b, out, N);
  return GL_CHECK_LAUNCH();
}

int ganlab_cr_msd_bwd_f32(const float* a, const float* b, const float* gout, float* ga, float* gb, int N, void* stream) {
  return cr_sqdiff_bwd(a, b, gout, ga, gb, N, stream);
}

size_t ganlab_cr_imsd_workspace(long long n) { return n > 0 ? (size_t)cr_imsd_blocks(n) * sizeof(double) : 0; }

int ganlab_cr_imsd_fwd_f32(const float* a, const float* b, float* out, long long n, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (!a || !b || !out || n <= 0) return GANLAB_EINVAL;
  const int blocks = cr_imsd_blocks(n);
  if (!workspace || workspace_bytes < (size_t)blocks * sizeof(double) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return GANLAB_EWORKSPACE;
  double* part = reinterpret_cast<double*>(workspace);
  if (cr_aligned16(a) && cr_aligned16(b))
    GL_LAUNCH(cr_imsd_partial_kernel<true>, dim3(blocks), dim3(256), 0, gl_stream(stream), a, b, part, n);
  else
    GL_LAUNCH(cr_imsd_partial_kernel<false>, dim3(blocks), dim3(256), 0, gl_stream(stream), a, b, part, n);
  GL_LAUNCH(cr_imsd_finish_kernel, dim3(1), dim3(256), 0, gl_stream(stream), (const double*)part, out, blocks, n);
  return GL_CHECK_LAUNCH();
}

int ganlab_cr_imsd_bwd_f32(const float* a, const float* b, const float* gout, float* ga, float* gb, long long n, void* stream) {
  return cr_sqdiff_bwd(a, b, gout, ga, gb, n, stream);
}

}  // extern "C"
