// Fused arena optimisers beside Adam (optim.py FusedRMSprop / FusedSGD / FusedOptimisticAdam): RMSprop, SGD with
// momentum and optimistic Adam over one flat run of n floats per launch.  Streaming kernels, no atomics, no reductions: every
// element is a pure function of its own inputs, so two runs are bitwise equal whatever the launch geometry.
//
// rmsprop   torch.optim.RMSprop(centered=False):  g' = g + wd p;  sq = alpha sq + (1 - alpha) g'^2;  d = g' / (sqrt(sq) + eps)
//           (eps OUTSIDE the root);  momentum > 0: buf = momentum buf + d, p -= lr buf;  else p -= lr d (buf is not touched).
// sgd       torch.optim.SGD(dampening=0, nesterov=False):  g' = g + wd p;  momentum > 0: buf = first ? g' : momentum buf + g',
//           p -= lr buf;  else p -= lr g'.
// oadam     optimistic Adam (Daskalakis et al. 2018, Algorithm 1):  m, v and the bias corrections are Adam's;
//           d = (m / bc1) / (sqrt(v) rsqrt(bc2) + eps) - the denominator is adam_kernel's (csrc/pointwise.hip) -;
//           p -= 2 lr d - lr prev;  prev = d.
//
// Geometry: adam_kernel's (at most 2048 blocks of 256 threads, grid-stride), but four elements per thread and trip through
// 16-byte loads and stores where every buffer is 16-byte aligned (an arena run always is), and a scalar loop over the last n % 4
// elements (or over everything, for an unaligned operand).  Padding floats of an arena have p = g = 0 and zero state: g' = 0,
// every state stays 0, d = 0 / (0 + eps) = 0 (eps > 0) and p stays 0.
// ``dev``: the per-step scalars of THIS step read from device memory - the step-graph form (graphs.py GraphedStep), see adam_kernel.
#include "common.h"

namespace {

constexpr int EW_MAX_BLOCKS = 256 * 8;
inline unsigned ew_blocks(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > EW_MAX_BLOCKS ? EW_MAX_BLOCKS : b));
}

template <bool MOM>
struct RmspropOp {
  static constexpr int NS = MOM ? 2 : 1;      // sq[, buf]
  float lr, alpha, eps, wd, mom;
  __device__ __forceinline__ void read(const float* __restrict__ dev) { lr = dev[0]; }
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void apply(float& p, float g, float* s) const {
    if (wd != 0.f) g += wd * p;
    const float sq = alpha * s[0] + (1.f - alpha) * g * g;
    s[0] = sq;
    const float d = g / (sqrtf(sq) + eps);
    if (MOM) {
      const float b = mom * s[1] + d;
      s[1] = b;
      p -= lr * b;
    } else {
      p -= lr * d;
    }
  }
};

template <bool MOM>
struct SgdOp {
  static constexpr int NS = MOM ? 1 : 0;      // [buf]
  float lr, wd, mom, first;
  __device__ __forceinline__ void read(const float* __restrict__ dev) {
    lr = dev[0];
    first = dev[1];
  }
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void apply(float& p, float g, float* s) const {
    if (wd != 0.f) g += wd * p;
    if (MOM) {
      const float b = first != 0.f ? g : mom * s[0] + g;
      s[0] = b;
      p -= lr * b;
    } else {
      p -= lr * g;
    }
  }
};

struct OadamOp {
  static constexpr int NS = 3;                // m, v, prev
  float lr, b1, b2, eps, wd, bc1, bc2, isq;
  __device__ __forceinline__ void read(const float* __restrict__ dev) {
    lr = dev[0];
    bc1 = dev[1];
    bc2 = dev[2];
  }
  __device__ __forceinline__ void prepare() { isq = rsqrtf(bc2); }
  __device__ __forceinline__ void apply(float& p, float g, float* s) const {
    if (wd != 0.f) g += wd * p;
    const float mi = b1 * s[0] + (1.f - b1) * g;
    const float vi = b2 * s[1] + (1.f - b2) * g * g;
    s[0] = mi;
    s[1] = vi;
    const float d = (mi / bc1) / (sqrtf(vi) * isq + eps);
    p -= 2.f * lr * d - lr * s[2];
    s[2] = d;
  }
};

template <class Op>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                    float* __restrict__ s1, float* __restrict__ s2, long long n, int vec, Op op,
                                                    const float* __restrict__ dev) {
  constexpr int NS = Op::NS, NA = NS > 0 ? NS : 1;
  if (dev != nullptr) op.read(dev);
  op.prepare();
  float* const s[3] = {s0, s1, s2};
  const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
  const long long n4 = vec ? (n >> 2) : 0;
  for (long long i = tid; i < n4; i += nth) {
    const float4 pv = reinterpret_cast<const float4*>(p)[i], gv = reinterpret_cast<const float4*>(g)[i];
    float pa[4] = {pv.x, pv.y, pv.z, pv.w};
    const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
    float sa[NA][4];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const float4 sv = reinterpret_cast<const float4*>(s[k])[i];
      sa[k][0] = sv.x, sa[k][1] = sv.y, sa[k][2] = sv.z, sa[k][3] = sv.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float st[NA];
#pragma unroll
      for (int k = 0; k < NS; ++k) st[k] = sa[k][j];
      op.apply(pa[j], ga[j], st);
#pragma unroll
      for (int k = 0; k < NS; ++k) sa[k][j] = st[k];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) reinterpret_cast<float4*>(s[k])[i] = make_float4(sa[k][0], sa[k][1], sa[k][2], sa[k][3]);
    reinterpret_cast<float4*>(p)[i] = make_float4(pa[0], pa[1], pa[2], pa[3]);
  }
  for (long long i = n4 * 4 + tid; i < n; i += nth) {
    float pi = p[i];
    float st[NA];
#pragma unroll
    for (int k = 0; k < NS; ++k) st[k] = s[k][i];
    op.apply(pi, g[i], st);
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k][i] = st[k];
    p[i] = pi;
  }
}

inline int all_aligned16(const void* a, const void* b, const void* c, const void* d, const void* e) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(e)) & 15) == 0;
}

// four elements per thread and trip where the 16-byte path runs
inline unsigned optim_blocks(long long n, int vec) { return ew_blocks(vec ? (n + 3) / 4 : n); }

}  // namespace

#define ST gl_stream(stream)

static int rmsprop_launch(float* p, const float* g, float* sq, float* buf, long long n, float lr, float alpha, float eps, float wd,
                          float momentum, const float* dev, void* stream) {
  if (!p || !g || !sq || n <= 0 || !(momentum >= 0.f) || (momentum > 0.f && !buf)) return GANLAB_EINVAL;
  if (momentum > 0.f) {
    const int vec = all_aligned16(p, g, sq, buf, nullptr);
    GL_LAUNCH(optim_kernel<RmspropOp<true>>, dim3(optim_blocks(n, vec)), dim3(256), 0, ST, p, g, sq, buf, (float*)nullptr, n, vec,
              (RmspropOp<true>{lr, alpha, eps, wd, momentum}), dev);
  } else {
    const int vec = all_aligned16(p, g, sq, nullptr, nullptr);
    GL_LAUNCH(optim_kernel<RmspropOp<false>>, dim3(optim_blocks(n, vec)), dim3(256), 0, ST, p, g, sq, (float*)nullptr,
              (float*)nullptr, n, vec, (RmspropOp<false>{lr, alpha, eps, wd, 0.f}), dev);
  }
  return GL_CHECK_LAUNCH();
}

static int sgd_launch(float* p, const float* g, float* buf, long long n, float lr, float wd, float momentum, float first,
                      const float* dev, void* stream) {
  if (!p || !g || n <= 0 || !(momentum >= 0.f) || (momentum > 0.f && !buf)) return GANLAB_EINVAL;
  if (momentum > 0.f) {
    const int vec = all_aligned16(p, g, buf, nullptr, nullptr);
    GL_LAUNCH(optim_kernel<SgdOp<true>>, dim3(optim_blocks(n, vec)), dim3(256), 0, ST, p, g, buf, (float*)nullptr, (float*)nullptr,
              n, vec, (SgdOp<true>{lr, wd, momentum, first}), dev);
  } else {
    const int vec = all_aligned16(p, g, nullptr, nullptr, nullptr);
    GL_LAUNCH(optim_kernel<SgdOp<false>>, dim3(optim_blocks(n, vec)), dim3(256), 0, ST, p, g, (float*)nullptr, (float*)nullptr,
              (float*)nullptr, n, vec, (SgdOp<false>{lr, wd, 0.f, 0.f}), dev);
  }
  return GL_CHECK_LAUNCH();
}

static int oadam_launch(float* p, const float* g, float* m, float* v, float* prev, long long n, float lr, float beta1, float beta2,
                        float eps, float wd, float bc1, float bc2, const float* dev, void* stream) {
  const int vec = all_aligned16(p, g, m, v, prev);
  GL_LAUNCH(optim_kernel<OadamOp>, dim3(optim_blocks(n, vec)), dim3(256), 0, ST, p, g, m, v, prev, n, vec,
            (OadamOp{lr, beta1, beta2, eps, wd, bc1, bc2, 1.f}), dev);
  return GL_CHECK_LAUNCH();
}

extern "C" {

int ganlab_rmsprop_f32(float* p, const float* g, float* sq, float* buf, long long n, float lr, float alpha, float eps, float wd,
                       float momentum, void* stream) {
  return rmsprop_launch(p, g, sq, buf, n, lr, alpha, eps, wd, momentum, nullptr, stream);
}

int ganlab_rmsprop_dev_f32(float* p, const float* g, float* sq, float* buf, long long n, const float* lr_x_x, float alpha,
                           float eps, float wd, float momentum, void* stream) {
  if (!lr_x_x) return GANLAB_EINVAL;
  return rmsprop_launch(p, g, sq, buf, n, 0.f, alpha, eps, wd, momentum, lr_x_x, stream);
}

int ganlab_sgd_f32(float* p, const float* g, float* buf, long long n, float lr, float wd, float momentum, int first,
                   void* stream) {
  return sgd_launch(p, g, buf, n, lr, wd, momentum, first ? 1.f : 0.f, nullptr, stream);
}

int ganlab_sgd_dev_f32(float* p, const float* g, float* buf, long long n, const float* lr_first_x, float wd, float momentum,
                       void* stream) {
  if (!lr_first_x) return GANLAB_EINVAL;
  return sgd_launch(p, g, buf, n, 0.f, wd, momentum, 0.f, lr_first_x, stream);
}

int ganlab_oadam_f32(float* p, const float* g, float* m, float* v, float* prev, long long n, float lr, float beta1, float beta2,
                     float eps, float wd, float bc1, float bc2, void* stream) {
  if (!p || !g || !m || !v || !prev || n <= 0 || bc1 <= 0.f || bc2 <= 0.f) return GANLAB_EINVAL;
  return oadam_launch(p, g, m, v, prev, n, lr, beta1, beta2, eps, wd, bc1, bc2, nullptr, stream);
}

int ganlab_oadam_dev_f32(float* p, const float* g, float* m, float* v, float* prev, long long n, const float* lr_bc1_bc2,
                         float beta1, float beta2, float eps, float wd, void* stream) {
  if (!p || !g || !m || !v || !prev || n <= 0 || !lr_bc1_bc2) return GANLAB_EINVAL;
  return oadam_launch(p, g, m, v, prev, n, 0.f, beta1, beta2, eps, wd, 1.f, 1.f, lr_bc1_bc2, stream);
}

}  // extern "C"
