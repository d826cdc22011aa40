// DiffAugment (Zhao et al. 2020, "Differentiable Augmentation for Data-Efficient GAN Training") of the critic's inputs:
// a per-sample random, differentiable map of an (N, 3, H, W) fp32 batch - color (brightness, saturation, contrast),
// translation with zero fill, cutout - and its adjoint.  DESIGN.md "DiffAugment" has the math; in short, with
// m = mean_chw(x), mc = mean_c(x) (per pixel) and p[n] = (b, s, c, tx, ty, ox, oy, 0):
//   forward   y[i, j]  = keep(i, j) && inside(i + tx, j + ty) ? cs x + c(1 - s) mc + (1 - c) m + b  at (i + tx, j + ty) : 0
//   backward  g1[i, j] = keep(i - tx, j - ty) && inside(i - tx, j - ty) ? g[i - tx, j - ty] : 0
//             gx       = cs g1 + c(1 - s) mean_c(g1) + (1 - c) mean_chw(g1)
// Each direction is one fixed-order per-sample reduction (only with color) and one gather pass.  No float atomics: the
// per-sample sum has a fixed chunking that depends on (H, W) only, so a sample's result does not depend on the batch it
// sits in (the paired critic pass augments [generated; real] in one launch) and two calls agree bit for bit.
#include "common.h"

namespace {

constexpr int kSumChunk = 16384;   // elements of one sample per reduction workgroup (256 threads x 16 float4)

__host__ __device__ inline int da_chunks(int H, int W) {
  const long long per = 3LL * H * W;
  return (int)((per + kSumChunk - 1) / kSumChunk);
}

// sh/sw = int(0.125 H + 0.5), ch/cw = int(0.5 H + 0.5)
__host__ __device__ inline int da_shift(int H) { return (H + 4) / 8; }
__host__ __device__ inline int da_cut(int H) { return (H + 1) / 2; }

struct DaParams {
  float A, B, b, c;        // A = c s, B = c (1 - s)
  int tx, ty;              // translation (0 without it)
  int r0, r1, c0, c1;      // cut rectangle [r0, r1) x [c0, c1) (empty without cutout)
};

__device__ __forceinline__ DaParams da_load(const float* __restrict__ p, int H, int W, int pol) {
  DaParams d;
  const float b = p[0], s = p[1], c = p[2];
  if (pol & GANLAB_DIFFAUG_COLOR) {
    d.A = c * s;
    d.B = c * (1.f - s);
    d.b = b;
    d.c = c;
  } else {
    d.A = 1.f; d.B = 0.f; d.b = 0.f; d.c = 1.f;
  }
  d.tx = (pol & GANLAB_DIFFAUG_TRANSLATION) ? (int)p[3] : 0;
  d.ty = (pol & GANLAB_DIFFAUG_TRANSLATION) ? (int)p[4] : 0;
  if (pol & GANLAB_DIFFAUG_CUTOUT) {
    const int ch = da_cut(H), cw = da_cut(W);
    d.r0 = (int)p[5] - ch / 2;
    d.r1 = d.r0 + ch;
    d.c0 = (int)p[6] - cw / 2;
    d.c1 = d.c0 + cw;
  } else {
    d.r0 = d.r1 = d.c0 = d.c1 = 0;
  }
  return d;
}

// output pixel (i, j) of the forward carries a value: not cut, and its source (i + tx, j + ty) is inside the image
__device__ __forceinline__ bool da_live(const DaParams& d, int i, int j, int H, int W) {
  const bool cut = i >= d.r0 && i < d.r1 && j >= d.c0 && j < d.c1;
  const int si = i + d.tx, sj = j + d.ty;
  return !cut && si >= 0 && si < H && sj >= 0 && sj < W;
}

// Stage 1.  part[n * chunks + k] = sum of chunk k of sample n: the plain sum of x (forward), or of the cotangent over the
// live output pixels (MASKED: the backward's sum of g1).  Threads accumulate fp32 over <= 16 float4, the workgroup in fp64.
template <bool MASKED>
__global__ __launch_bounds__(256) void diffaug_sum_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                          double* __restrict__ part, int H, int W, int pol) {
  __shared__ double red[4];
  const int n = blockIdx.y, k = blockIdx.x, chunks = gridDim.x;
  const long long hw = (long long)H * W, per = 3 * hw;
  const float* xs = x + n * per;
  const long long e0 = (long long)k * kSumChunk, e1 = e0 + kSumChunk < per ? e0 + kSumChunk : per;
  DaParams d;
  int i = 0, j = 0, di = 0, dj = 0;
  if (MASKED) {
    // the pixel (row i, column j) of element e, kept up to date as e advances by 1024 (di rows + dj columns): one division per
    // thread instead of one per float4 (the channel is irrelevant to the mask; rows wrap into the next channel)
    d = da_load(params + 8 * n, H, W, pol);
    const long long e = e0 + 4 * threadIdx.x;
    const int pix = (int)(e - (e >= 2 * hw ? 2 * hw : e >= hw ? hw : 0));
    i = pix / W;
    j = pix - i * W;
    di = 1024 / W;
    dj = 1024 - di * W;
  }
  float acc = 0.f;
  for (long long e = e0 + 4 * threadIdx.x; e < e1; e += 1024) {      // per % 4 == 0 (W % 4 == 0)
    const float4 v = *reinterpret_cast<const float4*>(xs + e);
    if (MASKED) {
      acc += (da_live(d, i, j, H, W) ? v.x : 0.f) + (da_live(d, i, j + 1, H, W) ? v.y : 0.f) +
             (da_live(d, i, j + 2, H, W) ? v.z : 0.f) + (da_live(d, i, j + 3, H, W) ? v.w : 0.f);
      i += di;
      j += dj;
      if (j >= W) {
        j -= W;
        ++i;
      }
      while (i >= H) i -= H;       // at most 1 + 1024 / (H W) turns: more than one float4 per thread needs H W > 1024 / 3
    } else {
      acc += (v.x + v.y) + (v.z + v.w);
    }
  }
  const double s = gl_block_sum_256d((double)acc, red);
  if (threadIdx.x == 0) part[(long long)n * chunks + k] = s;
}

// 4 consecutive floats starting r (0..3) floats into the 8 of (a, b)
__device__ __forceinline__ float4 da_window(const float4& a, const float4& b, int r) {
  switch (r) {
    case 0: return a;
    case 1: return float4{a.y, a.z, a.w, b.x};
    case 2: return float4{a.z, a.w, b.x, b.y};
    default: return float4{a.w, b.x, b.y, b.z};
  }
}

// Row `row` of a plane at columns [sj, sj + 4), zero outside [0, W) and where need[q] is false: two aligned 16-byte loads (W % 4 == 0,
// so an aligned quad is either wholly inside the row or wholly outside it); a quad none of whose needed columns is live is not
// loaded, nor is anything of a row outside the image
__device__ __forceinline__ float4 da_gather4(const float* __restrict__ plane, int row, int sj, int H, int W, const bool (&need)[4]) {
  const float4 z = float4{0.f, 0.f, 0.f, 0.f};
  if (row < 0 || row >= H) return z;
  const int r = sj & 3, a = sj - r;
  // pixel q sits at position r + q of the 8 floats (lo, hi): lo serves q < 4 - r, hi the rest
  bool need_lo = false, need_hi = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    need_lo |= need[q] && q < 4 - r;
    need_hi |= need[q] && q >= 4 - r;
  }
  const float* base = plane + (long long)row * W;
  const float4 lo = (need_lo && a >= 0 && a < W) ? *reinterpret_cast<const float4*>(base + a) : z;
  const float4 hi = (need_hi && r != 0 && a + 4 >= 0 && a + 4 < W) ? *reinterpret_cast<const float4*>(base + a + 4) : z;
  return da_window(lo, hi, r);
}

__device__ __forceinline__ float da_comp(const float4& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }

// Stage 2.  One thread = 4 consecutive pixels of one row and all 3 channels of them.  blockIdx.y = sample.
// FWD: out = live ? A x + B mc(x) + (1 - c) m + b : 0 at the shifted source.  !FWD: v = g at the back-shifted source where
// that source pixel was live in the forward, then out = A v + B mc(v) + (1 - c) mean(g1), at every pixel.
template <bool FWD>
__global__ __launch_bounds__(256) void diffaug_apply_kernel(const float* __restrict__ src, const float* __restrict__ params,
                                                            const double* __restrict__ part, float* __restrict__ dst, int H,
                                                            int W, int chunks, int pol) {
  __shared__ double red[4];
  const int n = blockIdx.y;
  const long long hw = (long long)H * W;
  const DaParams d = da_load(params + 8 * n, H, W, pol);
  float mean = 0.f;
  if (pol & GANLAB_DIFFAUG_COLOR) {       // the sample's sum: its chunk partials in a fixed order (same in every workgroup)
    double s = 0.0;
    for (int k = threadIdx.x; k < chunks; k += 256) s += part[(long long)n * chunks + k];
    mean = (float)(gl_block_sum_256d(s, red) / (double)(3 * hw));
  }
  const int wq = W / 4;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)H * wq) return;
  const int i = (int)(t / wq), j = (int)(t % wq) * 4;
  const float* s0 = src + (long long)n * 3 * hw;
  float* d0 = dst + (long long)n * 3 * hw + (long long)i * W + j;
  const float shift = FWD ? (1.f - d.c) * mean + d.b : (1.f - d.c) * mean;
  const int dy = FWD ? d.tx : -d.tx, dx = FWD ? d.ty : -d.ty;
  bool live[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)       // forward: the output pixel's own liveness; backward: that of its forward image
    live[q] = FWD ? da_live(d, i, j + q, H, W) : da_live(d, i - d.tx, j + q - d.ty, H, W);
  float4 v[3];                      // only the live pixels' sources are read (per aligned 16-byte quad)
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) v[ch] = da_gather4(s0 + ch * hw, i + dy, j + dx, H, W, live);
  float o[3][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float x[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) x[ch] = live[q] ? da_comp(v[ch], q) : 0.f;
    if (pol & GANLAB_DIFFAUG_COLOR) {
      const float mc = (x[0] + x[1] + x[2]) / 3.f;
      const float base = d.B * mc + shift;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch][q] = (FWD && !live[q]) ? 0.f : d.A * x[ch] + base;
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch][q] = x[ch];
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    *reinterpret_cast<float4*>(d0 + ch * hw) = float4{o[ch][0], o[ch][1], o[ch][2], o[ch][3]};
}

// One thread per sample: 2 Philox counters (8 words) at offset + 2n, offset + 2n + 1; u = (w >> 8) 2^-24.
__global__ __launch_bounds__(256) void diffaug_params_kernel(float* __restrict__ out, int N, int H, int W, uint64_t seed,
                                                             uint64_t offset, const uint64_t* __restrict__ base) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  if (base != nullptr) offset += *base;
  uint32_t w[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint64_t ctr = offset + 2 * (uint64_t)n + h;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int q = 0; q < 4; ++q) w[4 * h + q] = c[q];
  }
  const float two24 = 1.f / 16777216.f;
  // integer in [lo, lo + count): lo + floor(u * count), exactly (24-bit u times an int: integer arithmetic)
  auto pick = [](uint32_t word, int lo, int count) {
    return (float)(lo + (int)(((uint64_t)(word >> 8) * (uint64_t)count) >> 24));
  };
  const uint32_t u2 = (w[2] >> 8) + (1u << 23);           // 0.5 + u in units of 2^-24, in [2^23, 3 * 2^23)
  const int sh = da_shift(H), sw = da_shift(W), ch = da_cut(H), cw = da_cut(W);
  float* p = out + 8 * (long long)n;
  p[0] = (float)(w[0] >> 8) * two24 - 0.5f;                // brightness in [-0.5, 0.5)
  p[1] = (float)(w[1] >> 8) * two24 * 2.f;                 // saturation in [0, 2)
  p[2] = (float)(u2 >= (1u << 24) ? (u2 & ~1u) : u2) * two24;   // contrast in [0.5, 1.5): 0.5 + u rounded down to fp32
  p[3] = pick(w[3], -sh, 2 * sh + 1);
  p[4] = pick(w[4], -sw, 2 * sw + 1);
  p[5] = pick(w[5], 0, H + 1 - ch % 2);
  p[6] = pick(w[6], 0, W + 1 - cw % 2);
  p[7] = 0.f;
}

int da_check(int N, int H, int W, int pol) {
  if (N <= 0 || H <= 0 || W <= 0 || (W & 3) || N > 65535) return GANLAB_EINVAL;
  if (pol & ~(GANLAB_DIFFAUG_COLOR | GANLAB_DIFFAUG_TRANSLATION | GANLAB_DIFFAUG_CUTOUT)) return GANLAB_EINVAL;
  return GANLAB_OK;
}

template <bool FWD>
int da_run(const float* in, const float* params, float* out, int N, int H, int W, int pol, void* ws, size_t ws_bytes,
           void* stream) {
  if (!in || !params || !out || da_check(N, H, W, pol) != GANLAB_OK) return GANLAB_EINVAL;
  const int chunks = da_chunks(H, W);
  const bool color = (pol & GANLAB_DIFFAUG_COLOR) != 0;
  if (color && (!ws || ws_bytes < (size_t)N * chunks * sizeof(double))) return GANLAB_EWORKSPACE;
  hipStream_t st = gl_stream(stream);
  double* part = reinterpret_cast<double*>(ws);
  if (color) {
    if (FWD)
      GL_LAUNCH(diffaug_sum_kernel<false>, dim3(chunks, N), dim3(256), 0, st, in, params, part, H, W, pol);
    else
      GL_LAUNCH(diffaug_sum_kernel<true>, dim3(chunks, N), dim3(256), 0, st, in, params, part, H, W, pol);
  }
  const long long items = (long long)H * (W / 4);
  GL_LAUNCH(diffaug_apply_kernel<FWD>, dim3((unsigned)((items + 255) / 256), N), dim3(256), 0, st, in, params,
            (const double*)part, out, H, W, chunks, pol);
  return GL_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

int ganlab_diffaug_params_f32(float* out, int N, int H, int W, uint64_t seed, uint64_t offset, void* stream) {
  if (!out || N <= 0 || H <= 0 || W <= 0) return GANLAB_EINVAL;
  GL_LAUNCH(diffaug_params_kernel, dim3((N + 255) / 256), dim3(256), 0, gl_stream(stream), out, N, H, W, seed, offset,
            (const uint64_t*)nullptr);
  return GL_CHECK_LAUNCH();
}

int ganlab_diffaug_params_dev_f32(float* out, int N, int H, int W, uint64_t seed, const void* base, uint64_t delta,
                                  void* stream) {
  if (!out || N <= 0 || H <= 0 || W <= 0 || !base) return GANLAB_EINVAL;
  GL_LAUNCH(diffaug_params_kernel, dim3((N + 255) / 256), dim3(256), 0, gl_stream(stream), out, N, H, W, seed, delta,
            reinterpret_cast<const uint64_t*>(base));
  return GL_CHECK_LAUNCH();
}

size_t ganlab_diffaug_fwd_workspace(int N, int H, int W, int policy) {
  if (da_check(N, H, W, policy) != GANLAB_OK || !(policy & GANLAB_DIFFAUG_COLOR)) return 0;
  return (size_t)N * da_chunks(H, W) * sizeof(double);
}

size_t ganlab_diffaug_bwd_workspace(int N, int H, int W, int policy) { return ganlab_diffaug_fwd_workspace(N, H, W, policy); }

int ganlab_diffaug_fwd_f32(const float* x, const float* params, float* y, int N, int H, int W, int policy, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return da_run<true>(x, params, y, N, H, W, policy, workspace, workspace_bytes, stream);
}

int ganlab_diffaug_bwd_f32(const float* gy, const float* params, float* gx, int N, int H, int W, int policy,
                           void* workspace, size_t workspace_bytes, void* stream) {
  return da_run<false>(gy, params, gx, N, H, W, policy, workspace, workspace_bytes, stream);
}

}  // extern "C"
