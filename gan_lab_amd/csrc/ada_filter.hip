// ADA's image-space groups (Karras et al. 2020, appendix B): a per-sample separable 43-tap FIR built from four band gains, additive
// Gaussian noise and a cutout rectangle, applied after the warp and the color matrix of csrc/ada.hip:
//   y = cutout(noise(filter(color(warp(x)))))
// DESIGN.md 4.6 has the normative text; in short, for the (N, 16) row `ext`
//   [0, 4)   g      band gains          [4]      sigma          [5, 9)   j0, j1, i0, i1: columns [j0, j1) x rows [i0, i1) become 0
//   [9]      gates  (bit b = band b, bit 4 = noise, bit 5 = cutout)     [10, 14) the four band z      [14, 16) cx, cy
// and the (4, 43) bank F:  h[k] = fp32(sum_b g_b F[b][k]) (summed in fp64),
//   along one axis   y[p] = sum_k h[k] x[r(p + k - 21)],   r(i): m = i mod 2(W - 1), r = m < W ? m : 2(W - 1) - m
// (whole-sample reflection of any depth), rows first, then columns, the same h for all three channels.  The gate mask decides
// what acts: a row whose band gates are all closed is not filtered (never multiplied by the almost-impulse), sigma counts only
// with bit 4 and the rectangle only with bit 5, so a row with an empty mask is an exact copy; a row with sigma == 0 reads no noise.
// The adjoint is F^T (mask o g): along one axis gx[q] = sum over the pre-images m of q under r, -21 <= m <= W + 20, in ascending
// order, of c(m) = sum_k h[k] g0[m - k + 21] (g0 = g extended by zeros) - a gather in a fixed order, no float atomics.
// One workgroup = one 32 x 32 tile of one (n, c) plane: it stages the tile and its 21-pixel halo in LDS (reflection resolved at
// staging; the adjoint stages the cotangents its pre-images can reach, at most 74 x 74 as well), runs the first pass into LDS and
// the second out of it.
#include "common.h"

namespace {

constexpr int kExt = GANLAB_ADA_EXT_ROW;
constexpr int kTaps = GANLAB_ADA_FILTER_TAPS, kHalf = kTaps / 2;
constexpr int kT = 32;                       // tile edge
constexpr int kS = kT + 2 * kHalf;           // staged edge: 74
constexpr int kSP = kS + 1;                  // odd LDS row stride: lanes that walk a column hit distinct banks
constexpr int kTP = kT + 1;
// row pass: a staged row is 3 segments of 11 outputs, 33 with one spare that lands in the padding column of s_mid and reads the
// padding column of s_in (never used), so that the 74 x 3 items fit the 256 threads in one trip
constexpr int kSegs = 3, kSegW = 11;
static_assert(kSegs * kSegW <= kTP && (kSegs - 1) * kSegW + kSegW - 1 + kTaps - 1 < kSP,
              "row-pass segments stay inside the padded rows");
constexpr int kMid = kS * kTP > kT * kSP ? kS * kTP : kT * kSP;

__constant__ double kBank[4][kTaps] = {
#include "ada_filter_bank.h"
};
const double kBankHost[4][kTaps] = {
#include "ada_filter_bank.h"
};

__device__ __forceinline__ int ada_reflect(int i, int n) {      // n >= 2
  const int per = 2 * (n - 1);
  int m = i % per;
  if (m < 0) m += per;
  return m < n ? m : per - m;
}

// the taps of one sample into LDS (threads 0..42), then into every thread's registers
__device__ __forceinline__ void ada_taps(const float* __restrict__ e, float* s_h, float (&h)[kTaps]) {
  if (threadIdx.x < kTaps) {
    const int k = threadIdx.x;
    const double v = (double)e[0] * kBank[0][k] + (double)e[1] * kBank[1][k] + (double)e[2] * kBank[2][k] +
                     (double)e[3] * kBank[3][k];
    s_h[k] = (float)v;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kTaps; ++k) h[k] = s_h[k];
}

struct AdaExtRow {
  bool filt;
  float sigma;
  int j0, j1, i0, i1;
};

__device__ __forceinline__ AdaExtRow ada_ext_row(const float* __restrict__ e) {
  AdaExtRow r;
  const unsigned gates = (unsigned)e[9];
  r.filt = (gates & 15u) != 0u;
  r.sigma = (gates & 16u) ? e[4] : 0.f;
  r.j0 = r.j1 = r.i0 = r.i1 = 0;
  if (gates & 32u) {
    r.j0 = (int)e[5]; r.j1 = (int)e[6]; r.i0 = (int)e[7]; r.i1 = (int)e[8];
  }
  return r;
}

// grid (ceil(W / 32), ceil(H / 32), 3 N), 256 threads.  Row pass: a thread takes 11 consecutive outputs of one staged row from a
// 53-wide window (lanes walk down the rows: conflict-free at the odd stride).  Column pass and store: thread (col, rs) takes
// rows 4 rs .. 4 rs + 3 of column col, so a wave stores two 128-byte row segments at a time.
__global__ __launch_bounds__(256) void ada_ext_fwd_kernel(const float* __restrict__ x, const float* __restrict__ ext,
                                                          const float* __restrict__ noise, float* __restrict__ y, int H, int W) {
  __shared__ float s_in[kS * kSP];
  __shared__ float s_mid[kMid];
  __shared__ float s_h[kTaps + 1];
  const int plane = blockIdx.z, n = plane / 3;
  const int i0 = blockIdx.y * kT, j0 = blockIdx.x * kT;
  const AdaExtRow e = ada_ext_row(ext + (long long)kExt * n);
  const long long base = (long long)plane * H * W;
  const float* xs = x + base;
  const int tid = threadIdx.x, col = tid & 31, rs = tid >> 5;
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  if (e.filt) {
    for (int idx = tid; idx < kS * kS; idx += 256) {
      const int r = idx / kS, c = idx - r * kS;
      s_in[r * kSP + c] = xs[(long long)ada_reflect(i0 + r - kHalf, H) * W + ada_reflect(j0 + c - kHalf, W)];
    }
    float h[kTaps];
    ada_taps(ext + (long long)kExt * n, s_h, h);          // its barrier also covers the staging
    if (tid < kS * kSegs) {            // 222 items: one trip
      const int seg = tid / kS, r = tid - seg * kS;
      const float* p = s_in + r * kSP + seg * kSegW;
      float acc[kSegW];
#pragma unroll
      for (int q = 0; q < kSegW; ++q) acc[q] = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps + kSegW - 1; ++k) {
        const float v = p[k];
#pragma unroll
        for (int q = 0; q < kSegW; ++q)
          if (k - q >= 0 && k - q < kTaps) acc[q] = fmaf(h[k - q], v, acc[q]);
      }
#pragma unroll
      for (int q = 0; q < kSegW; ++q) s_mid[r * kTP + seg * kSegW + q] = acc[q];
    }
    __syncthreads();
    const float* p = s_mid + rs * 4 * kTP + col;
#pragma unroll
    for (int k = 0; k < kTaps + 3; ++k) {
      const float v = p[k * kTP];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k - q >= 0 && k - q < kTaps) out[q] = fmaf(h[k - q], v, out[q]);
    }
  }
  const int j = j0 + col;
  if (j >= W) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = i0 + rs * 4 + q;
    if (i >= H) break;
    const long long at = (long long)i * W + j;
    float v = e.filt ? out[q] : xs[at];
    if (noise != nullptr && e.sigma != 0.f) v = fmaf(e.sigma, noise[base + at], v);
    if (j >= e.j0 && j < e.j1 && i >= e.i0 && i < e.i1) v = 0.f;
    y[base + at] = v;
  }
}

// The cotangents that the pre-images of outputs [q0, q1) can reach, clipped to the axis: [plo, phi].  With 32-wide tiles the range
// is at most 74 long (a tile next to a border folds that border's halo back; a tile next to both has n <= 53).
__device__ __forceinline__ void ada_adj_range(int q0, int q1, int n, int& plo, int& phi) {
  const int mlo = q0 <= kHalf ? -kHalf : q0, mhi = q1 - 1 >= n - 1 - kHalf ? n + kHalf - 1 : q1 - 1;
  plo = max(0, mlo - kHalf);
  phi = min(min(n - 1, mhi + kHalf), plo + kS - 1);
}

// gx[q] along one axis from the staged cotangents s[(p - plo) * stride], plo <= p <= phi (zero elsewhere): the pre-images
// m = t per + q and t per + (per - q), ascending, each one's 43 taps summed on their own and then added
__device__ __forceinline__ float ada_adj_gather(const float* s, int stride, int q, int n, int plo, int phi,
                                                const float (&h)[kTaps]) {
  const int per = 2 * (n - 1);
  const int tmin = -((kHalf + per - 1) / per) - 1, tmax = (n + kHalf - 1) / per + 1;
  const bool single = q == 0 || q == n - 1;
  float total = 0.f;
  for (int t = tmin; t <= tmax; ++t) {
    for (int side = 0; side < 2; ++side) {
      if (side == 1 && single) break;
      const int m = t * per + (side ? per - q : q);
      if (m < -kHalf || m > n + kHalf - 1) continue;
      float c = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const int p = m - k + kHalf;
        const bool ok = p >= plo && p <= phi;
        const float v = s[(ok ? p - plo : 0) * stride];
        c = fmaf(h[k], ok ? v : 0.f, c);
      }
      total += c;
    }
  }
  return total;
}

// gx = F^T (mask o gy): the forward's grid.  Columns' adjoint first (into LDS, for the tile's rows and every staged column), then
// the rows' adjoint out of it.
__global__ __launch_bounds__(256) void ada_ext_adj_kernel(const float* __restrict__ gy, const float* __restrict__ ext,
                                                          float* __restrict__ gx, int H, int W) {
  __shared__ float s_in[kS * kSP];
  __shared__ float s_mid[kMid];
  __shared__ float s_h[kTaps + 1];
  const int plane = blockIdx.z, n = plane / 3;
  const int i0 = blockIdx.y * kT, j0 = blockIdx.x * kT;
  const int th = min(kT, H - i0), tw = min(kT, W - j0);
  const AdaExtRow e = ada_ext_row(ext + (long long)kExt * n);
  const long long base = (long long)plane * H * W;
  const float* gs = gy + base;
  const int tid = threadIdx.x;
  auto masked = [&](int i, int j) {
    return (j >= e.j0 && j < e.j1 && i >= e.i0 && i < e.i1) ? 0.f : gs[(long long)i * W + j];
  };
  if (!e.filt) {
    for (int idx = tid; idx < th * kT; idx += 256) {
      const int r = idx >> 5, c = idx & 31;
      if (c < tw) gx[base + (long long)(i0 + r) * W + j0 + c] = masked(i0 + r, j0 + c);
    }
    return;
  }
  int pilo, pihi, pjlo, pjhi;
  ada_adj_range(i0, i0 + th, H, pilo, pihi);
  ada_adj_range(j0, j0 + tw, W, pjlo, pjhi);
  const int ph = pihi - pilo + 1, pw = pjhi - pjlo + 1;          // both in [1, 74]
  for (int idx = tid; idx < ph * pw; idx += 256) {
    const int r = idx / pw, c = idx - r * pw;
    s_in[r * kSP + c] = masked(pilo + r, pjlo + c);
  }
  float h[kTaps];
  ada_taps(ext + (long long)kExt * n, s_h, h);            // its barrier also covers the staging
  for (int idx = tid; idx < th * pw; idx += 256) {
    const int r = idx / pw, c = idx - r * pw;
    s_mid[r * kSP + c] = ada_adj_gather(s_in + c, kSP, i0 + r, H, pilo, pihi, h);
  }
  __syncthreads();
  for (int idx = tid; idx < th * kT; idx += 256) {
    const int r = idx >> 5, c = idx & 31;
    if (c < tw) gx[base + (long long)(i0 + r) * W + j0 + c] = ada_adj_gather(s_mid + r * kSP, 1, j0 + c, W, pjlo, pjhi, h);
  }
}

// ---- parameter rows ------------------------------------------------------------------------------------------------------
// One thread per sample: GANLAB_ADA_EXT_COUNTERS Philox counters (16 words) at offset + 4n + h, where offset is the position
// right after the batch's main block (csrc/ada.hip).  u(k) and the Box-Muller are those of ada_params_kernel.  The mapping
// (normative):
//   gates     words 0..3: the four bands (group filter), 4: noise, 5: cutout; a gate fires when its group is in the policy and
//             u < p, compared in fp64
//   centre    6, 7: cx = u, cy = u
//   normals   (8, 9) -> z of bands 0, 1; (10, 11) -> z of bands 2, 3; (12, 13) -> (noise z, -); every one clamped to +-3
//   14, 15    reserved
// Every raw value is rounded to fp32 before g, sigma and the rectangle are composed from it in fp64.
__global__ __launch_bounds__(256) void ada_ext_params_kernel(float* __restrict__ out, int N, int H, int W,
                                                             const float* __restrict__ state, int policy, uint64_t seed,
                                                             uint64_t offset, const uint64_t* __restrict__ base) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  if (base != nullptr) offset += *base;
  uint32_t w[4 * GANLAB_ADA_EXT_COUNTERS];
#pragma unroll
  for (int h = 0; h < GANLAB_ADA_EXT_COUNTERS; ++h) {
    const uint64_t ctr = offset + (uint64_t)GANLAB_ADA_EXT_COUNTERS * (uint64_t)n + h;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int q = 0; q < 4; ++q) w[4 * h + q] = c[q];
  }
  const double two24 = 1.0 / 16777216.0, pi = 3.14159265358979323846;
  const double p = (double)state[0];
  auto uni = [&](int k) { return (double)(w[k] >> 8) * two24; };
  auto gate = [&](int k, int group) { return (policy & group) != 0 && uni(k) < p; };
  auto normal = [&](int k, double& z0, double& z1) {
    const double r = sqrt(-2.0 * log((double)((w[k] >> 8) + 1u) * two24)), a = 2.0 * pi * uni(k + 1);
    z0 = r * cos(a);
    z1 = r * sin(a);
  };
  auto clamp3 = [](double z) { return fmin(fmax(z, -3.0), 3.0); };
  bool g_band[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) g_band[b] = gate(b, GANLAB_ADA_FILTER);
  const bool g_noise = gate(4, GANLAB_ADA_NOISE), g_cut = gate(5, GANLAB_ADA_CUTOUT);
  const float cx = (float)uni(6), cy = (float)uni(7);
  double z[4], z_noise, z_unused;
  normal(8, z[0], z[1]);
  normal(10, z[2], z[3]);
  normal(12, z_noise, z_unused);
  float r_z[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) r_z[b] = (float)clamp3(z[b]);
  const float r_noise = (float)clamp3(z_noise);

  // every gated band i scales its own gain by 2^z and the whole vector back to the expected power sum_b e_b t_b^2 = 1,
  // e = (10, 1, 1, 1) / 13; a closed band changes nothing, so with none open g is exactly (1, 1, 1, 1)
  double g[4] = {1, 1, 1, 1};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!g_band[i]) continue;
    double t[4] = {1, 1, 1, 1};
    t[i] = exp2((double)r_z[i]);
    const double s = sqrt((10.0 * t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3]) / 13.0);
#pragma unroll
    for (int b = 0; b < 4; ++b) g[b] *= t[b] / s;
  }
  const float sigma = g_noise ? (float)(0.1 * fabs((double)r_noise)) : 0.f;

  // cutout: index k of an axis of n pixels is inside iff |(k + 0.5) / n - c| < 0.25, in fp64; the inside set is an interval,
  // found from an estimate of its ends and settled with the predicate itself
  auto bounds = [](int n, double c, int& lo, int& hi) {
    auto inside = [&](int k) { return fabs(((double)k + 0.5) / (double)n - c) < 0.25; };
    lo = (int)fmin(fmax(floor((c - 0.25) * n - 0.5) + 1.0, 0.0), (double)n);
    while (lo > 0 && inside(lo - 1)) --lo;
    while (lo < n && !inside(lo)) ++lo;
    hi = (int)fmin(fmax(ceil((c + 0.25) * n - 0.5), (double)lo), (double)n);
    while (hi < n && inside(hi)) ++hi;
    while (hi > lo && !inside(hi - 1)) --hi;
  };
  int j0 = 0, j1 = 0, i0 = 0, i1 = 0;
  if (g_cut) {
    bounds(W, (double)cx, j0, j1);
    bounds(H, (double)cy, i0, i1);
  }

  float* row = out + (long long)kExt * n;
#pragma unroll
  for (int b = 0; b < 4; ++b) row[b] = (float)g[b];
  row[4] = sigma;
  row[5] = (float)j0; row[6] = (float)j1; row[7] = (float)i0; row[8] = (float)i1;
  const unsigned bits = (unsigned)g_band[0] | (unsigned)g_band[1] << 1 | (unsigned)g_band[2] << 2 | (unsigned)g_band[3] << 3 |
                        (unsigned)g_noise << 4 | (unsigned)g_cut << 5;
  row[9] = (float)bits;
#pragma unroll
  for (int b = 0; b < 4; ++b) row[10 + b] = r_z[b];
  row[14] = cx; row[15] = cy;
  (void)z_unused;
}

int ada_ext_check(int N, int H, int W) {
  if (N <= 0 || H < 2 || W < 4 || (W & 3) || 3LL * N > 65535) return GANLAB_EINVAL;
  return GANLAB_OK;
}

dim3 ada_ext_grid(int N, int H, int W) { return dim3((W + kT - 1) / kT, (H + kT - 1) / kT, 3 * N); }

int ada_ext_params_run(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed, uint64_t offset,
                       const uint64_t* base, void* stream) {
  if (!out || !state || N <= 0 || H <= 0 || W <= 0) return GANLAB_EINVAL;
  const int all = GANLAB_ADA_BLIT | GANLAB_ADA_GEOM | GANLAB_ADA_COLOR | GANLAB_ADA_FILTER | GANLAB_ADA_NOISE | GANLAB_ADA_CUTOUT;
  if (policy & ~all) return GANLAB_EINVAL;
  GL_LAUNCH(ada_ext_params_kernel, dim3((N + 255) / 256), dim3(256), 0, gl_stream(stream), out, N, H, W, state, policy, seed,
            offset, base);
  return GL_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

int ganlab_ada_filter_bank(double* out) {
  if (!out) return GANLAB_EINVAL;
  for (int b = 0; b < 4; ++b)
    for (int k = 0; k < kTaps; ++k) out[b * kTaps + k] = kBankHost[b][k];
  return GANLAB_OK;
}

int ganlab_ada_ext_params_f32(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed, uint64_t offset,
                              void* stream) {
  return ada_ext_params_run(out, N, H, W, state, policy, seed, offset, nullptr, stream);
}

int ganlab_ada_ext_params_dev_f32(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed,
                                  const void* base, uint64_t delta, void* stream) {
  if (!base) return GANLAB_EINVAL;
  return ada_ext_params_run(out, N, H, W, state, policy, seed, delta, reinterpret_cast<const uint64_t*>(base), stream);
}

int ganlab_ada_ext_fwd_f32(const float* x, const float* ext, const float* noise, float* y, int N, int H, int W, void* stream) {
  if (!x || !ext || !y || x == y || ada_ext_check(N, H, W) != GANLAB_OK) return GANLAB_EINVAL;
  GL_LAUNCH(ada_ext_fwd_kernel, ada_ext_grid(N, H, W), dim3(256), 0, gl_stream(stream), x, ext, noise, y, H, W);
  return GL_CHECK_LAUNCH();
}

int ganlab_ada_ext_bwd_f32(const float* gy, const float* ext, float* gx, int N, int H, int W, void* stream) {
  if (!gy || !ext || !gx || gy == gx || ada_ext_check(N, H, W) != GANLAB_OK) return GANLAB_EINVAL;
  GL_LAUNCH(ada_ext_adj_kernel, ada_ext_grid(N, H, W), dim3(256), 0, gl_stream(stream), gy, ext, gx, H, W);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
