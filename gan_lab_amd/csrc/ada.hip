// Adaptive discriminator augmentation (Karras et al. 2020, "Training Generative Adversarial Networks with Limited Data"):
// a per-sample affine bilinear warp with zero fill followed by a 3x4 color matrix, its adjoint, the parameter draw and
// the controller of the augmentation probability p.  DESIGN.md "ADA" has the math; in short, for the (N, 32) row
//   [0, 6)  M  (2x3): output pixel -> source position, centred pixel units
//   [6, 10) G  (2x2): the inverse of M[:, :2] (adjoint footprint; stored so that no thread inverts a matrix)
//   [10,22) C  (3x4): color matrix, linear part and offset column
//   [22,32) gates, then the raw geometric draws (tests and debugging; no kernel reads them)
// and u = j - (W-1)/2, v = i - (H-1)/2:
//   forward   sj = M00 u + M01 v + M02 + (W-1)/2, si = M10 u + M11 v + M12 + (H-1)/2
//             y[:, i, j] = C[:, :3] bilinear(x, si, sj) + C[:, 3]         (a tap outside the image counts as zero)
//   adjoint   gx[:, q] = C[:, :3]^T sum over the output pixels p whose source lies within one pixel of q of w(p, q) g[:, p]
// The adjoint is a gather: the candidates p of q lie inside the parallelogram G (q - t + (-1, 1)^2); the kernel walks its
// integer bounding box (clipped to the image, whatever its size), recomputes every candidate's source position and weight
// with the forward's own code, and sums in row-major order.  No float atomics; a sample's result depends on its own row
// only.  Source positions are computed in fp64 from the fp32 rows: they cost nothing next to the memory traffic, flips,
// quarter turns and integer shifts come out as exact copies at any size, and forward and adjoint cannot disagree on a tap.
#include "common.h"

namespace {

constexpr int kRow = GANLAB_ADA_ROW;      // floats per parameter row
constexpr int kTileQuads = 8, kTileRows = 32;      // workgroup: 8 threads of 4 pixels x 32 rows

struct AdaGeom {
  double m00, m01, m02, m10, m11, m12;
  double cx, cy;                          // (W - 1) / 2, (H - 1) / 2
};

__device__ __forceinline__ AdaGeom ada_geom(const float* __restrict__ p, int H, int W) {
  AdaGeom g;
  g.cx = 0.5 * (W - 1);
  g.cy = 0.5 * (H - 1);
  g.m00 = p[0]; g.m01 = p[1]; g.m02 = p[2];
  g.m10 = p[3]; g.m11 = p[4]; g.m12 = p[5];
  return g;
}

// source position of output pixel (i, j): the one definition the forward and the adjoint share
__device__ __forceinline__ void ada_src(const AdaGeom& g, int i, int j, double& si, double& sj) {
  const double u = (double)j - g.cx, v = (double)i - g.cy;
  sj = fma(g.m00, u, fma(g.m01, v, g.m02)) + g.cx;
  si = fma(g.m10, u, fma(g.m11, v, g.m12)) + g.cy;
}

// The 2 x 2 taps around (si, sj): top-left tap (i0, j0) and the weights of rows i0, i0 + 1 / columns j0, j0 + 1.  Returns false
// when no tap can be inside the image (also for a non-finite position).
__device__ __forceinline__ bool ada_taps(double si, double sj, int H, int W, int& i0, int& j0, float (&wy)[2], float (&wx)[2]) {
  if (!(si > -1.0 && si < (double)H && sj > -1.0 && sj < (double)W)) return false;
  const double fi = floor(si), fj = floor(sj);
  i0 = (int)fi;
  j0 = (int)fj;
  const float fy = (float)(si - fi), fx = (float)(sj - fj);
  wy[0] = 1.f - fy; wy[1] = fy;
  wx[0] = 1.f - fx; wx[1] = fx;
  return true;
}

// One thread = 4 consecutive output pixels of one row, all 3 channels.  A workgroup is 8 x 32 threads = a 32 x 32 pixel tile, so
// a wave covers 32 pixels (one 128-byte line per channel) x 8 rows: under a rotation its gather touches the lines of a compact
// 32 x 8 patch of the source instead of those along a 256-pixel segment.  blockIdx.z = sample.
__global__ __launch_bounds__(256) void ada_fwd_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                      float* __restrict__ y, int H, int W) {
  const int n = blockIdx.z;
  const int i = blockIdx.y * kTileRows + threadIdx.y, j = (blockIdx.x * kTileQuads + threadIdx.x) * 4;
  if (i >= H || j >= W) return;
  const long long hw = (long long)H * W;
  const float* p = params + (long long)kRow * n;
  const AdaGeom g = ada_geom(p, H, W);
  float C[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) C[k] = p[10 + k];
  const float* xs = x + (long long)n * 3 * hw;
  float o[3][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double si, sj;
    ada_src(g, i, j + q, si, sj);
    float v[3] = {0.f, 0.f, 0.f};
    int i0, j0;
    float wy[2], wx[2];
    if (ada_taps(si, sj, H, W, i0, j0, wy, wx)) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int r = i0 + a, c = j0 + b;
          const float w = wy[a] * wx[b];
          if (w != 0.f && r >= 0 && r < H && c >= 0 && c < W) {     // a zero weight reads nothing (blits: one tap)
            const float* s = xs + (long long)r * W + c;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = fmaf(w, s[ch * hw], v[ch]);
          }
        }
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      o[ch][q] = fmaf(C[4 * ch], v[0], fmaf(C[4 * ch + 1], v[1], fmaf(C[4 * ch + 2], v[2], C[4 * ch + 3])));
  }
  float* d0 = y + (long long)n * 3 * hw + (long long)i * W + j;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    *reinterpret_cast<float4*>(d0 + ch * hw) = float4{o[ch][0], o[ch][1], o[ch][2], o[ch][3]};
}

// integer range [lo, hi] of the centred interval c +- e mapped to indices (+ off), clipped to [0, n - 1] (empty: lo > hi); a NaN
// bound selects the whole axis (fmax / fmin return their other argument), and every value is in int range before it is converted
__device__ __forceinline__ void ada_range(double c, double e, double off, int n, int& lo, int& hi) {
  lo = (int)fmin(fmax(0.0, ceil(c - e + off)), (double)n);
  hi = (int)fmax(fmin((double)(n - 1), floor(c + e + off)), -1.0);
}

// One thread = 4 consecutive input pixels of one row, all 3 channels; the forward's 32 x 32 pixel tiles.  blockIdx.z = sample.
__global__ __launch_bounds__(256) void ada_adj_kernel(const float* __restrict__ gy, const float* __restrict__ params,
                                                      float* __restrict__ gx, int H, int W) {
  const int n = blockIdx.z;
  const int qi = blockIdx.y * kTileRows + threadIdx.y, qj0 = (blockIdx.x * kTileQuads + threadIdx.x) * 4;
  if (qi >= H || qj0 >= W) return;
  const long long hw = (long long)H * W;
  const float* p = params + (long long)kRow * n;
  const AdaGeom g = ada_geom(p, H, W);
  const double g00 = p[6], g01 = p[7], g10 = p[8], g11 = p[9];
  float C[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) C[k] = p[10 + k];
  // half extents of G (-1, 1)^2, widened a little: G is the fp32-rounded inverse, and a candidate on the very edge of the
  // footprint has a vanishing weight but must not depend on that rounding
  const double ex = (fabs(g00) + fabs(g01)) * 1.001 + 0.01, ey = (fabs(g10) + fabs(g11)) * 1.001 + 0.01;
  const float* gs = gy + (long long)n * 3 * hw;
  float o[3][4];
  for (int q = 0; q < 4; ++q) {
    const int qj = qj0 + q;
    // centre of the footprint: the output position whose source is q
    const double du = ((double)qj - g.cx) - g.m02, dv = ((double)qi - g.cy) - g.m12;
    const double pu = g00 * du + g01 * dv, pv = g10 * du + g11 * dv;
    int jlo, jhi, ilo, ihi;
    ada_range(pu, ex, g.cx, W, jlo, jhi);
    ada_range(pv, ey, g.cy, H, ilo, ihi);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int i = ilo; i <= ihi; ++i) {
      for (int j = jlo; j <= jhi; ++j) {
        double si, sj;
        ada_src(g, i, j, si, sj);
        int i0, j0;
        float wy[2], wx[2];
        if (!ada_taps(si, sj, H, W, i0, j0, wy, wx)) continue;
        const int a = qi - i0, b = qj - j0;
        if (a < 0 || a > 1 || b < 0 || b > 1) continue;
        const float w = (a ? wy[1] : wy[0]) * (b ? wx[1] : wx[0]);
        if (w == 0.f) continue;
        const float* s = gs + (long long)i * W + j;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] = fmaf(w, s[ch * hw], acc[ch]);
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)       // C[:, :3]^T: the color map acts per pixel, so it commutes with the warp's transpose
      o[ch][q] = fmaf(C[ch], acc[0], fmaf(C[4 + ch], acc[1], C[8 + ch] * acc[2]));
  }
  float* d0 = gx + (long long)n * 3 * hw + (long long)qi * W + qj0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    *reinterpret_cast<float4*>(d0 + ch * hw) = float4{o[ch][0], o[ch][1], o[ch][2], o[ch][3]};
}

// ---- parameter rows ------------------------------------------------------------------------------------------------------
struct Mat3 { double a[3][3]; };

__device__ __forceinline__ void mat3_right(Mat3& m, double b00, double b01, double b02, double b10, double b11, double b12) {
  // m = m @ [[b00, b01, b02], [b10, b11, b12], [0, 0, 1]] (rows 0 and 1 of m are all that is kept)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double x = m.a[r][0], y = m.a[r][1], z = m.a[r][2];
    m.a[r][0] = x * b00 + y * b10;
    m.a[r][1] = x * b01 + y * b11;
    m.a[r][2] = x * b02 + y * b12 + z;
  }
}

__device__ __forceinline__ void mat2_left(double (&g)[4], double l00, double l01, double l10, double l11) {
  const double a = g[0], b = g[1], c = g[2], d = g[3];      // g = l @ g
  g[0] = l00 * a + l01 * c; g[1] = l00 * b + l01 * d;
  g[2] = l10 * a + l11 * c; g[3] = l10 * b + l11 * d;
}

// c = t @ c for a 3x3 linear map t and the 3x4 matrix c
__device__ __forceinline__ void col_left(double (&c)[12], const double (&t)[9]) {
  double o[12];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) o[4 * r + k] = t[3 * r] * c[k] + t[3 * r + 1] * c[4 + k] + t[3 * r + 2] * c[8 + k];
#pragma unroll
  for (int k = 0; k < 12; ++k) c[k] = o[k];
}

// One thread per sample: GANLAB_ADA_COUNTERS Philox counters (32 words) at offset + 8n + h.  Word k of the row is word k % 4 of
// counter k / 4; u(k) = (word k >> 8) 2^-24.  The mapping (normative, DESIGN.md "ADA"):
//   gates     words 0..12: x-flip, quarter turn, integer shift, isotropic scale, pre-rotation, anisotropic scale,
//             post-rotation, fractional shift, brightness, contrast, luma flip, hue, saturation.  A gate fires when its
//             group is in the policy and u < p (the two rotations: u < 1 - sqrt(1 - p)), compared in fp64.
//   integers  13: k = floor(4 u); 14: tx = -sw + floor((2 sw + 1) u); 15: ty likewise with sh; sh = (H + 4) / 8
//   normals   Box-Muller in fp64 on ((word a >> 8) + 1) 2^-24 and u(a + 1): (16, 17) -> (isotropic z, anisotropic z),
//             (20, 21) -> (shift zx, zy), (22, 23) -> (brightness z, -), (24, 25) -> (contrast z, saturation z);
//             the geometric ones clamped to +-3
//   angles    18, 19, 26: (2 u - 1) pi for the pre-rotation, the post-rotation and the hue
// Every raw value is rounded to fp32 before M, G and C are composed from it in fp64.
__global__ __launch_bounds__(256) void ada_params_kernel(float* __restrict__ out, int N, int H, int W,
                                                         const float* __restrict__ state, int policy, uint64_t seed,
                                                         uint64_t offset, const uint64_t* __restrict__ base) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  if (base != nullptr) offset += *base;
  uint32_t w[4 * GANLAB_ADA_COUNTERS];
#pragma unroll
  for (int h = 0; h < GANLAB_ADA_COUNTERS; ++h) {
    const uint64_t ctr = offset + (uint64_t)GANLAB_ADA_COUNTERS * (uint64_t)n + h;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int q = 0; q < 4; ++q) w[4 * h + q] = c[q];
  }
  const double two24 = 1.0 / 16777216.0, pi = 3.14159265358979323846;
  const double p = (double)state[0];
  const double prot = 1.0 - sqrt(1.0 - fmin(fmax(p, 0.0), 1.0));
  auto uni = [&](int k) { return (double)(w[k] >> 8) * two24; };
  auto gate = [&](int k, int group, double prob) { return (policy & group) != 0 && uni(k) < prob; };
  auto pick = [&](int k, int lo, int count) { return lo + (int)(((uint64_t)(w[k] >> 8) * (uint64_t)count) >> 24); };
  auto normal = [&](int k, double& z0, double& z1) {
    const double r = sqrt(-2.0 * log((double)((w[k] >> 8) + 1u) * two24)), a = 2.0 * pi * uni(k + 1);
    z0 = r * cos(a);
    z1 = r * sin(a);
  };
  auto clamp3 = [](double z) { return fmin(fmax(z, -3.0), 3.0); };
  const int B = GANLAB_ADA_BLIT, Gm = GANLAB_ADA_GEOM, Cc = GANLAB_ADA_COLOR;
  const bool g_flip = gate(0, B, p), g_turn = gate(1, B, p), g_shift = gate(2, B, p), g_iso = gate(3, Gm, p),
             g_pre = gate(4, Gm, prot), g_aniso = gate(5, Gm, p), g_post = gate(6, Gm, prot), g_frac = gate(7, Gm, p),
             g_bright = gate(8, Cc, p), g_contrast = gate(9, Cc, p), g_luma = gate(10, Cc, p), g_hue = gate(11, Cc, p),
             g_sat = gate(12, Cc, p);
  const int sh = (H + 4) / 8, sw = (W + 4) / 8;
  const int k = pick(13, 0, 4), tx = pick(14, -sw, 2 * sw + 1), ty = pick(15, -sh, 2 * sh + 1);
  double z_iso, z_aniso, z_fx, z_fy, z_bright, z_unused, z_contrast, z_sat;
  normal(16, z_iso, z_aniso);
  normal(20, z_fx, z_fy);
  normal(22, z_bright, z_unused);
  normal(24, z_contrast, z_sat);
  const float r_iso = (float)clamp3(z_iso), r_aniso = (float)clamp3(z_aniso), r_fx = (float)clamp3(z_fx),
              r_fy = (float)clamp3(z_fy), r_bright = (float)z_bright, r_contrast = (float)z_contrast, r_sat = (float)z_sat;
  const float r_pre = (float)((2.0 * uni(18) - 1.0) * pi), r_post = (float)((2.0 * uni(19) - 1.0) * pi),
              r_hue = (float)((2.0 * uni(26) - 1.0) * pi);

  // M = X^-1 Q^-1 T^-1 S^-1 Rpre^-1 A^-1 Rpost^-1 F^-1 (each factor: output -> source); G = F Rpost A Rpre S T Q X, linear parts
  Mat3 m = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
  double g[4] = {1, 0, 0, 1};
  if (g_flip) {
    mat3_right(m, -1, 0, 0, 0, 1, 0);
    mat2_left(g, -1, 0, 0, 1);
  }
  if (g_turn) {
    const double c = k == 0 ? 1 : k == 2 ? -1 : 0, s = k == 1 ? 1 : k == 3 ? -1 : 0;
    mat3_right(m, c, -s, 0, s, c, 0);
    mat2_left(g, c, s, -s, c);
  }
  if (g_shift) mat3_right(m, 1, 0, (double)tx, 0, 1, (double)ty);
  if (g_iso) {
    const double s = exp2(0.2 * (double)r_iso);
    mat3_right(m, 1.0 / s, 0, 0, 0, 1.0 / s, 0);
    mat2_left(g, s, 0, 0, s);
  }
  if (g_pre) {
    const double c = cos((double)r_pre), s = sin((double)r_pre);
    mat3_right(m, c, -s, 0, s, c, 0);
    mat2_left(g, c, s, -s, c);
  }
  if (g_aniso) {
    const double s = exp2(0.2 * (double)r_aniso);
    mat3_right(m, 1.0 / s, 0, 0, 0, s, 0);
    mat2_left(g, s, 0, 0, 1.0 / s);
  }
  if (g_post) {
    const double c = cos((double)r_post), s = sin((double)r_post);
    mat3_right(m, c, -s, 0, s, c, 0);
    mat2_left(g, c, s, -s, c);
  }
  if (g_frac) mat3_right(m, 1, 0, 0.125 * W * (double)r_fx, 0, 1, 0.125 * H * (double)r_fy);

  // C: brightness, contrast, luma flip, hue rotation, saturation, each applied after the ones before it
  double c[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  if (g_bright) {
    const double b = 0.2 * (double)r_bright;
    c[3] += b; c[7] += b; c[11] += b;
  }
  if (g_contrast) {
    const double s = exp2(0.5 * (double)r_contrast);
#pragma unroll
    for (int q = 0; q < 12; ++q) c[q] *= s;
  }
  const double third = 1.0 / 3.0;
  if (g_luma) {                  // I - 2 v v^T, v = (1, 1, 1) / sqrt(3)
    const double d = 1.0 - 2.0 * third, e = -2.0 * third;
    const double t[9] = {d, e, e, e, d, e, e, e, d};
    col_left(c, t);
  }
  if (g_hue) {                   // Rodrigues about v: cos I + sin [v]x + (1 - cos) v v^T
    const double cs = cos((double)r_hue), sn = sin((double)r_hue) / sqrt(3.0), d = cs + (1.0 - cs) * third,
                 e = (1.0 - cs) * third;
    const double t[9] = {d, e - sn, e + sn, e + sn, d, e - sn, e - sn, e + sn, d};
    col_left(c, t);
  }
  if (g_sat) {                   // v v^T + s (I - v v^T)
    const double s = exp2((double)r_sat), d = third + s * (1.0 - third), e = third - s * third;
    const double t[9] = {d, e, e, e, d, e, e, e, d};
    col_left(c, t);
  }

  float* row = out + (long long)kRow * n;
  row[0] = (float)m.a[0][0]; row[1] = (float)m.a[0][1]; row[2] = (float)m.a[0][2];
  row[3] = (float)m.a[1][0]; row[4] = (float)m.a[1][1]; row[5] = (float)m.a[1][2];
#pragma unroll
  for (int q = 0; q < 4; ++q) row[6 + q] = (float)g[q];
#pragma unroll
  for (int q = 0; q < 12; ++q) row[10 + q] = (float)c[q];
  const unsigned bits = (unsigned)g_flip | (unsigned)g_turn << 1 | (unsigned)g_shift << 2 | (unsigned)g_iso << 3 |
                        (unsigned)g_pre << 4 | (unsigned)g_aniso << 5 | (unsigned)g_post << 6 | (unsigned)g_frac << 7 |
                        (unsigned)g_bright << 8 | (unsigned)g_contrast << 9 | (unsigned)g_luma << 10 |
                        (unsigned)g_hue << 11 | (unsigned)g_sat << 12;
  row[22] = (float)bits;
  row[23] = (float)k; row[24] = (float)tx; row[25] = (float)ty;
  row[26] = r_iso; row[27] = r_pre; row[28] = r_aniso; row[29] = r_post; row[30] = r_fx; row[31] = r_fy;
  (void)r_bright; (void)r_contrast; (void)r_sat; (void)r_hue; (void)z_unused;
}

// ---- controller ------------------------------------------------------------------------------------------------------------
// state = (p, acc_sum, acc_n, calls), fp32 (the sums are integers far below 2^24: exact).  One workgroup: adds
// sum(sign(logits)) and N, counts the call, and when interval > 0 and calls >= interval moves p one step towards the target
// and clears the rest.  Signs are summed as integers, so the reduction order cannot matter.
__global__ __launch_bounds__(256) void ada_update_kernel(float* __restrict__ state, const float* __restrict__ logits, int N,
                                                         int interval, float step_size, float target) {
  __shared__ int red[4];
  int s = 0;
  for (int k = threadIdx.x; k < N; k += 256) {
    const float v = logits[k];
    s += (v > 0.f) - (v < 0.f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  float p = state[0];
  float acc_sum = state[1] + (float)(red[0] + red[1] + red[2] + red[3]);
  float acc_n = state[2] + (float)N;
  float calls = state[3] + 1.f;
  if (interval > 0 && calls >= (float)interval) {
    if (acc_n > 0.f) {
      const float d = acc_sum / acc_n - target;
      const float sgn = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
      p = fminf(fmaxf(p + sgn * step_size, 0.f), 1.f);
    }
    acc_sum = acc_n = calls = 0.f;
  }
  state[0] = p;
  state[1] = acc_sum;
  state[2] = acc_n;
  state[3] = calls;
}

int ada_check(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || (W & 3) || N > 65535) return GANLAB_EINVAL;
  return GANLAB_OK;
}

dim3 ada_grid(int N, int H, int W) {
  return dim3((W / 4 + kTileQuads - 1) / kTileQuads, (H + kTileRows - 1) / kTileRows, N);
}

int ada_params_run(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed, uint64_t offset,
                   const uint64_t* base, void* stream) {
  if (!out || !state || N <= 0 || H <= 0 || W <= 0) return GANLAB_EINVAL;
  if (policy & ~(GANLAB_ADA_BLIT | GANLAB_ADA_GEOM | GANLAB_ADA_COLOR)) return GANLAB_EINVAL;
  GL_LAUNCH(ada_params_kernel, dim3((N + 255) / 256), dim3(256), 0, gl_stream(stream), out, N, H, W, state, policy, seed,
            offset, base);
  return GL_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

int ganlab_ada_params_f32(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed, uint64_t offset,
                          void* stream) {
  return ada_params_run(out, N, H, W, state, policy, seed, offset, nullptr, stream);
}

int ganlab_ada_params_dev_f32(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed,
                              const void* base, uint64_t delta, void* stream) {
  if (!base) return GANLAB_EINVAL;
  return ada_params_run(out, N, H, W, state, policy, seed, delta, reinterpret_cast<const uint64_t*>(base), stream);
}

int ganlab_ada_fwd_f32(const float* x, const float* params, float* y, int N, int H, int W, void* stream) {
  if (!x || !params || !y || ada_check(N, H, W) != GANLAB_OK) return GANLAB_EINVAL;
  GL_LAUNCH(ada_fwd_kernel, ada_grid(N, H, W), dim3(kTileQuads, kTileRows), 0, gl_stream(stream), x, params, y, H, W);
  return GL_CHECK_LAUNCH();
}

int ganlab_ada_bwd_f32(const float* gy, const float* params, float* gx, int N, int H, int W, void* stream) {
  if (!gy || !params || !gx || ada_check(N, H, W) != GANLAB_OK) return GANLAB_EINVAL;
  GL_LAUNCH(ada_adj_kernel, ada_grid(N, H, W), dim3(kTileQuads, kTileRows), 0, gl_stream(stream), gy, params, gx, H, W);
  return GL_CHECK_LAUNCH();
}

int ganlab_ada_update_f32(float* state, const float* logits, int N, int interval, float step_size, float target,
                          void* stream) {
  if (!state || N < 0 || (N > 0 && !logits)) return GANLAB_EINVAL;
  GL_LAUNCH(ada_update_kernel, dim3(1), dim3(256), 0, gl_stream(stream), state, logits, N, interval, step_size, target);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
