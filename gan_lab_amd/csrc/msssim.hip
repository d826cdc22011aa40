// Multi-scale structural similarity (MS-SSIM; Wang, Simoncelli, Bovik 2003) between pairs of images: the sample-diversity metric
// of Karras et al. 2018 ("Progressive Growing of GANs", section 5), behind gan_lab_amd/msssim.py.  DESIGN.md 4.8 has the definition.
//   level    one workgroup = one 32 x 32 output tile of one (pair, channel) plane.  It stages the two input patches (tile + window
//            halo) in LDS, filters a, b, a a, b b, a b along x and then along y with the level's Gaussian window (valid mode), forms
//            cs and ssim per output pixel, and reduces the tile to two fp64 partials.  From the same LDS patches it writes the 2 x 2
//            mean of the rows and columns it owns: the next level of both images, so every level is read from memory once.
//   pair     one wave per pair: per level the partials in a fixed order -> (CS_i, SSIM_i) clamped at 0, and the weighted product
//   mean     the mean over pairs of the product and of the table's columns, summed in index order
// No atomics: every result is bitwise reproducible and does not depend on how the pairs were split over calls.
#include <cmath>

#include "common.h"

namespace {

constexpr int kTile = 32;                 // output tile side; even, so a tile owns whole 2 x 2 blocks
constexpr int kWin = GANLAB_MSSSIM_WINDOW;
constexpr int kLevels = GANLAB_MSSSIM_LEVELS;
constexpr int kHStride = kTile + 1;       // row stride of the x-filtered planes: the 4 rows a half-wave writes at a column stride
                                          // of 4 start on banks 0, 1, 2, 3

struct MsWindow { float g[kWin]; };       // a kernel argument: wave-uniform, read through the scalar cache

// Window side s of a level of side S, its output side, and its tiles per axis.
__host__ __device__ inline int ms_window(int S) { return S < kWin ? S : kWin; }
__host__ __device__ inline int ms_tiles(int S) { return (S - ms_window(S) + 1 + kTile - 1) / kTile; }

// cs and ssim of one pixel from its five filtered values.  Nothing here is contracted into an fma: with a == b the numerators and
// denominators are then the same bits, so identical images score exactly 1, and swapping a and b changes no bit.
__device__ __forceinline__ void ms_pixel(float ma, float mb, float aa, float bb, float ab, float c1, float c2, float& cs,
                                         float& ssim) {
#pragma clang fp contract(off)
  const float paa = ma * ma, pbb = mb * mb, pab = ma * mb;
  const float saa = aa - paa, sbb = bb - pbb, sab = ab - pab;
  const float v1 = 2.f * sab + c2, v2 = (saa + sbb) + c2;
  cs = v1 / v2;
  ssim = ((2.f * pab + c1) * v1) / (((paa + pbb) + c1) * v2);
}

template <int KS>
__global__ __launch_bounds__(256) void msssim_level_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           long long pair_stride, float* __restrict__ next_a,
                                                           float* __restrict__ next_b, long long next_stride,
                                                           double* __restrict__ part, MsWindow win, int S, int tiles, float c1,
                                                           float c2) {
  constexpr int PH = kTile + KS - 1;      // patch side: tile + halo
  constexpr int PS = PH | 1;              // patch row stride (43 for the full window: rows 0..3 x column stride 4 fall on distinct banks)
  __shared__ float pa[PH * PS], pb[PH * PS];
  __shared__ float h[5][PH * kHStride];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int per_plane = tiles * tiles;
  const long long plane = blockIdx.x / per_plane;              // pair * 3 + channel
  const int tile = (int)(blockIdx.x - plane * per_plane);
  const int ty = tile / tiles, tx = tile - ty * tiles;
  const long long pair = plane / 3;
  const int ch = (int)(plane - pair * 3);
  const int y0 = ty * kTile, x0 = tx * kTile;                  // origin of the tile: output pixel = top-left input pixel
  const int O = S - KS + 1;
  const long long in_off = pair * pair_stride + (long long)ch * S * S;

  // ---- stage both patches; outside the plane: 0 (those entries only reach outputs that are masked below)
  for (int e = tid; e < PH * PH; e += 256) {
    const int r = e / PH, q = e - r * PH;
    const int y = y0 + r, x = x0 + q;
    const bool in = y < S && x < S;
    const long long g = in_off + (long long)y * S + x;
    pa[r * PS + q] = in ? a[g] : 0.f;
    pb[r * PS + q] = in ? b[g] : 0.f;
  }
  __syncthreads();

  // ---- the next level: 2 x 2 means of the rows / columns [y0, min(y0 + 32, S)) this tile owns (S a power of two: the tiles'
  //      owned ranges cover the plane, and each lies inside its patch)
  if (next_a != nullptr) {
    const int S2 = S >> 1;
    const int own_h = (min(kTile, S - y0)) >> 1, own_w = (min(kTile, S - x0)) >> 1;
    const long long out_off = pair * next_stride + (long long)ch * S2 * S2 + (long long)(y0 >> 1) * S2 + (x0 >> 1);
    for (int e = tid; e < own_h * own_w; e += 256) {
      const int by = e / own_w, bx = e - by * own_w;
      const int i = 2 * by * PS + 2 * bx;
      next_a[out_off + (long long)by * S2 + bx] = ((pa[i] + pa[i + 1]) + (pa[i + PS] + pa[i + PS + 1])) * 0.25f;
      next_b[out_off + (long long)by * S2 + bx] = ((pb[i] + pb[i + 1]) + (pb[i + PS] + pb[i + PS + 1])) * 0.25f;
    }
  }

  // ---- along x: one item = one patch row x 4 adjacent output columns (a sliding window of KS + 3 inputs)
  for (int it = tid; it < PH * (kTile / 4); it += 256) {
    const int r = it >> 3, q0 = (it & 7) * 4;
    float va[KS + 3], vb[KS + 3];
#pragma unroll
    for (int k = 0; k < KS + 3; ++k) {
      va[k] = pa[r * PS + q0 + k];
      vb[k] = pb[r * PS + q0 + k];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float ma = 0.f, mb = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const float w = win.g[k], x = va[j + k], y = vb[j + k];
        ma = fmaf(w, x, ma);
        mb = fmaf(w, y, mb);
        aa = fmaf(w, x * x, aa);
        bb = fmaf(w, y * y, bb);
        ab = fmaf(w, x * y, ab);
      }
      const int o = r * kHStride + q0 + j;
      h[0][o] = ma; h[1][o] = mb; h[2][o] = aa; h[3][o] = bb; h[4][o] = ab;
    }
  }
  __syncthreads();

  // ---- along y: one thread = one output column x 4 adjacent output rows; then cs and ssim of its (up to) 4 pixels
  const int col = tid & 31, r0 = (tid >> 5) * 4;
  float acc[5][4];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[q][j] = 0.f;
#pragma unroll
    for (int k = 0; k < KS + 3; ++k) {
      const float v = h[q][(r0 + k) * kHStride + col];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k - j >= 0 && k - j < KS) acc[q][j] = fmaf(win.g[k - j], v, acc[q][j]);
    }
  }
  double cs_sum = 0., ssim_sum = 0.;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (y0 + r0 + j < O && x0 + col < O) {
      float cs, ssim;
      ms_pixel(acc[0][j], acc[1][j], acc[2][j], acc[3][j], acc[4][j], c1, c2, cs, ssim);
      cs_sum += (double)cs;
      ssim_sum += (double)ssim;
    }
  }
  cs_sum = gl_block_sum_256d(cs_sum, red);
  ssim_sum = gl_block_sum_256d(ssim_sum, red);
  if (tid == 0) {
    part[2 * (long long)blockIdx.x] = cs_sum;
    part[2 * (long long)blockIdx.x + 1] = ssim_sum;
  }
}

// Where the partials of each level start in the workspace (in doubles), how many (cs, ssim) entries a pair has there, and over
// how many values its means run.
struct MsLayout {
  long long off[kLevels];
  int per_pair[kLevels];
  double count[kLevels];
};

MsLayout ms_layout(int P, int R) {
  MsLayout lay;
  long long off = 0;
  for (int i = 0; i < kLevels; ++i) {
    const int S = R >> i, t = ms_tiles(S), O = S - ms_window(S) + 1;
    lay.off[i] = off;
    lay.per_pair[i] = 3 * t * t;
    lay.count[i] = 3.0 * O * O;
    off += 2LL * P * lay.per_pair[i];
  }
  return lay;
}

struct MsWeights { double w[kLevels]; };

__global__ __launch_bounds__(64) void msssim_pair_kernel(const double* __restrict__ ws, double* __restrict__ table,
                                                         double* __restrict__ values, MsLayout lay, MsWeights wt) {
  const long long p = blockIdx.x;
  const int lane = threadIdx.x;
  double prod = 1.;
#pragma unroll
  for (int i = 0; i < kLevels; ++i) {
    const double* src = ws + lay.off[i] + 2 * p * lay.per_pair[i];
    double cs = 0., ss = 0.;
    for (int t = lane; t < lay.per_pair[i]; t += 64) {
      cs += src[2 * t];
      ss += src[2 * t + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cs += __shfl_xor(cs, o, 64);
      ss += __shfl_xor(ss, o, 64);
    }
    cs /= lay.count[i];
    ss /= lay.count[i];
    cs = cs < 0. ? 0. : cs;               // (a NaN stays a NaN)
    ss = ss < 0. ? 0. : ss;
    if (lane == 0) {
      table[(p * kLevels + i) * 2] = cs;
      table[(p * kLevels + i) * 2 + 1] = ss;
    }
    prod *= pow(i < kLevels - 1 ? cs : ss, wt.w[i]);
  }
  if (lane == 0) values[p] = prod;
}

// out[0] = mean of values, out[1..4] = mean CS_0..3, out[5] = mean SSIM_4; each one lane, pairs in index order
__global__ __launch_bounds__(64) void msssim_mean_kernel(const double* __restrict__ table, const double* __restrict__ values,
                                                         double* __restrict__ out, int P) {
  const int k = threadIdx.x;
  if (k > kLevels) return;
  const double* src = k == 0 ? values : (k < kLevels ? table + 2 * (k - 1) : table + 2 * (kLevels - 1) + 1);
  const int stride = k == 0 ? 1 : 2 * kLevels;
  double s = 0.;
#pragma unroll 8
  for (int p = 0; p < P; ++p) s += src[(long long)p * stride];
  out[k] = s / (double)P;
}

bool ms_res_ok(int R) { return R >= (1 << (kLevels - 1)) && R <= 16384 && !(R & (R - 1)); }

size_t ms_workspace_bytes(int P, int R) {
  const MsLayout lay = ms_layout(P, R);
  return (size_t)(lay.off[kLevels - 1] + 2LL * P * lay.per_pair[kLevels - 1]) * sizeof(double);
}

}  // namespace

extern "C" {

size_t ganlab_msssim_workspace(int P, int R) {
  if (P <= 0 || !ms_res_ok(R)) return 0;
  return ms_workspace_bytes(P, R);
}

int ganlab_msssim_level_f32(const float* a, const float* b, long long pair_stride, float* next_a, float* next_b,
                            long long next_pair_stride, int first, int count, int P, int R, int level, float c1, float c2,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!a || !b || !workspace || P <= 0 || !ms_res_ok(R) || level < 0 || level >= kLevels || first < 0 || count <= 0 ||
      (long long)first + count > P || (next_a == nullptr) != (next_b == nullptr) || !(c1 > 0.f) || !(c2 > 0.f))
    return GANLAB_EINVAL;
  const int S = R >> level;
  if (pair_stride < 3LL * S * S) return GANLAB_EINVAL;
  if (next_a && (level == kLevels - 1 || next_pair_stride < 3LL * (S / 2) * (S / 2))) return GANLAB_EINVAL;
  if (workspace_bytes < ms_workspace_bytes(P, R)) return GANLAB_EWORKSPACE;
  const int s = ms_window(S), tiles = ms_tiles(S);
  const long long blocks = 3LL * count * tiles * tiles;
  if (blocks > 0x7fffffffLL) return GANLAB_EUNSUPPORTED;
  // the window: float64 on the host, rounded to fp32 for the kernel; taps beyond s are zero and never read
  MsWindow win;
  double g[kWin], sum = 0.;
  const double sigma = 1.5 * s / kWin;
  for (int k = 0; k < s; ++k) {
    const double d = k - (s - 1) / 2.0;
    g[k] = std::exp(-d * d / (2.0 * sigma * sigma));
    sum += g[k];
  }
  for (int k = 0; k < kWin; ++k) win.g[k] = k < s ? (float)(g[k] / sum) : 0.f;
  const MsLayout lay = ms_layout(P, R);
  double* part = reinterpret_cast<double*>(workspace) + lay.off[level] + 2LL * first * lay.per_pair[level];
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t st = gl_stream(stream);
#define MS_LAUNCH(KS)                                                                                                      \
  GL_LAUNCH(msssim_level_kernel<KS>, grid, block, 0, st, a, b, pair_stride, next_a, next_b, next_pair_stride, part, win, S, \
            tiles, c1, c2)
  switch (s) {
    case 11: MS_LAUNCH(11); break;
    case 8: MS_LAUNCH(8); break;
    case 4: MS_LAUNCH(4); break;
    case 2: MS_LAUNCH(2); break;
    default: MS_LAUNCH(1); break;
  }
#undef MS_LAUNCH
  return GL_CHECK_LAUNCH();
}

int ganlab_msssim_finish_f64(const void* workspace, size_t workspace_bytes, int P, int R, double* table, double* values,
                             double* out, void* stream) {
  if (!workspace || !table || !values || !out || P <= 0 || !ms_res_ok(R)) return GANLAB_EINVAL;
  if (workspace_bytes < ms_workspace_bytes(P, R)) return GANLAB_EWORKSPACE;
  const MsWeights wt = {{0.0448, 0.2856, 0.3001, 0.2363, 0.1333}};
  hipStream_t st = gl_stream(stream);
  GL_LAUNCH(msssim_pair_kernel, dim3(P), dim3(64), 0, st, reinterpret_cast<const double*>(workspace), table, values,
            ms_layout(P, R), wt);
  GL_LAUNCH(msssim_mean_kernel, dim3(1), dim3(64), 0, st, table, values, out, P);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
