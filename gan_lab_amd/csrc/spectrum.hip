// Azimuthally averaged power spectrum of (3, R, R) images (Durall et al. 2020; Dzanic et al. 2020): the frequency-content
// validation metric behind gan_lab_amd/spectrum.py.  DESIGN.md 4.9 has the definition.
//   tables   the Hann window and the R/2 twiddle factors exp(-2 pi i k / R), computed in double and rounded to fp32
//   rows     one workgroup = 1024 / R pairs of image rows.  Two real rows (window applied on load) are the real and imaginary
//            part of one complex FFT of length R in LDS; the Hermitian symmetry separates them, and columns 0 .. R/2 of both
//            rows go to the half-spectrum scratch, the only intermediate that reaches memory.
//   cols     one workgroup = a tile of C adjacent columns of one image.  Per channel it stages the tile (C x 8 contiguous
//            bytes per row), transforms its columns in LDS, and one lane per (column, bin) adds |F|^2 over the contiguous run of
//            rows |kv| the bin owns in that column, in fp64 and in a fixed order.  The tile's columns are then added per bin
//            with the half-spectrum weights (1 for columns 0 and R/2, 2 between): one fp64 partial per (image, tile, bin).
//   profile  per image and bin: the tiles in index order, over (members of the bin) x 3 R^2 W.
//   finish   the set profile (images in index order), decibels, and the two distances.
// The FFT is an in-place radix-2 decimation in frequency whose stages are taken two at a time (a radix-4 pass in registers);
// output slot s holds frequency bitrev(s), which binning and the Hermitian split look up instead of reordering.
// No atomics: every result is bitwise reproducible and does not depend on how the images were split over calls.
//
// The regulariser (gan_lab_amd/spectrum_reg.py) is the second half of the file: the same forward up to the per-image
// profiles, then
//   reg finish  S[k], L = mean_{k in B} (ln S[k] - ln T[k])^2 as one fp32 scalar, and coef[k] = dL/dS[k] / (N members_k 3 R^2 W)
//   target      T <- decay T + (1 - decay) S, or T <- S
//   cols bwd    per column tile of the recomputed half spectrum: the column transform again, every coefficient times
//               coef[bin] dL (the same integer binning), conjugated and put into natural order, transformed once more (the inverse
//               transform as the forward one on conjugated data) and written back over the tile, unnormalised
//   rows bwd    two rows of the result are completed by Hermitian symmetry and packed as real and imaginary part of one inverse
//               transform; times 2 (the 2 R^2 of the adjoint over the two unnormalised inverses) and the window -> dx
#include <cmath>

#include "common.h"

namespace {

constexpr int kMinRes = GANLAB_SPECTRUM_MIN_RES, kMaxRes = GANLAB_SPECTRUM_MAX_RES;
constexpr int kThreads = 256;
constexpr int kRowElems = 1024;           // complex elements of a rows workgroup: 8 KiB of LDS, 1024 / R transforms
constexpr int kColElems = 4096;           // ... of a cols workgroup: 32 KiB; C = min(16, 4096 / R) columns
constexpr double kDbFloor = 1e-30;

__host__ __device__ constexpr int sp_log2(int R) { return R <= 1 ? 0 : 1 + sp_log2(R >> 1); }
__host__ __device__ constexpr int sp_cols(int R) { return kColElems / R < 16 ? kColElems / R : 16; }
__host__ __device__ inline int sp_bins(int R) { return R / 2 + 1; }
__host__ __device__ inline int sp_tiles(int R) { return (R / 2 + 1 + sp_cols(R) - 1) / sp_cols(R); }

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return float2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// B in-place FFTs of length R in LDS, transform b at buf + b * stride; tw[k] = exp(-2 pi i k / R), k < R / 2.  Decimation in
// frequency: the stage of half-size h maps (x[i], x[i + h]) to (x[i] + x[i + h], (x[i] - x[i + h]) tw[k R / (2 h)]), k = i mod h.
// Two stages (h, h / 2) touch the same four elements and are done in registers; an odd log2 R ends with the stage h = 1.
// On return slot s of a transform holds the coefficient of frequency bitrev(s).  Every thread of the workgroup calls it.
template <int R>
__device__ __forceinline__ void sp_fft(float2* __restrict__ buf, const float2* __restrict__ tw, int B, int stride) {
  constexpr int LOG = sp_log2(R);
  int h = R / 2;
#pragma unroll
  for (int pass = 0; pass < LOG / 2; ++pass, h >>= 2) {
    const int q = h >> 1, s = R / (2 * h);
    __syncthreads();
    for (int it = threadIdx.x; it < B * (R / 4); it += kThreads) {
      const int b = it / (R / 4), t = it - b * (R / 4);
      const int grp = t / q, k = t - grp * q;
      float2* p = buf + b * stride + grp * 2 * h + k;
      const float2 e0 = p[0], e1 = p[q], e2 = p[h], e3 = p[h + q];
      const float2 w1 = tw[k * s], w2 = tw[(k + q) * s], w3 = tw[2 * k * s];
      const float2 a0 = float2{e0.x + e2.x, e0.y + e2.y}, a2 = cmul(float2{e0.x - e2.x, e0.y - e2.y}, w1);
      const float2 a1 = float2{e1.x + e3.x, e1.y + e3.y}, a3 = cmul(float2{e1.x - e3.x, e1.y - e3.y}, w2);
      p[0] = float2{a0.x + a1.x, a0.y + a1.y};
      p[q] = cmul(float2{a0.x - a1.x, a0.y - a1.y}, w3);
      p[h] = float2{a2.x + a3.x, a2.y + a3.y};
      p[h + q] = cmul(float2{a2.x - a3.x, a2.y - a3.y}, w3);
    }
  }
  if (LOG & 1) {                          // h == 1: the twiddle is 1
    __syncthreads();
    for (int it = threadIdx.x; it < B * (R / 2); it += kThreads) {
      const int b = it / (R / 2), t = it - b * (R / 2);
      float2* p = buf + b * stride + 2 * t;
      const float2 e0 = p[0], e1 = p[1];
      p[0] = float2{e0.x + e1.x, e0.y + e1.y};
      p[1] = float2{e0.x - e1.x, e0.y - e1.y};
    }
  }
  __syncthreads();
}

template <int R>
__device__ __forceinline__ int sp_slot(int f) { return (int)(__brev((unsigned)f) >> (32 - sp_log2(R))); }

// win[R], tw[R / 2] (as float2) behind it: double precision, rounded once
__global__ __launch_bounds__(kThreads) void spectrum_tables_kernel(float* __restrict__ tab, int R, int hann) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= R) return;
  tab[i] = hann ? (float)(0.5 - 0.5 * cospi(2.0 * i / R)) : 1.f;
  if (i < R / 2) {
    tab[R + 2 * i] = (float)cospi(2.0 * i / R);
    tab[R + 2 * i + 1] = (float)(-sinpi(2.0 * i / R));
  }
}

// half[plane][row][v], v = 0 .. R/2 (row length R/2 + 1 float2), plane = image * 3 + channel of this call's images
template <int R>
__global__ __launch_bounds__(kThreads) void spectrum_rows_kernel(const float* __restrict__ x, long long image_stride,
                                                                 const float* __restrict__ tab, float2* __restrict__ half,
                                                                 long long pairs) {
  constexpr int B = kRowElems / R, NB = R / 2 + 1;
  __shared__ float2 buf[kRowElems];
  __shared__ float2 tw[R / 2];
  __shared__ float win[R];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * B;
  for (int i = tid; i < R; i += kThreads) win[i] = tab[i];
  for (int i = tid; i < R / 2; i += kThreads) tw[i] = float2{tab[R + 2 * i], tab[R + 2 * i + 1]};
  __syncthreads();
  for (int e = tid; e < B * R; e += kThreads) {
    const int b = e / R, j = e - b * R;
    const long long p = p0 + b;
    float2 z = float2{0.f, 0.f};
    if (p < pairs) {
      const long long plane = p / (R / 2);
      const int r = (int)(p - plane * (R / 2));
      const long long img = plane / 3;
      const float* src = x + img * image_stride + (plane - img * 3) * (long long)(R * R) + (long long)(2 * r) * R + j;
      z.x = (src[0] * win[j]) * win[2 * r];
      z.y = (src[R] * win[j]) * win[2 * r + 1];
    }
    buf[e] = z;
  }
  sp_fft<R>(buf, tw, B, R);
  // Z = X0 + i X1 with X0, X1 the transforms of the two real rows: X0[v] = (Z[v] + conj Z[-v]) / 2, X1[v] = (Z[v] - conj Z[-v]) / 2i
  for (int e = tid; e < B * NB; e += kThreads) {
    const int b = e / NB, v = e - b * NB;
    const long long p = p0 + b;
    if (p >= pairs) continue;
    const float2 z = buf[b * R + sp_slot<R>(v)], y = buf[b * R + sp_slot<R>((R - v) & (R - 1))];
    float2* dst = half + (2 * p) * NB + v;          // row 2 r of the pair's plane: rows are NB apart and planes R rows
    dst[0] = float2{0.5f * (z.x + y.x), 0.5f * (z.y - y.y)};
    dst[NB] = float2{0.5f * (z.y + y.y), -0.5f * (z.x - y.x)};
  }
}

// Rows |kv| = m of column ku = v that belong to bin k form the run [lo(k), lo(k + 1)) of m, where lo(k) is the smallest
// m >= 0 with 4 (v^2 + m^2) >= (2 k - 1)^2, and lo(0) = 0: the nearest-integer radius, in exact integer arithmetic.
__host__ __device__ inline int sp_run_lo(int v, int k) {
  if (k <= 0) return 0;
  const long long t = (long long)(2 * k - 1) * (2 * k - 1) - 4LL * v * v;
  if (t <= 0) return 0;
  long long m = (long long)(sqrt((double)t) * 0.5);
  while (4 * m * m < t) ++m;
  while (m > 0 && 4 * (m - 1) * (m - 1) >= t) --m;
  return (int)m;
}

// part[(image * tiles + tile) * NB + k], fp64
template <int R>
__global__ __launch_bounds__(kThreads) void spectrum_cols_kernel(const float2* __restrict__ half, const float* __restrict__ tab,
                                                                 double* __restrict__ part) {
  constexpr int C = sp_cols(R), NB = R / 2 + 1, STRIDE = R + 1, ITEMS = (C * NB + kThreads - 1) / kThreads;
  constexpr int TILES = (NB + C - 1) / C;
  static_assert(C * NB * sizeof(double) <= C * STRIDE * sizeof(float2), "the per-column bin sums reuse the FFT buffer");
  __shared__ float2 buf[C * STRIDE];
  __shared__ float2 tw[R / 2];
  const int tid = threadIdx.x;
  const long long img = blockIdx.x / TILES;
  const int tile = (int)(blockIdx.x - img * TILES);
  const int v0 = tile * C;
  for (int i = tid; i < R / 2; i += kThreads) tw[i] = float2{tab[R + 2 * i], tab[R + 2 * i + 1]};

  // the items (column c, bin k) of this thread and their runs of |kv|; a run is empty for a column outside the spectrum
  int lo[ITEMS], hi[ITEMS];
  double acc[ITEMS];
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int it = tid + s * kThreads;
    const int c = it / NB, k = it - c * NB;
    const bool live = it < C * NB && v0 + c < NB;
    lo[s] = live ? sp_run_lo(v0 + c, k) : 0;
    hi[s] = live ? min(sp_run_lo(v0 + c, k + 1), R / 2 + 1) : 0;
    acc[s] = 0.;
  }

  for (int ch = 0; ch < 3; ++ch) {
    const float2* src = half + (img * 3 + ch) * (long long)R * NB;
    __syncthreads();                                // the previous channel's sums have read buf
    for (int e = tid; e < C * R; e += kThreads) {
      const int u = e / C, c = e - u * C;
      buf[c * STRIDE + u] = v0 + c < NB ? src[(long long)u * NB + v0 + c] : float2{0.f, 0.f};
    }
    sp_fft<R>(buf, tw, C, STRIDE);
#pragma unroll
    for (int s = 0; s < ITEMS; ++s) {
      const int it = tid + s * kThreads;
      const float2* col = buf + (it / NB) * STRIDE;
      for (int m = lo[s]; m < hi[s]; ++m) {         // row kv = m, then row kv = -m where that is another row
        const float2 f = col[sp_slot<R>(m)];
        acc[s] += (double)(f.x * f.x + f.y * f.y);
        if (m > 0 && m < R / 2) {
          const float2 g = col[sp_slot<R>(R - m)];
          acc[s] += (double)(g.x * g.x + g.y * g.y);
        }
      }
    }
  }

  __syncthreads();
  double* sums = reinterpret_cast<double*>(buf);   // [c][k]
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int it = tid + s * kThreads;
    if (it < C * NB) sums[it] = acc[s];
  }
  __syncthreads();
  for (int k = tid; k < NB; k += kThreads) {
    double t = 0.;
    for (int c = 0; c < C; ++c) {
      const int v = v0 + c;
      if (v < NB) t += (v == 0 || v == R / 2 ? 1. : 2.) * sums[c * NB + k];
    }
    part[((long long)img * TILES + tile) * NB + k] = t;
  }
}

// prof[image][k] = (sum of the image's tiles) / (members of bin k x 3 R^2 W)
__global__ __launch_bounds__(kThreads) void spectrum_profile_kernel(const double* __restrict__ part, double* __restrict__ prof,
                                                                    int R, int tiles, double inv_norm) {
  const int NB = R / 2 + 1;
  const int k = blockIdx.y * kThreads + threadIdx.x;
  if (k >= NB) return;
  const long long img = blockIdx.x;
  long long members = 0;
  for (int v = 0; v <= R / 2; ++v) {
    const int a = sp_run_lo(v, k), b = min(sp_run_lo(v, k + 1), R / 2 + 1);
    if (b <= a) continue;
    const int rows = 2 * (b - a) - (a == 0 ? 1 : 0) - (b == R / 2 + 1 ? 1 : 0);   // kv = 0 and kv = -R/2 are one row each
    members += (v == 0 || v == R / 2 ? 1 : 2) * rows;
  }
  double t = 0.;
  for (int i = 0; i < tiles; ++i) t += part[(img * tiles + i) * NB + k];
  prof[img * NB + k] = t * inv_norm / (double)members;
}

// out = power[NB], db[NB] of set a; with b: the same of set b behind them, then spectrum, hf
__global__ __launch_bounds__(kThreads) void spectrum_finish_kernel(const double* __restrict__ pa, const double* __restrict__ pb,
                                                                   double* __restrict__ out, int N, int R) {
  const int NB = R / 2 + 1;
  for (int set = 0; set < (pb ? 2 : 1); ++set) {
    const double* prof = set ? pb : pa;
    for (int k = threadIdx.x; k < NB; k += kThreads) {
      double t = 0.;
      for (int n = 0; n < N; ++n) t += prof[(long long)n * NB + k];
      t /= (double)N;
      out[set * 2 * NB + k] = t;
      out[set * 2 * NB + NB + k] = 10. * log10(t > kDbFloor ? t : kDbFloor);   // (a NaN is clamped too)
    }
  }
  if (!pb) return;
  __syncthreads();
  if (threadIdx.x < 2) {
    const int first = threadIdx.x == 0 ? 1 : R / 4 + 1;
    double t = 0.;
    for (int k = first; k <= R / 2; ++k) {
      const double d = out[2 * NB + NB + k] - out[NB + k];
      t += d * d;
    }
    out[4 * NB + threadIdx.x] = sqrt(t / (double)(R / 2 - first + 1));
  }
}

bool sp_res_ok(int R) { return R >= kMinRes && R <= kMaxRes && !(R & (R - 1)); }
size_t sp_tables_bytes(int R) { return (size_t)2 * R * sizeof(float); }
size_t sp_half_bytes(int R) { return (size_t)3 * R * sp_bins(R) * sizeof(float2); }
size_t sp_part_bytes(int R) { return (size_t)sp_tiles(R) * sp_bins(R) * sizeof(double); }

template <int R>
void sp_launch(const float* x, long long image_stride, int count, const float* tab, float2* half, double* part, hipStream_t st) {
  const long long pairs = 3LL * count * (R / 2);
  constexpr int B = kRowElems / R;
  GL_LAUNCH((spectrum_rows_kernel<R>), dim3((unsigned)((pairs + B - 1) / B)), dim3(kThreads), 0, st, x, image_stride, tab, half,
            pairs);
  GL_LAUNCH((spectrum_cols_kernel<R>), dim3((unsigned)(count * sp_tiles(R))), dim3(kThreads), 0, st, half, tab, part);
}

}  // namespace

extern "C" {

size_t ganlab_spectrum_workspace(int N, int R) {
  if (N <= 0 || !sp_res_ok(R)) return 0;
  return (size_t)N * sp_bins(R) * sizeof(double);
}

size_t ganlab_spectrum_scratch(int count, int R) {
  if (count <= 0 || !sp_res_ok(R)) return 0;
  return sp_tables_bytes(R) + (size_t)count * (sp_half_bytes(R) + sp_part_bytes(R));
}

int ganlab_spectrum_feed_f32(const float* x, long long image_stride, int first, int count, int N, int R, int window,
                             void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !scratch || !workspace || N <= 0 || R <= 0 || first < 0 || count <= 0 || (long long)first + count > N ||
      (window != GANLAB_SPECTRUM_WINDOW_NONE && window != GANLAB_SPECTRUM_WINDOW_HANN))
    return GANLAB_EINVAL;
  if (!sp_res_ok(R)) return GANLAB_EUNSUPPORTED;
  if (image_stride < 3LL * R * R) return GANLAB_EINVAL;
  if (workspace_bytes < ganlab_spectrum_workspace(N, R) || scratch_bytes < ganlab_spectrum_scratch(count, R))
    return GANLAB_EWORKSPACE;
  if (3LL * count * (R / 2) > 0x7fffffffLL) return GANLAB_EUNSUPPORTED;
  hipStream_t st = gl_stream(stream);
  float* tab = reinterpret_cast<float*>(scratch);
  float2* half = reinterpret_cast<float2*>(reinterpret_cast<char*>(scratch) + sp_tables_bytes(R));
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(half) + (size_t)count * sp_half_bytes(R));
  GL_LAUNCH(spectrum_tables_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, tab, R,
            window == GANLAB_SPECTRUM_WINDOW_HANN ? 1 : 0);
  switch (R) {
    case 16: sp_launch<16>(x, image_stride, count, tab, half, part, st); break;
    case 32: sp_launch<32>(x, image_stride, count, tab, half, part, st); break;
    case 64: sp_launch<64>(x, image_stride, count, tab, half, part, st); break;
    case 128: sp_launch<128>(x, image_stride, count, tab, half, part, st); break;
    case 256: sp_launch<256>(x, image_stride, count, tab, half, part, st); break;
    case 512: sp_launch<512>(x, image_stride, count, tab, half, part, st); break;
    default: sp_launch<1024>(x, image_stride, count, tab, half, part, st); break;
  }
  // W = (sum_i w[i]^2 / R)^2: (3/8)^2 for the periodic Hann window
  const double W = window == GANLAB_SPECTRUM_WINDOW_HANN ? 9. / 64. : 1.;
  const int NB = sp_bins(R);
  GL_LAUNCH(spectrum_profile_kernel, dim3((unsigned)count, (unsigned)((NB + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part,
            reinterpret_cast<double*>(workspace) + (long long)first * NB, R, sp_tiles(R), 1. / (3. * (double)R * (double)R * W));
  return GL_CHECK_LAUNCH();
}

int ganlab_spectrum_finish_f64(const void* workspace_a, const void* workspace_b, size_t workspace_bytes, int N, int R, double* out,
                               size_t out_bytes, void* stream) {
  if (!workspace_a || !out || N <= 0 || R <= 0) return GANLAB_EINVAL;
  if (!sp_res_ok(R)) return GANLAB_EUNSUPPORTED;
  if (workspace_bytes < ganlab_spectrum_workspace(N, R)) return GANLAB_EWORKSPACE;
  const size_t NB = (size_t)sp_bins(R);
  if (out_bytes < (workspace_b ? 4 * NB + 2 : 2 * NB) * sizeof(double)) return GANLAB_EINVAL;
  GL_LAUNCH(spectrum_finish_kernel, dim3(1), dim3(kThreads), 0, gl_stream(stream), reinterpret_cast<const double*>(workspace_a),
            reinterpret_cast<const double*>(workspace_b), out, N, R);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"

// ---- the power-spectrum regulariser: L(S, T) and its gradient with respect to the images -----------------------
namespace {

// the bin of the coefficient (|ku|, |kv|) = (v, m): the k with (2k-1)^2 <= 4 (v^2 + m^2) < (2k+1)^2, as sp_run_lo draws the runs
__device__ __forceinline__ int sp_bin(int v, int m) {
  const long long t = 4LL * ((long long)v * v + (long long)m * m);
  long long k = (long long)((sqrt((double)t) + 1.) * 0.5);
  while ((2 * k + 1) * (2 * k + 1) <= t) ++k;
  while (k > 0 && (2 * k - 1) * (2 * k - 1) > t) --k;
  return (int)k;
}

// the number of coefficients of bin k (spectrum_profile_kernel's count)
__device__ inline long long sp_members(int R, int k) {
  long long members = 0;
  for (int v = 0; v <= R / 2; ++v) {
    const int a = sp_run_lo(v, k), b = min(sp_run_lo(v, k + 1), R / 2 + 1);
    if (b <= a) continue;
    const int rows = 2 * (b - a) - (a == 0 ? 1 : 0) - (b == R / 2 + 1 ? 1 : 0);
    members += (v == 0 || v == R / 2 ? 1 : 2) * rows;
  }
  return members;
}

// S[k] exactly as spectrum_finish_kernel forms it: the images in index order, then one division
__device__ __forceinline__ double sp_set_mean(const double* __restrict__ prof, int N, int NB, int k) {
  double t = 0.;
  for (int n = 0; n < N; ++n) t += prof[(long long)n * NB + k];
  return t / (double)N;
}

// loss[0] = mean_{k = first .. R/2} (ln max(S[k], floor) - ln max(T[k], floor))^2;  coef[k] = dL/dS[k] inv_norm / (N members_k),
// 0 outside the band and where S[k] sits on the floor
__global__ __launch_bounds__(kThreads) void spectrum_reg_finish_kernel(const double* __restrict__ prof,
                                                                       const double* __restrict__ target, float* __restrict__ loss,
                                                                       double* __restrict__ coef, int N, int R, int first,
                                                                       double inv_norm) {
  __shared__ double sq[kMaxRes / 2 + 1];
  const int NB = R / 2 + 1;
  const double band = (double)(R / 2 - first + 1);
  for (int k = threadIdx.x; k < NB; k += kThreads) {
    double d2 = 0., c = 0.;
    if (k >= first) {
      const double s = sp_set_mean(prof, N, NB, k), t = target[k];
      const double d = log(s > kDbFloor ? s : kDbFloor) - log(t > kDbFloor ? t : kDbFloor);
      d2 = d * d;
      if (s > kDbFloor) c = 2. * d / (band * s) * inv_norm / ((double)N * (double)sp_members(R, k));
    }
    sq[k] = d2;
    coef[k] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.;
    for (int k = first; k <= R / 2; ++k) t += sq[k];
    loss[0] = (float)(t / band);
  }
}

__global__ __launch_bounds__(kThreads) void spectrum_reg_target_kernel(const double* __restrict__ prof, double* __restrict__ target,
                                                                       int N, int R, double decay, int first) {
  const int NB = R / 2 + 1;
  for (int k = threadIdx.x; k < NB; k += kThreads) {
    const double s = sp_set_mean(prof, N, NB, k);
    target[k] = first ? s : decay * target[k] + (1. - decay) * s;
  }
}

// half: the row-transformed half spectra of this call's images (spectrum_rows_kernel); on return the unnormalised inverse column
// transform of coef[bin] dL F in their place.  One workgroup owns its tile's columns of one image: no other touches them.
template <int R>
__global__ __launch_bounds__(kThreads) void spectrum_reg_cols_bwd_kernel(float2* __restrict__ half, const float* __restrict__ tab,
                                                                         const double* __restrict__ coef,
                                                                         const float* __restrict__ grad_loss) {
  constexpr int C = sp_cols(R), NB = R / 2 + 1, STRIDE = R + 1, TILES = (NB + C - 1) / C;
  __shared__ float2 buf[C * STRIDE];
  __shared__ float2 tw[R / 2];
  __shared__ float wk[NB];
  const int tid = threadIdx.x;
  const long long img = blockIdx.x / TILES;
  const int tile = (int)(blockIdx.x - img * TILES);
  const int v0 = tile * C;
  for (int i = tid; i < R / 2; i += kThreads) tw[i] = float2{tab[R + 2 * i], tab[R + 2 * i + 1]};
  const double gl = (double)grad_loss[0];
  for (int k = tid; k < NB; k += kThreads) wk[k] = (float)(coef[k] * gl);

  for (int ch = 0; ch < 3; ++ch) {
    float2* plane = half + (img * 3 + ch) * (long long)R * NB;
    __syncthreads();                                // the previous channel's stores have read buf
    for (int e = tid; e < C * R; e += kThreads) {
      const int u = e / C, c = e - u * C;
      buf[c * STRIDE + u] = v0 + c < NB ? plane[(long long)u * NB + v0 + c] : float2{0.f, 0.f};
    }
    sp_fft<R>(buf, tw, C, STRIDE);
    // slot s holds frequency bitrev(s): weight both ends of the swap, conjugate, and leave frequency f in slot f
    for (int e = tid; e < C * R; e += kThreads) {
      const int c = e / R, s = e - c * R, f = sp_slot<R>(s);
      if (f < s) continue;
      float2* col = buf + c * STRIDE;
      const float2 a = col[s], b = col[f];          // frequencies f and s
      const int ka = sp_bin(v0 + c, f < R / 2 ? f : R - f), kb = sp_bin(v0 + c, s < R / 2 ? s : R - s);
      const float wa = ka <= R / 2 ? wk[ka] : 0.f, wb = kb <= R / 2 ? wk[kb] : 0.f;
      col[f] = float2{a.x * wa, -(a.y * wa)};
      col[s] = float2{b.x * wb, -(b.y * wb)};
    }
    sp_fft<R>(buf, tw, C, STRIDE);
    for (int e = tid; e < C * R; e += kThreads) {
      const int u = e / C, c = e - u * C;
      if (v0 + c >= NB) continue;
      const float2 z = buf[c * STRIDE + sp_slot<R>(u)];
      plane[(long long)u * NB + v0 + c] = float2{z.x, -z.y};
    }
  }
}

// dx[plane][2 r], dx[plane][2 r + 1] from rows 2 r, 2 r + 1 of the plane's half[row][v]; dx is contiguous
template <int R>
__global__ __launch_bounds__(kThreads) void spectrum_reg_rows_bwd_kernel(const float2* __restrict__ half, const float* __restrict__ tab,
                                                                         float* __restrict__ dx, long long pairs) {
  constexpr int B = kRowElems / R, NB = R / 2 + 1;
  __shared__ float2 buf[kRowElems];
  __shared__ float2 tw[R / 2];
  __shared__ float win[R];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * B;
  for (int i = tid; i < R; i += kThreads) win[i] = tab[i];
  for (int i = tid; i < R / 2; i += kThreads) tw[i] = float2{tab[R + 2 * i], tab[R + 2 * i + 1]};
  __syncthreads();
  // A0, A1: the spectra of two real rows, A[R - v] = conj A[v], imaginary parts of v = 0 and R/2 dropped.  conj(A0 + i A1) goes in:
  // the forward transform of it is conj(R (a0 + i a1))
  for (int e = tid; e < B * R; e += kThreads) {
    const int b = e / R, v = e - b * R;
    const long long p = p0 + b;
    float2 z = float2{0.f, 0.f};
    if (p < pairs) {
      const int w = v <= R / 2 ? v : R - v;
      const float2* src = half + (2 * p) * NB + w;
      float2 a0 = src[0], a1 = src[NB];
      if (w == 0 || w == R / 2) a0.y = a1.y = 0.f;
      if (v > R / 2) { a0.y = -a0.y; a1.y = -a1.y; }
      z = float2{a0.x - a1.y, -(a0.y + a1.x)};
    }
    buf[e] = z;
  }
  sp_fft<R>(buf, tw, B, R);
  for (int e = tid; e < B * R; e += kThreads) {
    const int b = e / R, j = e - b * R;
    const long long p = p0 + b;
    if (p >= pairs) continue;
    const long long plane = p / (R / 2);
    const int r = (int)(p - plane * (R / 2));
    const float2 z = buf[b * R + sp_slot<R>(j)];
    float* dst = dx + plane * (long long)(R * R) + (long long)(2 * r) * R + j;
    dst[0] = ((2.f * z.x) * win[j]) * win[2 * r];
    dst[R] = ((-2.f * z.y) * win[j]) * win[2 * r + 1];
  }
}

template <int R>
void sp_reg_launch(const float* x, long long image_stride, int count, const float* tab, float2* half, const double* coef,
                   const float* grad_loss, float* dx, hipStream_t st) {
  const long long pairs = 3LL * count * (R / 2);
  constexpr int B = kRowElems / R;
  const dim3 rows((unsigned)((pairs + B - 1) / B));
  GL_LAUNCH((spectrum_rows_kernel<R>), rows, dim3(kThreads), 0, st, x, image_stride, tab, half, pairs);
  GL_LAUNCH((spectrum_reg_cols_bwd_kernel<R>), dim3((unsigned)(count * sp_tiles(R))), dim3(kThreads), 0, st, half, tab, coef,
            grad_loss);
  GL_LAUNCH((spectrum_reg_rows_bwd_kernel<R>), rows, dim3(kThreads), 0, st, half, tab, dx, pairs);
}

bool sp_window_ok(int window) { return window == GANLAB_SPECTRUM_WINDOW_NONE || window == GANLAB_SPECTRUM_WINDOW_HANN; }

}  // namespace

extern "C" {

size_t ganlab_spectrum_reg_scratch(int count, int R) {
  if (count <= 0 || !sp_res_ok(R)) return 0;
  return sp_tables_bytes(R) + (size_t)count * sp_half_bytes(R);
}

int ganlab_spectrum_reg_finish_f64(const void* workspace, size_t workspace_bytes, int N, int R, int window, int band,
                                   const double* target, float* loss, double* coef, void* stream) {
  if (!workspace || !target || !loss || !coef || N <= 0 || R <= 0 || !sp_window_ok(window) ||
      (band != GANLAB_SPECTRUM_BAND_ALL && band != GANLAB_SPECTRUM_BAND_HF))
    return GANLAB_EINVAL;
  if (!sp_res_ok(R)) return GANLAB_EUNSUPPORTED;
  if (workspace_bytes < ganlab_spectrum_workspace(N, R)) return GANLAB_EWORKSPACE;
  const double W = window == GANLAB_SPECTRUM_WINDOW_HANN ? 9. / 64. : 1.;
  GL_LAUNCH(spectrum_reg_finish_kernel, dim3(1), dim3(kThreads), 0, gl_stream(stream), reinterpret_cast<const double*>(workspace),
            target, loss, coef, N, R, band == GANLAB_SPECTRUM_BAND_HF ? R / 4 + 1 : 1, 1. / (3. * (double)R * (double)R * W));
  return GL_CHECK_LAUNCH();
}

int ganlab_spectrum_reg_target_f64(const void* workspace, size_t workspace_bytes, int N, int R, double decay, int first,
                                   double* target, void* stream) {
  if (!workspace || !target || N <= 0 || R <= 0 || !(decay >= 0. && decay < 1.)) return GANLAB_EINVAL;
  if (!sp_res_ok(R)) return GANLAB_EUNSUPPORTED;
  if (workspace_bytes < ganlab_spectrum_workspace(N, R)) return GANLAB_EWORKSPACE;
  GL_LAUNCH(spectrum_reg_target_kernel, dim3(1), dim3(kThreads), 0, gl_stream(stream), reinterpret_cast<const double*>(workspace),
            target, N, R, decay, first ? 1 : 0);
  return GL_CHECK_LAUNCH();
}

int ganlab_spectrum_reg_backward_f32(const float* x, long long image_stride, int count, int R, int window, const double* coef,
                                     const float* grad_loss, float* dx, void* scratch, size_t scratch_bytes, void* stream) {
  if (!x || !coef || !grad_loss || !dx || !scratch || count <= 0 || R <= 0 || !sp_window_ok(window)) return GANLAB_EINVAL;
  if (!sp_res_ok(R)) return GANLAB_EUNSUPPORTED;
  if (image_stride < 3LL * R * R) return GANLAB_EINVAL;
  if (scratch_bytes < ganlab_spectrum_reg_scratch(count, R)) return GANLAB_EWORKSPACE;
  if (3LL * count * (R / 2) > 0x7fffffffLL) return GANLAB_EUNSUPPORTED;
  hipStream_t st = gl_stream(stream);
  float* tab = reinterpret_cast<float*>(scratch);
  float2* half = reinterpret_cast<float2*>(reinterpret_cast<char*>(scratch) + sp_tables_bytes(R));
  GL_LAUNCH(spectrum_tables_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, tab, R,
            window == GANLAB_SPECTRUM_WINDOW_HANN ? 1 : 0);
  switch (R) {
    case 16: sp_reg_launch<16>(x, image_stride, count, tab, half, coef, grad_loss, dx, st); break;
    case 32: sp_reg_launch<32>(x, image_stride, count, tab, half, coef, grad_loss, dx, st); break;
    case 64: sp_reg_launch<64>(x, image_stride, count, tab, half, coef, grad_loss, dx, st); break;
    case 128: sp_reg_launch<128>(x, image_stride, count, tab, half, coef, grad_loss, dx, st); break;
    case 256: sp_reg_launch<256>(x, image_stride, count, tab, half, coef, grad_loss, dx, st); break;
    case 512: sp_reg_launch<512>(x, image_stride, count, tab, half, coef, grad_loss, dx, st); break;
    default: sp_reg_launch<1024>(x, image_stride, count, tab, half, coef, grad_loss, dx, st); break;
  }
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
