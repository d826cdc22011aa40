// Sliced Wasserstein distance between Laplacian-pyramid patch descriptors (Karras et al. 2018, "Progressive Growing of GANs",
// section 5 / appendix): the validation metric of gan_lab_amd/swd.py.  DESIGN.md 4.7 has the definition; the stages are
//   down        f (x) f, f = [1,4,6,4,1]/16, mirror boundary (the edge sample is not repeated), only the kept (even) pixels
//   band        gauss[i] - up(gauss[i+1]); up = zero insertion at the even positions, then (2f) (x) (2f) with mirror boundary.  The
//               mirrored index keeps its parity, so an even output row / column has the 3 taps (1,6,1)/8 and an odd one (4,4)/8
//   gather      (N, n, 2) int32 centres -> (N n, 147) rows in (channel, dy, dx) order, plus per-image fp64 sums of v and v^2 per
//               channel (one workgroup per image, fixed order: the statistics of a set do not depend on how it was fed)
//   project     out[d][m] = sum_k dirs[d][k] (desc[m][k] - mean_c) / std_c on v_mfma_f32_16x16x4_f32, K padded to 148
//   sort        ascending, per direction (rocPRIM radix sorts: bitwise the order of any other correct sort of finite keys)
//   distance    sum |a - b| over two sorted (D, M) buffers / (D M), fp64 partials in a fixed order
// No float atomics anywhere: every result is bitwise reproducible.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "common.h"

namespace {

constexpr int kDesc = GANLAB_SWD_DESC;      // 147 = 3 channels x 7 x 7
constexpr int kKPad = 148;                  // K of the projection, padded to the MFMA's 4; also the LDS row stride: rows 0..15 x
                                            // k 0..3 fall on 64 distinct banks (148 = 20 mod 64)
constexpr int kTileM = 64, kTileD = 128;    // projection workgroup tile: 64 descriptors x 128 directions

__device__ __forceinline__ int swd_mirror(int q, int n) { return q < 0 ? -q : (q >= n ? 2 * (n - 1) - q : q); }

// ---- pyramid --------------------------------------------------------------------------------------------------------------
// One thread = one kept pixel: 25 taps read through the caches (a wave's 64 outputs of a row share 132 input floats per row).
__global__ __launch_bounds__(256) void swd_down_kernel(const float* __restrict__ x, float* __restrict__ y, long long planes,
                                                       int H, int W) {
  const int H2 = H >> 1, W2 = W >> 1, hw2 = H2 * W2;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= planes * hw2) return;
  const long long p = gid / hw2;
  const int r = (int)(gid - p * hw2), i = r / W2, j = r - i * W2;
  const float* src = x + p * (long long)H * W;
  const float f[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  int cols[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) cols[b] = swd_mirror(2 * j + b - 2, W);
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const float* row = src + (long long)swd_mirror(2 * i + a - 2, H) * W;
    float h = 0.f;
#pragma unroll
    for (int b = 0; b < 5; ++b) h = fmaf(f[b], row[cols[b]], h);
    acc = fmaf(f[a], h, acc);
  }
  y[gid] = acc;
}

// taps of the zero-insert upsample along one axis at output index i: source indices (in the half-size plane) and weights of 2f
__device__ __forceinline__ int swd_up_taps(int i, int n, int (&idx)[3], float (&w)[3]) {
  if (i & 1) {
    idx[0] = swd_mirror(i - 1, n) >> 1; w[0] = 0.5f;
    idx[1] = swd_mirror(i + 1, n) >> 1; w[1] = 0.5f;
    idx[2] = 0; w[2] = 0.f;
    return 2;
  }
  idx[0] = swd_mirror(i - 2, n) >> 1; w[0] = 0.125f;
  idx[1] = i >> 1; w[1] = 0.75f;
  idx[2] = swd_mirror(i + 2, n) >> 1; w[2] = 0.125f;
  return 3;
}

__global__ __launch_bounds__(256) void swd_band_kernel(const float* __restrict__ g0, const float* __restrict__ g1,
                                                       float* __restrict__ out, long long planes, int H, int W) {
  const int hw = H * W, W2 = W >> 1;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= planes * hw) return;
  const long long p = gid / hw;
  const int r = (int)(gid - p * hw), i = r / W, j = r - i * W;
  const float* src = g1 + p * (long long)(hw >> 2);
  int ri[3], ci[3];
  float rw[3], cw[3];
  const int nr = swd_up_taps(i, H, ri, rw), nc = swd_up_taps(j, W, ci, cw);
  float acc = 0.f;
  for (int a = 0; a < nr; ++a) {
    const float* row = src + (long long)ri[a] * W2;
    float h = 0.f;
    for (int b = 0; b < nc; ++b) h = fmaf(cw[b], row[ci[b]], h);
    acc = fmaf(rw[a], h, acc);
  }
  out[gid] = g0[gid] - acc;
}

// ---- descriptors ----------------------------------------------------------------------------------------------------------
// One workgroup = one image: its n x 147 descriptor floats in order (coalesced stores), the 7 x 7 x 3 windows read through the
// caches.  Centres are clamped to [3, S - 4] so that no index can leave the plane, whatever the caller passed.
__global__ __launch_bounds__(256) void swd_gather_kernel(const float* __restrict__ band, const int* __restrict__ pos,
                                                         float* __restrict__ desc, double* __restrict__ partials, int n, int S) {
  __shared__ double red[4][6];
  const int img = blockIdx.x;
  const float* src = band + (long long)img * 3 * S * S;
  const int* pp = pos + (long long)img * n * 2;
  float* dst = desc + (long long)img * n * kDesc;
  double s[3] = {0., 0., 0.}, q[3] = {0., 0., 0.};
  const int total = n * kDesc;
  for (int e = threadIdx.x; e < total; e += 256) {
    const int h = e / kDesc, k = e - h * kDesc;
    const int c = k / 49, t = k - c * 49, dy = t / 7, dx = t - dy * 7;
    const int cy = min(max(pp[2 * h], 3), S - 4), cx = min(max(pp[2 * h + 1], 3), S - 4);
    const float v = src[((long long)c * S + (cy + dy - 3)) * S + (cx + dx - 3)];
    dst[e] = v;
    const double d = (double)v;
    if (c == 0) { s[0] += d; q[0] += d * d; }
    else if (c == 1) { s[1] += d; q[1] += d * d; }
    else { s[2] += d; q[2] += d * d; }
  }
  double v6[6] = {s[0], s[1], s[2], q[0], q[1], q[2]};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v6[k] += __shfl_xor(v6[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[threadIdx.x >> 6][k] = v6[k];
  }
  __syncthreads();
  if (threadIdx.x < 6)
    partials[(long long)img * 6 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// (images, 6) partials -> mean[3], std[3] (population), one workgroup, fixed order
__global__ __launch_bounds__(256) void swd_stats_kernel(const double* __restrict__ partials, long long images,
                                                        double per_image, double* __restrict__ out) {
  __shared__ double red[4][6];
  double v6[6] = {0., 0., 0., 0., 0., 0.};
  for (long long i = threadIdx.x; i < images; i += 256) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v6[k] += partials[i * 6 + k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v6[k] += __shfl_xor(v6[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[threadIdx.x >> 6][k] = v6[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    const double cnt = per_image * (double)images;
    const double sum = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    const double sq = (red[0][c + 3] + red[1][c + 3]) + (red[2][c + 3] + red[3][c + 3]);
    const double mean = sum / cnt;
    const double var = fmax(sq / cnt - mean * mean, 0.0);
    out[c] = mean;
    out[3 + c] = sqrt(var);
  }
}

// ---- projection -----------------------------------------------------------------------------------------------------------
// rows [r0, r0 + rows) of a row-major (*, 147) matrix -> LDS [rows_cap][148], column 147 and the rows past `count` zero;
// mean / std (nullptr: none) normalise per channel on the way in.  A zero std divides by zero on purpose: the level is NaN.
__device__ __forceinline__ void swd_stage(float* __restrict__ lds, const float* __restrict__ src, long long r0, long long count,
                                          int rows_cap, const float* mean, const float* stdv) {
  const long long avail = count - r0;
  const int rows = (int)(avail < (long long)rows_cap ? (avail > 0 ? avail : 0) : rows_cap);
  const float* base = src + r0 * kDesc;
  const int total = rows * kDesc;
  for (int e = threadIdx.x; e < total; e += 256) {
    const int m = e / kDesc, k = e - m * kDesc;
    float v = base[e];
    if (mean != nullptr) {
      const int c = k / 49;
      v = (v - mean[c]) / stdv[c];
    }
    lds[m * kKPad + k] = v;
  }
  for (int m = threadIdx.x; m < rows; m += 256) lds[m * kKPad + kDesc] = 0.f;
  const int rest = (rows_cap - rows) * kKPad;
  for (int e = threadIdx.x; e < rest; e += 256) lds[rows * kKPad + e] = 0.f;
}

// Workgroup = 4 waves; blockIdx.y picks 128 directions (staged once), the workgroup then walks 64-descriptor tiles with stride
// gridDim.x.  Wave w owns descriptors 16w .. 16w + 15 of the tile and all 128 directions: 8 independent accumulators.  MFMA
// operands (cdna_hip_programming.md): A[i = l & 15][k = l >> 4] = descriptor row, B[k = l >> 4][j = l & 15] = direction;
// D: lane holds column j = l & 15 (direction) and rows i = 4 (l >> 4) + r (4 consecutive descriptors: one 16-byte store
// into the transposed (D, M) output).
__global__ __launch_bounds__(256) void swd_project_kernel(const float* __restrict__ desc, const float* __restrict__ dirs,
                                                          const double* __restrict__ stats, float* __restrict__ out,
                                                          long long M, int D) {
  extern __shared__ float lds[];
  float* sB = lds;                             // [128][148] directions
  float* sA = lds + kTileD * kKPad;            // [64][148] normalised descriptors
  __shared__ float nrm[6];
  if (threadIdx.x < 6) nrm[threadIdx.x] = (float)stats[threadIdx.x];
  const int d0 = blockIdx.y * kTileD;
  swd_stage(sB, dirs, d0, D, kTileD, nullptr, nullptr);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const long long tiles = (M + kTileM - 1) / kTileM;
  const bool vec = (M & 3) == 0;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long m0 = t * kTileM;
    swd_stage(sA, desc, m0, M, kTileM, nrm, nrm + 3);
    __syncthreads();
    f32x4 acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* pa = sA + (wave * 16 + li) * kKPad + lk;
    const float* pb = sB + li * kKPad + lk;
#pragma unroll 4
    for (int ks = 0; ks < kKPad / 4; ++ks) {
      const float a = pa[4 * ks];
#pragma unroll
      for (int c = 0; c < 8; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pb[c * 16 * kKPad + 4 * ks], acc[c], 0, 0, 0);
    }
    const long long m = m0 + wave * 16 + lk * 4;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int d = d0 + c * 16 + li;
      if (d >= D) continue;
      float* o = out + (long long)d * M + m;
      if (vec && m + 3 < M) {
        *reinterpret_cast<float4*>(o) = float4{acc[c][0], acc[c][1], acc[c][2], acc[c][3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (m + r < M) o[r] = acc[c][r];
      }
    }
    __syncthreads();
  }
}

// ---- sort -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swd_offsets_kernel(unsigned int* __restrict__ off, int segments, long long M) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= segments) off[i] = (unsigned int)((long long)i * M);
}

// Segments at least this long are sorted one after the other by the device-wide radix sort (every CU works on one segment);
// shorter ones by the segmented sort (one workgroup per segment).
constexpr long long kSortWide = 1 << 16;

size_t swd_align(size_t v) { return (v + 255) & ~(size_t)255; }

size_t swd_sort_temp(int segments, long long M) {
  size_t bytes = 0;
  float* none = nullptr;
  if (M >= kSortWide) {
    if (rocprim::radix_sort_keys(nullptr, bytes, none, none, (size_t)M) != hipSuccess) return 0;
  } else {
    unsigned int* off = nullptr;
    if (rocprim::segmented_radix_sort_keys(nullptr, bytes, none, none, (unsigned int)(segments * M), (unsigned int)segments, off,
                                           off + 1) != hipSuccess)
      return 0;
  }
  return swd_align(bytes ? bytes : 1);
}

// ---- distance -------------------------------------------------------------------------------------------------------------
constexpr int kDistPer = 256 * 16;      // elements per workgroup pass

__host__ __device__ inline int swd_dist_chunks(long long M) {
  const long long c = (M + kDistPer - 1) / kDistPer;
  return (int)(c < 64 ? c : 64);
}

__global__ __launch_bounds__(256) void swd_dist_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       double* __restrict__ part, long long M) {
  __shared__ double red[4];
  const int chunks = gridDim.x;
  const long long base = (long long)blockIdx.y * M;
  double s = 0.;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)chunks * 256)
    s += fabs((double)a[base + i] - (double)b[base + i]);
  s = gl_block_sum_256d(s, red);
  if (threadIdx.x == 0) part[(long long)blockIdx.y * chunks + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void swd_dist_finish_kernel(const double* __restrict__ part, long long count, double denom,
                                                              double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.;
  for (long long i = threadIdx.x; i < count; i += 256) s += part[i];
  s = gl_block_sum_256d(s, red);
  if (threadIdx.x == 0) out[0] = s / denom;
}

// ---- draws ----------------------------------------------------------------------------------------------------------------
// centres: image i uses counters offset + i * ceil(2n / 4) ..; word e of its (n, 2) row block -> 3 + floor(u (S - 6))
__global__ __launch_bounds__(256) void swd_positions_kernel(int* __restrict__ out, int N, int n, int S, uint64_t seed,
                                                            uint64_t offset) {
  const int per = (2 * n + 3) / 4;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)N * per) return;
  const int img = (int)(g / per), w4 = (int)(g - (long long)img * per);
  const uint64_t ctr = offset + (uint64_t)g;
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = 4 * w4 + k;
    if (e < 2 * n) out[(long long)img * 2 * n + e] = 3 + (int)(((uint64_t)(c[k] >> 8) * (uint64_t)(S - 6)) >> 24);
  }
}

// directions: one wave per direction; element e of direction d is the Box-Muller cosine of words 0, 1 of counter
// offset + 147 d + e (fp64, like the ADA draw), the row then scaled to unit L2 norm
__global__ __launch_bounds__(64) void swd_directions_kernel(float* __restrict__ out, int D, uint64_t seed, uint64_t offset) {
  const int d = blockIdx.x, lane = threadIdx.x;
  const double two24 = 1.0 / 16777216.0, pi = 3.14159265358979323846;
  double z[3] = {0., 0., 0.}, ss = 0.;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = lane + 64 * k;
    if (e < kDesc) {
      const uint64_t ctr = offset + (uint64_t)d * kDesc + e;
      uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
      philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
      const double r = sqrt(-2.0 * log((double)((c[0] >> 8) + 1u) * two24));
      z[k] = r * cos(2.0 * pi * (double)(c[1] >> 8) * two24);
      ss += z[k] * z[k];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const double inv = 1.0 / sqrt(ss);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = lane + 64 * k;
    if (e < kDesc) out[(long long)d * kDesc + e] = (float)(z[k] * inv);
  }
}

bool swd_plane_ok(long long planes, int H, int W) {
  return planes > 0 && H >= 4 && W >= 4 && !(H & 1) && !(W & 1) && H <= 16384 && W <= 16384 &&
         planes * H * W / 256 < 0x7fffffffLL;
}

}  // namespace

extern "C" {

int ganlab_swd_down_f32(const float* x, float* y, long long planes, int H, int W, void* stream) {
  if (!x || !y || !swd_plane_ok(planes, H, W)) return GANLAB_EINVAL;
  const long long total = planes * (H / 2) * (W / 2);
  GL_LAUNCH(swd_down_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, gl_stream(stream), x, y, planes, H, W);
  return GL_CHECK_LAUNCH();
}

int ganlab_swd_band_f32(const float* g0, const float* g1, float* out, long long planes, int H, int W, void* stream) {
  if (!g0 || !g1 || !out || !swd_plane_ok(planes, H, W)) return GANLAB_EINVAL;
  const long long total = planes * H * W;
  GL_LAUNCH(swd_band_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, gl_stream(stream), g0, g1, out, planes, H, W);
  return GL_CHECK_LAUNCH();
}

int ganlab_swd_gather_f32(const float* band, const int* pos, float* desc, double* partials, int N, int n, int S, void* stream) {
  if (!band || !pos || !desc || !partials || N <= 0 || n <= 0 || S < 7 || S > 16384 || (long long)n * kDesc > 0x7fffffffLL)
    return GANLAB_EINVAL;
  GL_LAUNCH(swd_gather_kernel, dim3(N), dim3(256), 0, gl_stream(stream), band, pos, desc, partials, n, S);
  return GL_CHECK_LAUNCH();
}

int ganlab_swd_stats_f64(const double* partials, long long images, long long per_image, double* out, void* stream) {
  if (!partials || !out || images <= 0 || per_image <= 0) return GANLAB_EINVAL;
  GL_LAUNCH(swd_stats_kernel, dim3(1), dim3(256), 0, gl_stream(stream), partials, images, (double)per_image, out);
  return GL_CHECK_LAUNCH();
}

int ganlab_swd_project_f32(const float* desc, const float* dirs, const double* stats, float* out, long long M, int D,
                           void* stream) {
  if (!desc || !dirs || !stats || !out || M <= 0 || D <= 0) return GANLAB_EINVAL;
  const size_t lds = (size_t)(kTileD + kTileM) * kKPad * sizeof(float);
  static const bool raised = hipFuncSetAttribute(reinterpret_cast<const void*>(swd_project_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
  if (!raised) return GANLAB_ELAUNCH;
  const long long tiles = (M + kTileM - 1) / kTileM;
  const int dchunks = (D + kTileD - 1) / kTileD;
  const long long want = 512 / dchunks > 0 ? 512 / dchunks : 1;
  GL_LAUNCH(swd_project_kernel, dim3((unsigned)(tiles < want ? tiles : want), dchunks), dim3(256), lds, gl_stream(stream), desc,
            dirs, stats, out, M, D);
  return GL_CHECK_LAUNCH();
}

size_t ganlab_swd_sort_workspace(int segments, long long M) {
  if (segments <= 0 || M <= 0 || (long long)segments * M >= 0xffffffffLL) return 0;
  const size_t temp = swd_sort_temp(segments, M);
  return temp ? temp + swd_align((size_t)(segments + 1) * sizeof(unsigned int)) : 0;
}

int ganlab_swd_sort_f32(const float* in, float* out, int segments, long long M, void* workspace, size_t workspace_bytes,
                        void* stream) {
  if (!in || !out || in == out || !workspace || segments <= 0 || M <= 0 || (long long)segments * M >= 0xffffffffLL)
    return GANLAB_EINVAL;
  const size_t temp = swd_sort_temp(segments, M);
  if (!temp) return GANLAB_EUNSUPPORTED;
  if (workspace_bytes < temp + swd_align((size_t)(segments + 1) * sizeof(unsigned int))) return GANLAB_EWORKSPACE;
  hipStream_t st = gl_stream(stream);
  size_t bytes = temp;
  if (M >= kSortWide) {
    for (int s = 0; s < segments; ++s)
      if (rocprim::radix_sort_keys(workspace, bytes, in + (long long)s * M, out + (long long)s * M, (size_t)M, 0, 32, st) !=
          hipSuccess)
        return GANLAB_ELAUNCH;
    return GANLAB_OK;
  }
  unsigned int* off = reinterpret_cast<unsigned int*>(static_cast<char*>(workspace) + temp);
  GL_LAUNCH(swd_offsets_kernel, dim3((segments + 256) / 256), dim3(256), 0, st, off, segments, M);
  if (GL_CHECK_LAUNCH() != GANLAB_OK) return GANLAB_ELAUNCH;
  if (rocprim::segmented_radix_sort_keys(workspace, bytes, in, out, (unsigned int)(segments * M), (unsigned int)segments, off,
                                         off + 1, 0, 32, st) != hipSuccess)
    return GANLAB_ELAUNCH;
  return GANLAB_OK;
}

size_t ganlab_swd_distance_workspace(int D, long long M) {
  if (D <= 0 || M <= 0) return 0;
  return (size_t)D * swd_dist_chunks(M) * sizeof(double);
}

int ganlab_swd_distance_f64(const float* a, const float* b, double* out, int D, long long M, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!a || !b || !out || !workspace || D <= 0 || D > 65535 || M <= 0) return GANLAB_EINVAL;
  const int chunks = swd_dist_chunks(M);
  if (workspace_bytes < (size_t)D * chunks * sizeof(double)) return GANLAB_EWORKSPACE;
  double* part = reinterpret_cast<double*>(workspace);
  GL_LAUNCH(swd_dist_kernel, dim3(chunks, D), dim3(256), 0, gl_stream(stream), a, b, part, M);
  GL_LAUNCH(swd_dist_finish_kernel, dim3(1), dim3(256), 0, gl_stream(stream), part, (long long)D * chunks,
            (double)D * (double)M, out);
  return GL_CHECK_LAUNCH();
}

int ganlab_swd_positions_i32(int* out, int N, int n, int S, uint64_t seed, uint64_t offset, void* stream) {
  if (!out || N <= 0 || n <= 0 || S < 7 || S > 16384) return GANLAB_EINVAL;
  const long long total = (long long)N * ((2 * n + 3) / 4);
  GL_LAUNCH(swd_positions_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, gl_stream(stream), out, N, n, S, seed,
            offset);
  return GL_CHECK_LAUNCH();
}

int ganlab_swd_directions_f32(float* out, int D, uint64_t seed, uint64_t offset, void* stream) {
  if (!out || D <= 0) return GANLAB_EINVAL;
  GL_LAUNCH(swd_directions_kernel, dim3(D), dim3(64), 0, gl_stream(stream), out, D, seed, offset);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
