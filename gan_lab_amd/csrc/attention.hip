// SAGAN self-attention core (Zhang et al. 2019) on the exact-fp32 MFMA, flash style: nothing of size L x S reaches memory.
// Operands are channel-major, as the 1x1 convolutions leave them: q (N, Dk, L), k (N, Dk, S), v (N, Dv, S); no 1/sqrt(d).
//   P[n,l,:] = softmax_s(sum_d q[n,d,l] k[n,d,s]) ; o[n,c,l] = sum_s v[n,c,s] P[n,l,s] ; lse[n,l] = logsumexp_s
// Every product runs on v_mfma_f32_32x32x2_f32 (lane L supplies A[i = L & 31][kk = L >> 5] and B[kk = L >> 5][j = L & 31]; the
// result sits at column j = L & 31, rows at_row(r, L >> 5) of register r).  A wave owns 32 queries (forward, dq) or 32 keys
// (dk / dv) and always keeps ITS index in the column j, so the per-query softmax statistics are per-lane scalars:
//   forward  S^T[s][l] = K^T Q   -> the online max / sum of query l live in lanes (l, l + 32), joined by one xor-32 shuffle;
//            O[c][l]  += V P^T   -> the result registers of S^T are fed back as the B operand unchanged: register r of the
//                                   two lane halves holds keys at_row(r, 0) and at_row(r, 1), so MFMA step r contracts exactly
//                                   those two keys and the A operand reads V at the same two columns (a permuted k order,
//                                   no shuffles, no LDS round trip for P).
//   dq       S^T and dP^T[s][l] = V^T dO, dS^T = P^T o (dP^T - D[l]), dQ[d][l] += K dS^T           (parallel over query tiles)
//   dk, dv   S[l][s] = Q^T K, dP[l][s] = dO^T V, dK[d][s] += Q dS, dV[c][s] += dO P                (parallel over key tiles)
// with D[n,l] = sum_c dO[n,c,l] o[n,c,l] from a small kernel in front.  No atomics: every output element is owned by one
// lane and summed in a fixed order (key tiles, resp. query tiles, ascending), so results are bitwise reproducible.
// LDS tiles are [row][33]: the MFMA A operand is read either along a row (lanes walk the 32 columns) or down a column
// (lanes walk 32 rows at stride 33), both conflict free.  Tails in L, S, Dk, Dv are zero-filled on load and masked on store;
// keys past S get the logit -inf (forward, dq), queries past L the statistic lse = +inf (dk / dv), so their P is exactly 0.
// Also here: the block's 2x2 max pool with a packed 2-bit argmax, and the gated residual out = x + gamma * y.
#include "common.h"
#include <math.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int AT_LD = 33;                     // LDS row stride of a 32-column tile
constexpr int AT_WAVES = 4;                   // waves per workgroup, each owning 32 queries (keys)
constexpr int AT_BLOCK = AT_WAVES * 32;       // queries (keys) per workgroup

__device__ __forceinline__ f32x16 at_mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of result register r in lane half h
__device__ __forceinline__ int at_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// LDS tile [rows_pad][AT_LD] <- src[row][c0 .. c0 + 32) of a (rows_valid, len) row-major matrix; zero outside
__device__ __forceinline__ void at_load_tile(float* lds, const float* __restrict__ src, int rows_valid, int rows_pad, int len,
                                             int c0) {
  for (int idx = threadIdx.x; idx < rows_pad * 32; idx += 256) {
    const int r = idx >> 5, c = idx & 31;
    float v = 0.f;
    if (r < rows_valid && c0 + c < len) v = src[(long long)r * len + c0 + c];
    lds[r * AT_LD + c] = v;
  }
}

// registers of the B operand of a (row-pair per step) product: src[2 * step + h][col], zero outside
template <int STEPS>
__device__ __forceinline__ void at_load_regs(float (&reg)[STEPS], const float* __restrict__ src, int rows, int len, int col,
                                             int h) {
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int r = 2 * st + h;
    reg[st] = (r < rows && col < len) ? src[(long long)r * len + col] : 0.f;
  }
}

__device__ __forceinline__ f32x16 at_zero() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// C[i][j] = sum_r rowmat[r][i] * reg[r][j]: the A operand walks a tile row (i = lane & 31), rows r < rows
template <int STEPS>
__device__ __forceinline__ f32x16 at_rows_dot(const float* lds, const float (&reg)[STEPS], int rows, int j, int h) {
  f32x16 c = at_zero();
#pragma unroll
  for (int st = 0; st < STEPS; ++st)
    if (2 * st < rows) c = at_mfma(lds[(2 * st + h) * AT_LD + j], reg[st], c);
  return c;
}

// acc[t][i][j] += sum_x lds[t * 32 + i][x] * b[x][j], x over the tile's 32 columns in the result-register order of b
template <int T>
__device__ __forceinline__ void at_cols_acc(f32x16 (&acc)[T], const float* lds, const f32x16& b, int rows, int j, int h) {
#pragma unroll
  for (int t = 0; t < T; ++t)
    if (t * 32 < rows) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t] = at_mfma(lds[(t * 32 + j) * AT_LD + at_row(r, h)], b[r], acc[t]);
    }
}

// dst[t * 32 + row][col] = acc * mul for rows < rows, col < len
template <int T>
__device__ __forceinline__ void at_store(float* __restrict__ dst, const f32x16 (&acc)[T], int rows, int len, int col, int h,
                                         float mul) {
  if (col >= len) return;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = t * 32 + at_row(r, h);
      if (row < rows) dst[(long long)row * len + col] = acc[t][r] * mul;
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int KT, int NT>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, float* __restrict__ o,
                                                       float* __restrict__ lse, int Dk, int Dv, int L, int S, int tiles) {
  __shared__ float ks[KT * 32 * AT_LD];
  __shared__ float vs[NT * 32 * AT_LD];
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int l = tile * AT_BLOCK + wave * 32 + j;
  const bool wave_on = tile * AT_BLOCK + wave * 32 < L;
  q += (long long)n * Dk * L;
  k += (long long)n * Dk * S;
  v += (long long)n * Dv * S;
  float qr[KT * 16];
  at_load_regs(qr, q, Dk, L, l, h);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = at_zero();
  float m = -INFINITY, sum = 0.f;
  for (int s0 = 0; s0 < S; s0 += 32) {
    __syncthreads();
    at_load_tile(ks, k, Dk, Dk, S, s0);
    at_load_tile(vs, v, Dv, (Dv + 31) & ~31, S, s0);
    __syncthreads();
    if (!wave_on) continue;
    f32x16 st = at_rows_dot(ks, qr, Dk, j, h);             // S^T[s = at_row(r, h)][l = j]
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (s0 + at_row(r, h) >= S) st[r] = -INFINITY;
      tmax = fmaxf(tmax, st[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax);                    // finite: key s0 of every tile is valid
    const float scale = expf(m - m_new);                   // first tile: exp(-inf) = 0
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = expf(st[r] - m_new);
      rs += st[r];
    }
    rs += __shfl_xor(rs, 32, 64);
    sum = sum * scale + rs;
    m = m_new;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] *= scale;
    at_cols_acc(acc, vs, st, Dv, j, h);                    // O[c][l] += sum_s V[c][s] P^T[s][l]
  }
  if (!wave_on) return;
  at_store(o + (long long)n * Dv * L, acc, Dv, L, l, h, 1.f / sum);
  if (h == 0 && l < L) lse[(long long)n * L + l] = m + logf(sum);
}

// ---- D[n, l] = sum_c dO[n, c, l] o[n, c, l] -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_bwd_d_kernel(const float* __restrict__ dO, const float* __restrict__ o,
                                                         float* __restrict__ dw, int Dv, int L, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long n = idx / L;
  const int l = (int)(idx - n * L);
  const long long base = n * Dv * L + l;
  float a = 0.f;
  for (int c = 0; c < Dv; ++c) a += dO[base + (long long)c * L] * o[base + (long long)c * L];
  dw[idx] = a;
}

// ---- dq: parallel over query tiles ----------------------------------------------------------------------------------------------
template <int KT, int NT>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                          const float* __restrict__ v, const float* __restrict__ lse,
                                                          const float* __restrict__ dO, const float* __restrict__ dw,
                                                          float* __restrict__ dq, int Dk, int Dv, int L, int S, int tiles) {
  __shared__ float ks[KT * 32 * AT_LD];
  __shared__ float vs[NT * 32 * AT_LD];
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int l = tile * AT_BLOCK + wave * 32 + j;
  const bool wave_on = tile * AT_BLOCK + wave * 32 < L;
  q += (long long)n * Dk * L;
  k += (long long)n * Dk * S;
  v += (long long)n * Dv * S;
  dO += (long long)n * Dv * L;
  float qr[KT * 16], dor[NT * 16];
  at_load_regs(qr, q, Dk, L, l, h);
  at_load_regs(dor, dO, Dv, L, l, h);
  const float lse_l = l < L ? lse[(long long)n * L + l] : 0.f;
  const float d_l = l < L ? dw[(long long)n * L + l] : 0.f;
  f32x16 acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) acc[t] = at_zero();
  for (int s0 = 0; s0 < S; s0 += 32) {
    __syncthreads();
    at_load_tile(ks, k, Dk, (Dk + 31) & ~31, S, s0);
    at_load_tile(vs, v, Dv, Dv, S, s0);
    __syncthreads();
    if (!wave_on) continue;
    const f32x16 st = at_rows_dot(ks, qr, Dk, j, h);       // S^T[s][l]
    const f32x16 dp = at_rows_dot(vs, dor, Dv, j, h);      // dP^T[s][l] = sum_c V[c][s] dO[c][l]
    f32x16 ds;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = s0 + at_row(r, h) < S ? expf(st[r] - lse_l) : 0.f;
      ds[r] = p * (dp[r] - d_l);
    }
    at_cols_acc(acc, ks, ds, Dk, j, h);                    // dQ[d][l] += sum_s K[d][s] dS^T[s][l]
  }
  if (!wave_on) return;
  at_store(dq + (long long)n * Dk * L, acc, Dk, L, l, h, 1.f);
}

// ---- dk, dv: parallel over key tiles --------------------------------------------------------------------------------------------
template <int KT, int NT>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ lse,
                                                           const float* __restrict__ dO, const float* __restrict__ dw,
                                                           float* __restrict__ dk, float* __restrict__ dv, int Dk, int Dv,
                                                           int L, int S, int tiles) {
  __shared__ float qs[KT * 32 * AT_LD];
  __shared__ float dos[NT * 32 * AT_LD];
  __shared__ float lses[32];
  __shared__ float dws[32];
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int s = tile * AT_BLOCK + wave * 32 + j;
  const bool wave_on = tile * AT_BLOCK + wave * 32 < S;
  q += (long long)n * Dk * L;
  k += (long long)n * Dk * S;
  v += (long long)n * Dv * S;
  dO += (long long)n * Dv * L;
  lse += (long long)n * L;
  dw += (long long)n * L;
  float kr[KT * 16], vr[NT * 16];
  at_load_regs(kr, k, Dk, S, s, h);
  at_load_regs(vr, v, Dv, S, s, h);
  f32x16 dka[KT], dva[NT];
#pragma unroll
  for (int t = 0; t < KT; ++t) dka[t] = at_zero();
#pragma unroll
  for (int t = 0; t < NT; ++t) dva[t] = at_zero();
  for (int l0 = 0; l0 < L; l0 += 32) {
    __syncthreads();
    at_load_tile(qs, q, Dk, (Dk + 31) & ~31, L, l0);
    at_load_tile(dos, dO, Dv, (Dv + 31) & ~31, L, l0);
    if (threadIdx.x < 32) {
      const bool in = l0 + (int)threadIdx.x < L;
      lses[threadIdx.x] = in ? lse[l0 + threadIdx.x] : INFINITY;      // P of a query past L: exp(-inf) = 0
      dws[threadIdx.x] = in ? dw[l0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    if (!wave_on) continue;
    const f32x16 st = at_rows_dot(qs, kr, Dk, j, h);       // S[l = at_row(r, h)][s = j]
    const f32x16 dp = at_rows_dot(dos, vr, Dv, j, h);      // dP[l][s] = sum_c dO[c][l] V[c][s]
    f32x16 p, ds;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = at_row(r, h);
      p[r] = expf(st[r] - lses[lr]);
      ds[r] = p[r] * (dp[r] - dws[lr]);
    }
    at_cols_acc(dka, qs, ds, Dk, j, h);                    // dK[d][s] += sum_l Q[d][l] dS[l][s]
    at_cols_acc(dva, dos, p, Dv, j, h);                    // dV[c][s] += sum_l dO[c][l] P[l][s]
  }
  if (!wave_on) return;
  at_store(dk + (long long)n * Dk * S, dka, Dk, S, s, h, 1.f);
  at_store(dv + (long long)n * Dv * S, dva, Dv, S, s, h, 1.f);
}

long long at_grid(int N, int len) { return (long long)N * ((len + AT_BLOCK - 1) / AT_BLOCK); }

bool at_supported(int N, int Dk, int Dv, int L, int S) {
  if (N < 1 || L < 1 || S < 1) return false;
  if (Dk < 4 || Dk > 64 || (Dk & 3)) return false;
  if (Dv < 16 || Dv > 256 || (Dv & 15)) return false;
  return at_grid(N, L) <= 0x7fffffffLL && at_grid(N, S) <= 0x7fffffffLL && ((long long)N * L + 255) / 256 <= 0x7fffffffLL;
}

// the kernel instance for (Dk, Dv): KT = tiles of 32 over Dk (1, 2), NT = tiles of 32 over Dv rounded up to 1, 2, 4, 8
#define AT_DISPATCH(CALL)                                      \
  do {                                                         \
    const int nt_ = (Dv + 31) / 32;                            \
    if (Dk <= 32) {                                            \
      if (nt_ <= 1) { CALL(1, 1); }                            \
      else if (nt_ <= 2) { CALL(1, 2); }                       \
      else if (nt_ <= 4) { CALL(1, 4); }                       \
      else { CALL(1, 8); }                                     \
    } else {                                                   \
      if (nt_ <= 1) { CALL(2, 1); }                            \
      else if (nt_ <= 2) { CALL(2, 2); }                       \
      else if (nt_ <= 4) { CALL(2, 4); }                       \
      else { CALL(2, 8); }                                     \
    }                                                          \
  } while (0)

// ---- 2x2 max pool with a packed 2-bit argmax ------------------------------------------------------------------------------------
// one thread = 4 consecutive outputs (flat index over planes x Ho x Wo) = one byte of argmax codes (2 * dy + dx, first maximum
// in row-major order, a NaN wins like in ATen)
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         unsigned char* __restrict__ bits, long long total, int Ho, int Wo) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g * 4 >= total) return;
  unsigned code = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long oi = g * 4 + e;
    if (oi >= total) break;
    const int ox = (int)(oi % Wo);
    const long long t = oi / Wo;
    const int oy = (int)(t % Ho);
    const long long plane = t / Ho;
    const float* p = x + (plane * 2 * Ho + 2 * oy) * (2LL * Wo) + 2 * ox;
    const float c[4] = {p[0], p[1], p[2 * Wo], p[2 * Wo + 1]};
    float best = c[0];
    unsigned arg = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (c[i] > best || c[i] != c[i]) { best = c[i]; arg = i; }
    y[oi] = best;
    code |= arg << (2 * e);
  }
  bits[g] = (unsigned char)code;
}

// gather: every input element reads its output's code
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const float* __restrict__ gy, const unsigned char* __restrict__ bits,
                                                             float* __restrict__ gx, long long total_in, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total_in) return;
  const int W = 2 * Wo;
  const int ix = (int)(i % W);
  const long long t = i / W;
  const int iy = (int)(t % (2 * Ho));
  const long long plane = t / (2 * Ho);
  const long long oi = (plane * Ho + (iy >> 1)) * Wo + (ix >> 1);
  const unsigned arg = (bits[oi >> 2] >> (2 * (int)(oi & 3))) & 3u;
  gx[i] = arg == (unsigned)((iy & 1) * 2 + (ix & 1)) ? gy[oi] : 0.f;
}

// ---- gated residual ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gated_residual_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ gamma, float* __restrict__ out,
                                                             long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = x[i] + gamma[0] * y[i];
}

constexpr int DOT_CHUNK = 4096;     // elements per block of the first stage
constexpr int DOT_MAX_BLOCKS = 1024;

int dot_blocks(long long n) {
  const long long b = (n + DOT_CHUNK - 1) / DOT_CHUNK;
  return (int)(b < 1 ? 1 : (b > DOT_MAX_BLOCKS ? DOT_MAX_BLOCKS : b));
}

__global__ __launch_bounds__(256) void dot_stage1(const float* __restrict__ a, const float* __restrict__ b,
                                                  double* __restrict__ part, long long n) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    acc += (double)a[i] * (double)b[i];
  acc = gl_block_sum_256d(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void dot_stage2(const double* __restrict__ part, float* __restrict__ out, int nb) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
  acc = gl_block_sum_256d(acc, red);
  if (threadIdx.x == 0) out[0] = (float)acc;
}

unsigned ew_grid(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

int ganlab_attn_supported(int N, int Dk, int Dv, int L, int S) { return at_supported(N, Dk, Dv, L, S) ? 1 : 0; }

int ganlab_attn_fwd_f32(const float* q, const float* k, const float* v, float* o, float* lse, int N, int Dk, int Dv, int L,
                        int S, void* stream) {
  if (!q || !k || !v || !o || !lse) return GANLAB_EINVAL;
  if (N < 1 || Dk < 1 || Dv < 1 || L < 1 || S < 1) return GANLAB_EINVAL;
  if (!at_supported(N, Dk, Dv, L, S)) return GANLAB_EUNSUPPORTED;
  hipStream_t st = gl_stream(stream);
  const int tiles = (L + AT_BLOCK - 1) / AT_BLOCK;
#define AT_FWD(KT, NT) \
  GL_LAUNCH((attn_fwd_kernel<KT, NT>), dim3((unsigned)at_grid(N, L)), dim3(256), 0, st, q, k, v, o, lse, Dk, Dv, L, S, tiles)
  AT_DISPATCH(AT_FWD);
#undef AT_FWD
  return GL_CHECK_LAUNCH();
}

size_t ganlab_attn_bwd_workspace(int N, int L) { return N > 0 && L > 0 ? (size_t)N * L * sizeof(float) : 0; }

int ganlab_attn_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* d_o,
                        float* dq, float* dk, float* dv, int N, int Dk, int Dv, int L, int S, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (!q || !k || !v || !o || !lse || !d_o || !dq || !dk || !dv) return GANLAB_EINVAL;
  if (N < 1 || Dk < 1 || Dv < 1 || L < 1 || S < 1) return GANLAB_EINVAL;
  if (!at_supported(N, Dk, Dv, L, S)) return GANLAB_EUNSUPPORTED;
  if (!workspace || workspace_bytes < ganlab_attn_bwd_workspace(N, L)) return GANLAB_EWORKSPACE;
  hipStream_t st = gl_stream(stream);
  float* dw = (float*)workspace;
  const long long rows = (long long)N * L;
  GL_LAUNCH(attn_bwd_d_kernel, dim3(ew_grid(rows)), dim3(256), 0, st, d_o, o, dw, Dv, L, rows);
  const int ltiles = (L + AT_BLOCK - 1) / AT_BLOCK, stiles = (S + AT_BLOCK - 1) / AT_BLOCK;
#define AT_DQ(KT, NT)                                                                                                   \
  GL_LAUNCH((attn_bwd_dq_kernel<KT, NT>), dim3((unsigned)at_grid(N, L)), dim3(256), 0, st, q, k, v, lse, d_o, dw, dq, Dk, \
            Dv, L, S, ltiles)
  AT_DISPATCH(AT_DQ);
#undef AT_DQ
#define AT_DKV(KT, NT)                                                                                                       \
  GL_LAUNCH((attn_bwd_dkv_kernel<KT, NT>), dim3((unsigned)at_grid(N, S)), dim3(256), 0, st, q, k, v, lse, d_o, dw, dk, dv, Dk, \
            Dv, L, S, stiles)
  AT_DISPATCH(AT_DKV);
#undef AT_DKV
  return GL_CHECK_LAUNCH();
}

size_t ganlab_maxpool2x2_bits_bytes(long long planes, int H, int W) {
  if (planes <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)((planes * (H / 2) * (W / 2) + 3) / 4);
}

int ganlab_maxpool2x2_f32(const float* x, float* y, void* bits, long long planes, int H, int W, void* stream) {
  if (!x || !y || !bits || planes <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return GANLAB_EINVAL;
  const long long total = planes * (H / 2) * (W / 2);
  const long long groups = (total + 3) / 4;
  if ((groups + 255) / 256 > 0x7fffffffLL) return GANLAB_EINVAL;
  GL_LAUNCH(maxpool2x2_kernel, dim3(ew_grid(groups)), dim3(256), 0, gl_stream(stream), x, y, (unsigned char*)bits, total,
            H / 2, W / 2);
  return GL_CHECK_LAUNCH();
}

int ganlab_maxpool2x2_bwd_f32(const float* gy, const void* bits, float* gx, long long planes, int H, int W, void* stream) {
  if (!gy || !gx || !bits || planes <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return GANLAB_EINVAL;
  const long long total = planes * H * W;
  if ((total + 255) / 256 > 0x7fffffffLL) return GANLAB_EINVAL;
  GL_LAUNCH(maxpool2x2_bwd_kernel, dim3(ew_grid(total)), dim3(256), 0, gl_stream(stream), gy, (const unsigned char*)bits, gx,
            total, H / 2, W / 2);
  return GL_CHECK_LAUNCH();
}

int ganlab_gated_residual_f32(const float* x, const float* y, const float* gamma, float* out, long long n, void* stream) {
  if (!x || !y || !gamma || !out || n <= 0 || (n + 255) / 256 > 0x7fffffffLL) return GANLAB_EINVAL;
  GL_LAUNCH(gated_residual_kernel, dim3(ew_grid(n)), dim3(256), 0, gl_stream(stream), x, y, gamma, out, n);
  return GL_CHECK_LAUNCH();
}

size_t ganlab_dot_workspace(long long n) { return n > 0 ? (size_t)dot_blocks(n) * sizeof(double) : 0; }

int ganlab_dot_f32(const float* a, const float* b, float* out, long long n, void* workspace, size_t workspace_bytes,
                   void* stream) {
  if (!a || !b || !out || n <= 0) return GANLAB_EINVAL;
  const int nb = dot_blocks(n);
  if (!workspace || workspace_bytes < (size_t)nb * sizeof(double)) return GANLAB_EWORKSPACE;
  hipStream_t st = gl_stream(stream);
  GL_LAUNCH(dot_stage1, dim3(nb), dim3(256), 0, st, a, b, (double*)workspace, n);
  GL_LAUNCH(dot_stage2, dim3(1), dim3(256), 0, st, (const double*)workspace, out, nb);
  return GL_CHECK_LAUNCH();
}

}  // extern "C"
