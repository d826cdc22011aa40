// The plane pass of the per-sample BatchNorm backwards (cond.hip: class-conditional; hier.hip: modulated): it needs neither the
// labels nor the per-sample affine, so both families share it.
#pragma once
#include "common.h"

namespace {

// one wave per (n, c) plane, four planes per workgroup: part[plane] = {sum gz, sum gz * xhat} (fp64 from the lane accumulator
// on); with yact (the output of the fused activation) gz = gy * lrelu'(yact) is also stored for the apply pass
template <bool VEC4>
__global__ __launch_bounds__(256) void cbn_bwd_planes_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ yact, float* __restrict__ gz,
                                                             double* __restrict__ part, long long planes, int C, long long HW,
                                                             float slope) {
  const long long plane = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (plane >= planes) return;
  const int lane = threadIdx.x & 63;
  const int c = (int)(plane % C);
  const float mu = mean[c], rs = rstd[c];
  const long long base = plane * HW;
  double s0 = 0.0, s1 = 0.0;
  if (VEC4) {
    const long long n4 = HW >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(gy + base);
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    for (long long i = lane; i < n4; i += 64) {
      float4 g = g4[i];
      const float4 xv = x4[i];
      if (yact != nullptr) {
        const float4 yv = reinterpret_cast<const float4*>(yact + base)[i];
        if (!(yv.x > 0.f)) g.x *= slope;
        if (!(yv.y > 0.f)) g.y *= slope;
        if (!(yv.z > 0.f)) g.z *= slope;
        if (!(yv.w > 0.f)) g.w *= slope;
        reinterpret_cast<float4*>(gz + base)[i] = g;
      }
      s0 += (double)g.x + (double)g.y + (double)g.z + (double)g.w;
      s1 += (double)g.x * (double)((xv.x - mu) * rs) + (double)g.y * (double)((xv.y - mu) * rs) +
            (double)g.z * (double)((xv.z - mu) * rs) + (double)g.w * (double)((xv.w - mu) * rs);
    }
  } else {
    for (long long i = lane; i < HW; i += 64) {
      float g = gy[base + i];
      if (yact != nullptr) {
        if (!(yact[base + i] > 0.f)) g *= slope;
        gz[base + i] = g;
      }
      s0 += (double)g;
      s1 += (double)g * (double)((x[base + i] - mu) * rs);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64);
    s1 += __shfl_xor(s1, o, 64);
  }
  if (lane == 0) {
    part[plane * 2] = s0;
    part[plane * 2 + 1] = s1;
  }
}

}  // namespace
