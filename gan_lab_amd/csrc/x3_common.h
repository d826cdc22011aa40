// The vocabulary shared by the split-product (3xbf16) convolution kernels: conv_x3.hip (where the arithmetic is explained),
// conv_x3_up.hip, conv_x3_down.hip, conv_x3_wgrad.hip, conv_x3_s2_wgrad.hip.  Every item is a macro or a forced-inline device
// function: moving one here leaves a kernel's instruction stream as it was (tools/isa_diff.py checks that).
#pragma once
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// ---- staging loads -----------------------------------------------------------------------------------------------------------
// The loads are inline asm: hipcc neither sees them in its vmcnt bookkeeping (beside an LDS-DMA it waits vmcnt(0) in front of
// the first use of any load it does see: the whole prefetch pipeline drained several times per stage) nor may recycle their
// registers before x3_ld_wait, which is tied to them and counts the younger operations by hand.
// x3_rsrc: a raw buffer resource over [base, base + bytes): a load outside the range (offset 0x80000000) returns zeros.
__device__ __forceinline__ u32x4 x3_rsrc(const void* base, unsigned bytes) {
  const unsigned long long b = reinterpret_cast<unsigned long long>(base);
  return u32x4{(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32)) & 0xffffu,
               (unsigned)__builtin_amdgcn_readfirstlane((int)bytes), 0x00020000u};
}
__device__ __forceinline__ void x3_ld(f32x4& d, const u32x4& rs, int voff, int soff) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(d) : "v"(voff), "s"(rs), "s"(soff));
}
// ... with no scalar offset (an overload of its own: a zero passed in a scalar register is another instruction stream).
// Neither form clobbers "memory": volatile asm statements keep their order among themselves, and what these loads read is
// written by no store the compiler sees (kernel inputs; conv_x3_s2_wgrad.hip's workspace tiles, stored by asm).
__device__ __forceinline__ void x3_ld(f32x4& d, const u32x4& rs, int voff) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(d) : "v"(voff), "s"(rs));
}
// The loads' data, once all but the `YOUNGER` vector-memory operations issued after them have completed.  The wait is tied to
// the loads' registers (they count as rewritten by it), so no use of them can be scheduled in front of it.
template <int YOUNGER>
__device__ __forceinline__ void x3_ld_wait(f32x4 (&a)[4]) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]) : "n"(YOUNGER));
}
template <int YOUNGER>
__device__ __forceinline__ void x3_ld_wait(f32x4 (&a)[4], f32x4& s_, f32x4& t_) {
  asm volatile("s_waitcnt vmcnt(%6)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(s_), "+v"(t_) : "n"(YOUNGER));
}
template <int YOUNGER>
__device__ __forceinline__ void x3_ld_wait(f32x4& a, f32x4& b) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(YOUNGER));
}

// The barrier of a stage: everything a wave must have finished before it - its LDS-DMA of the next stage's weights (all but
// the `YOUNGER` vector-memory operations issued after them), its ds_writes and ds_reads.
template <int YOUNGER>
__device__ __forceinline__ void x3_barrier() {
  if constexpr (YOUNGER == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else if constexpr (YOUNGER == 4) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  static_assert(YOUNGER == 0 || YOUNGER == 4 || YOUNGER == 6, "an activation staging issues four loads (six with the affine)");
}

// ---- matrix work -------------------------------------------------------------------------------------------------------------
// The MFMAs are inline asm: accumulators pinned in their registers (tied operand), issued in exactly the order written (hipcc
// renamed the accumulators of an unrolled k-loop across registers and spilled them into the loop).  hipcc's hazard recogniser
// does not see through asm: an accumulator read by the vector ALU needs the matrix pipe drained first (X3_DRAIN before a chain
// dump and an epilogue), and a vector-ALU write to one is not interlocked against the MFMA that reads it as srcC two
// instructions later (X3_SETTLE behind the zeroing).
#define X3_MFMA(acc, a, b) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b))
// drain / settle: wait states tied to an operand list - "+v"(acc), ...: a whole accumulator set, spelled by the kernel's own
// list macro.  The set counts as rewritten by them, so neither the vector-ALU code in front of the block nor the MFMAs behind it
// can be scheduled across.
#define X3_DRAIN(...) asm volatile("s_nop 15\n\ts_nop 15" : __VA_ARGS__)
#define X3_SETTLE(...) asm volatile("s_nop 7\n\ts_nop 7" : __VA_ARGS__)

// ---- the split ---------------------------------------------------------------------------------------------------------------
// v into lane j of three plane vectors (gl_split3 of common.h; written on the vector lanes: handing the three scalars over
// afterwards orders the kernels' staging code differently)
__device__ __forceinline__ void x3_split_lane(float v, int j, bf16x4& h, bf16x4& m, bf16x4& l) {
  h[j] = (__bf16)v;
  const float r1 = v - (float)h[j];
  m[j] = (__bf16)r1;
  l[j] = (__bf16)(r1 - (float)m[j]);
}
// four values into planes, 8 bytes each
__device__ __forceinline__ void x3_split4(const f32x4& v, u32x2& h, u32x2& m, u32x2& l) {
  bf16x4 hh, mm, ll;
#pragma unroll
  for (int j = 0; j < 4; ++j) x3_split_lane(v[j], j, hh, mm, ll);
  h = __builtin_bit_cast(u32x2, hh); m = __builtin_bit_cast(u32x2, mm); l = __builtin_bit_cast(u32x2, ll);
}

}  // namespace
