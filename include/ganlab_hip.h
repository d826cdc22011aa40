/*
 * ganlab_hip.h - C ABI of the MI355X (gfx950) kernel library for the gan-lab G+D training step.
 *
 * The reference (sidward14/gan-lab v0.4.2) is pure Python/PyTorch: it has no FFI, plugin or
 * operator interface of its own.  The boundary this library replaces is therefore
 * the set of ATen call sites inside the reference's layer ops; each entry point below cites the
 * reference file:line (relative to /root/reference/gan_lab) whose math it implements.  A
 * maintainer binds these with ctypes from `torch.autograd.Function`s - see INTEGRATION.md and
 * gan_lab_amd/_lib.py.
 *
 * Conventions
 *  - all tensors are fp32, contiguous NCHW (weights OIHW), device pointers owned by the caller;
 *  - nothing is allocated inside: scratch is a caller-provided workspace;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *  - return value: 0 on success, negative GANLAB_E* on error (never throws across the ABI);
 *  - re-entrant: no global mutable state.
 */
#ifndef GANLAB_HIP_H
#define GANLAB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GANLAB_OK 0
#define GANLAB_EINVAL (-1)   /* bad argument (null pointer, non-positive dim, unsupported ks) */
#define GANLAB_EWORKSPACE (-2) /* workspace too small */
#define GANLAB_ELAUNCH (-3)  /* hipGetLastError() != hipSuccess after the launch */
#define GANLAB_EUNSUPPORTED (-4) /* geometry outside what the fused kernel handles (see *_supported) */

#define GANLAB_ACT_NONE 0
#define GANLAB_ACT_LRELU 1

#define GANLAB_PACK_FWD 0    /* out[tap][ci][co] = scale * w[co][ci][tap]                */
#define GANLAB_PACK_DGRAD 1  /* out[tap][co][ci] = scale * w[co][ci][KK-1-tap] (flipped) */

int ganlab_abi_version(void);

/* Diagnostic (no reference counterpart): demangled symbol and workgroup count of the calling thread's most recent
 * kernel launch made by this library.  Returns the symbol's length (it is truncated to cap-1 characters), 0 when
 * nothing was launched yet.  bench.py uses it to name the kernel its `roofline` prices from what was dispatched. */
int ganlab_last_launch(char* name, int cap, unsigned* grid);
/* Diagnostics for tests that assert WHICH kernels a step dispatched (an entry point may launch several: a weight
 * gradient and its slot reduction): the number of kernels the calling thread has launched through this library so far,
 * and the launch `back` positions before its most recent one (0 = what ganlab_last_launch reports; the library keeps
 * the last 16; returns 0 beyond that). */
unsigned long long ganlab_launch_count(void);
int ganlab_launch_history(int back, char* name, int cap, unsigned* grid);

/* Geometry of one convolution C(x, w) = scale * conv2d(up2?(x), w, stride 1, padding pad).
 * Replaces Conv2dEx.forward / LinearEx.forward (utils/custom_layers.py:202-211, :282-291) with the
 * eq-LR runtime scale folded into `scale` (the reference multiplies the input, :204), and the
 * nearest-neighbour 2x upsample in front of a generator conv
 * (stylegan/architectures.py:292-334, progan/architectures.py:119-148) folded in as `up`. */
typedef struct {
  int N, Cin, Hin, Win; /* physical input (before the optional 2x nearest upsample)     */
  int Cout, ks, pad;    /* square kernel ks in {1,3}; a 4x4 valid conv is run as a linear */
  int up;               /* 1: input is nearest-upsampled 2x on the fly                   */
  int pool;             /* 1: output is 2x2 average-pooled (ganlab_conv_s2_* entry points only) */
} ganlab_conv_geom;

/* sizeof(ganlab_conv_geom) as this library was compiled: a binding asserts its mirror struct against it once. */
int ganlab_conv_geom_size(void);

/* Output spatial size of a geometry: Hout = (up ? 2*Hin : Hin) + 2*pad - ks + 1. */
int ganlab_conv_out_hw(const ganlab_conv_geom* g, int* Hout, int* Wout);

/* Re-layout OIHW weights for the implicit-GEMM kernels; `mode` is GANLAB_PACK_*.
 * Returns the number of floats the packed buffer needs when `out` is NULL. */
long long ganlab_conv_pack_f32(const float* w, float* out, int Cout, int Cin, int ks, int mode,
                               float scale, void* stream);

/* y = act( conv(x, wp) + bias * bias_scale ), fp32 MFMA implicit GEMM.
 * wp: GANLAB_PACK_FWD-packed weights (scale already folded in).  bias may be NULL.
 * custom_layers.py:202-211 (+ Conv2dBias :222-226, LeakyReLU) */
int ganlab_conv_fwd_f32(const float* x, const float* wp, const float* bias, float* y,
                        const ganlab_conv_geom* g, float bias_scale, int act, float slope,
                        void* stream);

/* gx = conv_transpose(gy, w) wrt the conv input (the autograd rule of custom_layers.py:204-206).
 * wp: GANLAB_PACK_DGRAD-packed weights.  When g->up == 1 the result is the gradient w.r.t. the
 * *virtual* (upsampled) input, shape (N, Cin, 2*Hin, 2*Win); fold it with ganlab_pool2_f32. */
int ganlab_conv_dgrad_f32(const float* gy, const float* wp, float* gx_virtual,
                          const ganlab_conv_geom* g, void* stream);

/* Split-K variants for the small, channel-heavy layers (512-channel 4x4 / 8x8 maps; linear layers at small batch), whose
 * plain launch is a few dozen workgroups walking a long contraction: ganlab_conv_splitk_plan returns S (0 / 1: use the plain
 * entry point); S >= 2: S workgroups share one output tile, raw partial sums go to the workspace (S * output elements
 * floats) and a finishing kernel adds them in a fixed order, + bias, + activation.  No upsample. */
int ganlab_conv_splitk_plan(const ganlab_conv_geom* g, int dgrad);
int ganlab_conv_fwd_splitk_f32(const float* x, const float* wp, const float* bias, float* y, const ganlab_conv_geom* g,
                               float bias_scale, int act, float slope, void* workspace, size_t workspace_bytes,
                               void* stream);
int ganlab_conv_dgrad_splitk_f32(const float* gy, const float* wp, float* gx, const ganlab_conv_geom* g, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* gx = dgrad(gy, w) * lrelu'(x) where x, the conv's input (shaped like gx), is the LeakyReLU output of the layer in
 * front (D block k's pooled conv -> block k+1's first conv, progan/architectures.py:280-293): that layer's backward then
 * takes gx as the gradient of its PRE-activation and skips its own gy * lrelu'(y) pass.  3x3 pad-1 convs, no
 * upsample, rows of >= 16 4-aligned pixels (*_supported). */
int ganlab_conv_dgrad_mask_supported(const ganlab_conv_geom* g);
int ganlab_conv_dgrad_mask_f32(const float* gy, const float* wp, const float* x, float* gx, const ganlab_conv_geom* g,
                               float slope, void* stream);

/* fromRGB (1x1 conv from <= 3 channels + bias + LeakyReLU, progan/architectures.py:232-237) at >= 64x64 runs on
 * HBM-streaming kernels that can fold the activation's backward into the conv's own gradient kernels, saving the
 * separate  gz = gy * lrelu'(y)  pass over the widest tensor of the discriminator:
 *   dgrad_act : gx = dgrad(gy * lrelu'(y), w)             fwd_mask : out = conv(x, w) * lrelu'(y)  (its adjoint)
 *   wgrad_act : gw = scale * wgrad(gy * lrelu'(y), x) and gb = bias_scale * sum(gy * lrelu'(y))
 * y is the conv's activated OUTPUT.  *_supported() == 0 -> GANLAB_EUNSUPPORTED, compose the plain entry points. */
int ganlab_conv_act_bwd_fused_supported(const ganlab_conv_geom* g);
int ganlab_conv_dgrad_act_f32(const float* gy, const float* y, const float* wp, float* gx, const ganlab_conv_geom* g,
                              float slope, void* stream);
int ganlab_conv_fwd_mask_f32(const float* x, const float* wp, const float* y, float* out, const ganlab_conv_geom* g,
                             float slope, void* stream);
int ganlab_conv_wgrad_act_f32(const float* gy, const float* y, const float* x, float* gw, float* gb,
                              const ganlab_conv_geom* g, float scale, float bias_scale, float slope, void* workspace,
                              size_t workspace_bytes, void* stream);

/* gw[co][ci][ky][kx] = scale * sum_{n,y,x} gy[n,co,y,x] * up2?(x)[n,ci,y+ky-pad,x+kx-pad].
 * Deterministic two-stage reduction through `workspace`; query the size with
 * ganlab_conv_wgrad_workspace (bytes). */
size_t ganlab_conv_wgrad_workspace(const ganlab_conv_geom* g);
int ganlab_conv_wgrad_f32(const float* gy, const float* x, float* gw, const ganlab_conv_geom* g,
                          float scale, void* workspace, size_t workspace_bytes, void* stream);

/* ---- stride-2 fused layers (csrc/conv_s2.hip) -------------------------------------------------------
 * D "down" layer AvgPool2d(2)(conv3x3(x)) (progan/architectures.py:261-284; geom.pool = 1) and G "up"
 * layer conv3x3(Upsample2x(x)) (stylegan/architectures.py:292-334; geom.up = 1) collapse exactly to a
 * 4x4 stride-2 kernel K4 = M W M^T: 16 instead of 36 MACs per low-res pixel, no full-resolution
 * intermediate.  Same calling convention as the plain entry points; `geom` describes the ORIGINAL 3x3
 * layer (ks = 3, pad = 1, exactly one of up / pool set).  ganlab_conv_s2_supported() tells whether the
 * shape qualifies (even sizes, low-res width >= 16 and a multiple of 4); otherwise compose the plain
 * kernels.  pack: `up` selects the combination matrix, `transpose` = 1 packs for the operator that
 * consumes the output gradient (dgrad). */
int ganlab_conv_s2_supported(const ganlab_conv_geom* g);
long long ganlab_conv_s2_pack_f32(const float* w, float* out, int Cout, int Cin, int up, int transpose,
                                  float scale, void* stream);
int ganlab_conv_s2_fwd_f32(const float* x, const float* wp, const float* bias, float* y,
                           const ganlab_conv_geom* g, float bias_scale, int act, float slope, void* stream);
int ganlab_conv_s2_dgrad_f32(const float* gy, const float* wp, float* gx, const ganlab_conv_geom* g,
                             void* stream);
size_t ganlab_conv_s2_wgrad_workspace(const ganlab_conv_geom* g);
int ganlab_conv_s2_wgrad_f32(const float* gy, const float* x, float* gw, const ganlab_conv_geom* g,
                             float scale, void* workspace, size_t workspace_bytes, void* stream);

/* ---- bf16-compute convolutions (csrc/conv_bf16.hip; BASELINE config #2 "bf16 compute / fp32 master") ---------
 * Same math and call sites as the fp32 entry points above (custom_layers.py:202-211 and its autograd rules), but
 * the operands are rounded to bf16 (RNE) on their way into LDS and multiplied on v_mfma_f32_16x16x32_bf16 with fp32
 * accumulation; every tensor in HBM stays fp32 (the reference's storage type, fp32 master weights).  The reference
 * itself is fp32 only, so this path is an extension selected by the caller (gan_lab_amd.ops.compute_dtype).
 * Supported (ganlab_conv_bf16_supported; forward and input gradient): 3x3, pad 1, Cin % 64 == 0, Cout % 64 == 0 and, at
 * the resolution the taps run on (2 Hin x 2 Win with up), either H % 8 == 0, W % 32 == 0 or H % 16 == 0, W % 16 == 0;
 * up (nearest 2x upsample in front, progan/architectures.py:160-186) or pool (2x2 average pool behind, :261-284) - not
 * both - fold into the kernels: x / gx are Hin x Win, y / gy are Ho x Wo as for ganlab_conv_s2_*; everything else stays
 * on the exact fp32 kernels.  The weight gradient needs W % 32 == 0, H % 8 == 0 at the taps' resolution (with up it reads
 * the Hin x Win input in place, with pool the pooled gy): ganlab_conv_wgrad_bf16_workspace returns 0 for a geometry it
 * does not take (ganlab_conv_wgrad_bf16 then returns GANLAB_EUNSUPPORTED) and the caller uses ganlab_conv_wgrad_f32 on
 * the plain geometry with the materialised upsample of x, resp. of gy / 4.
 * pack: returns the number of bf16 elements (9*Cout*Cin) when `out` is NULL; mode is GANLAB_PACK_*. */
int ganlab_conv_bf16_supported(const ganlab_conv_geom* g);
long long ganlab_conv_pack_bf16(const float* w, void* out, int Cout, int Cin, int mode, float scale, void* stream);
int ganlab_conv_fwd_bf16(const float* x, const void* wp, const float* bias, float* y, const ganlab_conv_geom* g,
                         float bias_scale, int act, float slope, void* stream);
int ganlab_conv_dgrad_bf16(const float* gy, const void* wp, float* gx, const ganlab_conv_geom* g, void* stream);
/* split-K forms of the two for layers with few output tiles (the 512-channel 16x16 layers at batch 8: 64 workgroups on 256
 * CUs): ganlab_conv_bf16_splitk_plan = number of K-splits S (1: nothing to split); workspace: S * N * C * H * W floats at the
 * taps' resolution (C: the operator's output channels), raw partial sums + a fixed-order finish (pool / scale / bias / act) */
int ganlab_conv_bf16_splitk_plan(const ganlab_conv_geom* g, int dgrad);
int ganlab_conv_fwd_bf16_splitk(const float* x, const void* wp, const float* bias, float* y, const ganlab_conv_geom* g,
                                float bias_scale, int act, float slope, void* workspace, size_t workspace_bytes,
                                void* stream);
int ganlab_conv_dgrad_bf16_splitk(const float* gy, const void* wp, float* gx, const ganlab_conv_geom* g, void* workspace,
                                  size_t workspace_bytes, void* stream);
size_t ganlab_conv_wgrad_bf16_workspace(const ganlab_conv_geom* g);
int ganlab_conv_wgrad_bf16(const float* gy, const float* x, float* gw, const ganlab_conv_geom* g, float scale,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- fp32 convolutions as split products on the bf16 matrix cores (csrc/conv_x3.hip) ---------------------------------
 * Same math and call sites as ganlab_conv_fwd_f32 / ganlab_conv_dgrad_f32 (custom_layers.py:202-211), fp32 in, fp32 out:
 * every operand is cut into three bf16 planes that sum to it EXACTLY, a product is six v_mfma_f32_16x16x32_bf16 products
 * (the three dropped cross terms are <= 2^-26 of it) and the sums are kept in fp32 chains of one 32-channel chunk each,
 * so the result is as close to float64 as the exact-fp32 kernels' (tools/op_error_probe.py) at 16/6 of their MFMA rate.
 * Supported (ganlab_conv_x3_supported): 3x3, pad 1, no up / pool, H % 16 == 0, W % 16 == 0, contraction channels % 64 == 0,
 * output channels % 64 == 0.  pack: OIHW -> three-plane k-step images, returns the number of bf16 elements
 * (27*Cout*Cin) when `out` is NULL; mode is GANLAB_PACK_*. */
int ganlab_conv_x3_supported(const ganlab_conv_geom* g, int dgrad);
long long ganlab_conv_x3_pack(const float* w, void* out, int Cout, int Cin, int mode, float scale, void* stream);
int ganlab_conv_fwd_x3(const float* x, const void* wp, const float* bias, float* y, const ganlab_conv_geom* g,
                       float bias_scale, int act, float slope, void* stream);
int ganlab_conv_dgrad_x3(const float* gy, const void* wp, float* gx, const ganlab_conv_geom* g, void* stream);
/* the forms of the exact-fp32 entry points the thick layers use, same arguments except the packed weights:
 * ganlab_conv_dgrad_mask_f32, ganlab_conv_fwd_aff_f32, ganlab_conv_fwd_aff_tail_f32 (+ its tiles-per-plane query) */
int ganlab_conv_dgrad_mask_x3(const float* gy, const void* wp, const float* x, float* gx, const ganlab_conv_geom* g,
                              float slope, void* stream);
int ganlab_conv_fwd_aff_x3(const float* x, const void* wp, const float* aff_s, const float* aff_t, const float* bias,
                           float* y, const ganlab_conv_geom* g, float bias_scale, int act, float slope, void* stream);
int ganlab_conv_fwd_aff_tail_x3_chunks(const ganlab_conv_geom* g);
/* the stride-2 fused layers' transposed form (the exact-fp32 T kernel of csrc/conv_s2.hip): ganlab_conv_s2_fwd_f32 /
 * ganlab_conv_s2_fwd_aff_f32 of an up layer (geom.up = 1; dgrad = 0) and ganlab_conv_s2_dgrad_f32 of a pooled layer
 * (geom.pool = 1; dgrad = 1), low resolution H % 8 == 0, W % 16 == 0, contraction channels % 64 == 0, output channels
 * % 32 == 0 (not a multiple of 64: the 32-channel form - both row parities per workgroup, its own packed layout).  pack: `up` = 1 packs an up
 * layer's forward weights, 0 a pooled layer's input-gradient weights (48*Cout*Cin bf16 elements; in a ganlab_pack_desc:
 * kind GANLAB_PACKKIND_X3 with ks = 4 and the same `up`). */
int ganlab_conv_s2_x3_supported(const ganlab_conv_geom* g, int dgrad);
long long ganlab_conv_s2_x3_pack(const float* w, void* out, int Cout, int Cin, int up, float scale, void* stream);
int ganlab_conv_s2_fwd_x3(const float* x, const void* wp, const float* bias, float* y, const ganlab_conv_geom* g,
                          float bias_scale, int act, float slope, void* stream);
int ganlab_conv_s2_fwd_aff_x3(const float* x, const void* wp, const float* aff_s, const float* aff_t, const float* bias,
                              float* y, const ganlab_conv_geom* g, float bias_scale, int act, float slope, void* stream);
int ganlab_conv_s2_dgrad_x3(const float* gy, const void* wp, float* gx, const ganlab_conv_geom* g, void* stream);
/* ... and their strided form (csrc/conv_x3_down.hip; the exact-fp32 S kernel of csrc/conv_s2.hip): ganlab_conv_s2_fwd_f32 of a
 * pooled layer (geom.pool = 1; dgrad = 0) and ganlab_conv_s2_dgrad_f32 of an up layer (geom.up = 1; dgrad = 1); low resolution
 * H % 8 == 0, W % 16 == 0, contraction channels % 16 == 0, output channels % 128 == 0.  pack: `up` = 0 a pooled layer's forward
 * weights, 1 an up layer's input-gradient weights (48*Cout*Cin bf16 elements; ganlab_pack_desc: kind X3, ks = 5, same `up`). */
int ganlab_conv_s2_down_x3_supported(const ganlab_conv_geom* g, int dgrad);
long long ganlab_conv_s2_down_x3_pack(const float* w, void* out, int Cout, int Cin, int up, float scale, void* stream);
int ganlab_conv_s2_down_fwd_x3(const float* x, const void* wp, const float* bias, float* y, const ganlab_conv_geom* g,
                               float bias_scale, int act, float slope, void* stream);
int ganlab_conv_s2_down_dgrad_x3(const float* gy, const void* wp, float* gx, const ganlab_conv_geom* g, void* stream);
/* weight gradient of a plain 3x3 layer (csrc/conv_x3_wgrad.hip): ganlab_conv_wgrad_f32, or with aff_s / aff_t non-null
 * ganlab_conv_wgrad_aff_f32, as split products; H a power of two, W % 32 == 0, Cin % 64 == 0, Cout % 32 == 0.  Deterministic
 * (per-workgroup slots in the workspace, fixed-order reduction). */
int ganlab_conv_wgrad_x3_supported(const ganlab_conv_geom* g);
size_t ganlab_conv_wgrad_x3_workspace(const ganlab_conv_geom* g);
int ganlab_conv_wgrad_x3(const float* gy, const float* x, const float* aff_s, const float* aff_t, float* gw,
                         const ganlab_conv_geom* g, float scale, void* workspace, size_t workspace_bytes, void* stream);
/* weight gradient of a stride-2 3x3 layer (csrc/conv_x3_s2_wgrad.hip; geom.pool = 1: avgpool2(conv3(x)), geom.up = 1:
 * conv3(up2(x))): ganlab_conv_s2_wgrad_f32, or with aff_s / aff_t non-null (up layers) ganlab_conv_s2_wgrad_aff_f32, as split
 * products over the 2x2 box sums of the high-resolution operand; low resolution H a power of two >= 4, W % 32 == 0 or W == 16, channels of
 * the low-resolution operand (pool: Cout, up: Cin) % 64 == 0, of the high-resolution one % 32 == 0.  Deterministic. */
int ganlab_conv_s2_wgrad_x3_supported(const ganlab_conv_geom* g);
size_t ganlab_conv_s2_wgrad_x3_workspace(const ganlab_conv_geom* g);
int ganlab_conv_s2_wgrad_x3(const float* gy, const float* x, const float* aff_s, const float* aff_t, float* gw,
                            const ganlab_conv_geom* g, float scale, void* workspace, size_t workspace_bytes, void* stream);
int ganlab_conv_fwd_aff_tail_x3(const float* x, const void* wp, const float* aff_s, const float* aff_t, const float* bias,
                                const float* noise, const float* noise_w, float* y, float* mean, float* rstd,
                                const ganlab_conv_geom* g, float bias_scale, int act, float slope, float eps, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- depthwise / resampling (custom_layers.py:36-53; nn.Upsample / nn.AvgPool2d call sites) ---- */
/* y = depthwise [1 2 1]x[1 2 1]/16 blur, zero padding (self-adjoint: also its own backward). */
int ganlab_blur3x3_f32(const float* x, float* y, long long planes, int H, int W, void* stream);
/* y[2h+i,2w+j] = scale * x[h,w]  (nearest upsample; backward of pool2) */
int ganlab_up2_f32(const float* x, float* y, long long planes, int H, int W, float scale, void* stream);
/* y[h,w] = scale * sum_{i,j<2} x[2h+i,2w+j]  (avg-pool with scale .25; backward of up2) */
int ganlab_pool2_f32(const float* x, float* y, long long planes, int Hout, int Wout, float scale,
                     void* stream);
/* The other resamplers of custom_layers.py:59-75 (NearestPool2d, BilinearPool2d) and of nn.Upsample(mode='bilinear')
 * (resnetgan/learner.py:147-170), forward and adjoint: a separable table-driven gather
 *   y[p,oy,ox] = sum_{a<Ty} sum_{b<Tx} wy[oy*Ty+a] * wx[ox*Tx+b] * x[p, iy[oy*Ty+a], ix[ox*Tx+b]]
 * with int32 source indices / float weights per output row and column (1 <= Ty, Tx <= 6; pad with weight 0). */
int ganlab_resample2d_f32(const float* x, float* y, const int* iy, const float* wy, const int* ix, const float* wx,
                          long long planes, int Hi, int Wi, int Ho, int Wo, int Ty, int Tx, void* stream);

/* ---- bias / activation / noise (custom_layers.py:213-226, stylegan/architectures.py:105-119) ---- */
/* y = act(x + noise_w[c]*noise[n,hw] + bias[c]*bias_scale); noise/noise_w and bias may be NULL. */
int ganlab_bias_act_f32(const float* x, const float* bias, const float* noise, const float* noise_w,
                        float* y, int N, int C, long long HW, float bias_scale, int act, float slope,
                        void* stream);
/* gz = gy * (y > 0 ? 1 : slope)   (LeakyReLU backward from the saved OUTPUT) */
int ganlab_act_bwd_f32(const float* gy, const float* y, float* gz, long long n, float slope, void* stream);
/* gz = gy * (y > 0 ? 1 : slope) and gb[c] = scale * sum_{n,hw} gz[n,c,hw] in ONE pass (the backward of
 * Conv2dBias + LeakyReLU, custom_layers.py:222-226); workspace as ganlab_channel_sum_workspace */
int ganlab_act_bwd_bias_f32(const float* gy, const float* y, float* gz, float* gb, int N, int C, long long HW,
                            float slope, float scale, void* workspace, size_t workspace_bytes, void* stream);
/* ---- blur fused with its pointwise neighbours (H even, W % 4 == 0: ganlab_blur_fused_supported) --------
 * The binomial blur of a G layer sits between the up-conv and noise/bias/LeakyReLU
 * (stylegan/architectures.py:331-360 -> :105-119, progan/architectures.py:95-107), that of a D block
 * between LeakyReLU and the down-conv (progan/architectures.py:280-293): one pass instead of two.
 *   blur_bias_act:  y   = act(blur(x) + noise_w[c]*noise[n,hw] + bias[c]*bias_scale)
 *   blur_act_bwd:   out = lrelu'(y) * blur(g),  gb[c] = bias_scale * sum out        (gb nullable)
 *   act_bwd_blur:   out = blur(lrelu'(y) * g),  gb[c] = bias_scale * sum lrelu'(y)*g,
 *                   gnw[c] = sum lrelu'(y)*g*noise[n,hw]                             (gb, gnw nullable)
 * blur_act_bwd and act_bwd_blur are adjoint: each is the other's backward (R1 double backward). */
int ganlab_blur_fused_supported(int H, int W);
size_t ganlab_blur_fused_workspace(int N, int C, int H, int W);
int ganlab_blur_bias_act_f32(const float* x, const float* bias, const float* noise, const float* noise_w, float* y,
                             int N, int C, int H, int W, float bias_scale, int act, float slope, void* stream);
int ganlab_blur_act_bwd_f32(const float* g, const float* y, float* out, float* gb, int N, int C, int H, int W,
                            float slope, float bias_scale, void* workspace, size_t workspace_bytes, void* stream);
int ganlab_act_bwd_blur_f32(const float* g, const float* y, const float* noise, float* out, float* gb, float* gnw,
                            int N, int C, int H, int W, float slope, float bias_scale, void* workspace,
                            size_t workspace_bytes, void* stream);
/* The same two forward ops, also producing the InstanceNorm statistics of their OUTPUT in the same pass (the generator
 * layer is conv -> [blur] -> noise + bias + LeakyReLU -> InstanceNorm + style, stylegan/architectures.py:497-526: the
 * statistics pass of ganlab_instnorm_stats_f32 over the tensor just written is saved).  mean / rstd: (N*C,), rstd =
 * 1/sqrt(biased var + eps); fp64 sums; workspace ganlab_act_stats_workspace bytes.  HW % 4 == 0. */
size_t ganlab_act_stats_workspace(int N, int C, long long HW);
int ganlab_bias_act_stats_f32(const float* x, const float* bias, const float* noise, const float* noise_w, float* y,
                              float* mean, float* rstd, int N, int C, long long HW, float bias_scale, int act,
                              float slope, float eps, void* workspace, size_t workspace_bytes, void* stream);
int ganlab_blur_bias_act_stats_f32(const float* x, const float* bias, const float* noise, const float* noise_w,
                                   float* y, float* mean, float* rstd, int N, int C, int H, int W, float bias_scale,
                                   int act, float slope, float eps, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* ... and the matching backward: InstanceNorm+style backward fused with the LeakyReLU / bias / noise backward in front
 * of it (x = that layer's activated output = the InstanceNorm input).  gz = dL/d(pre-activation), gb (C,) =
 * bias_scale * sum gz or NULL, gnw (C,) = sum gz*noise or NULL; s1, s2 from ganlab_instnorm_style_bwd_reduce_f32. */
size_t ganlab_instnorm_bwd_act_workspace(int N, int C, long long HW);
int ganlab_instnorm_style_bwd_act_f32(const float* gy, const float* x, const float* mean, const float* rstd,
                                      const float* style, const float* s1, const float* s2, const float* noise,
                                      float* gz, float* gb, float* gnw, int N, int C, long long HW, int act,
                                      float slope, float bias_scale, void* workspace, size_t workspace_bytes,
                                      void* stream);
/* ... followed by the (self-adjoint) blur of a BLURRED generator layer in the same pass: out = blur(gz), gz is not written
 * (blur -> noise/bias/LeakyReLU -> InstanceNorm/style backward of stylegan/architectures.py:497-526 behind :331-360) */
int ganlab_instnorm_style_bwd_act_blur_f32(const float* gy, const float* x, const float* mean, const float* rstd,
                                           const float* style, const float* s1, const float* s2, const float* noise,
                                           float* out, float* gb, float* gnw, int N, int C, int H, int W, int act,
                                           float slope, float bias_scale, void* workspace, size_t workspace_bytes,
                                           void* stream);
/* The same two passes (ganlab_instnorm_style_bwd_reduce_f32, ganlab_instnorm_style_bwd_act_f32) for the generator's LAST
 * layer, whose only reader is toRGB (stylegan/architectures.py:170-172, :398-402 - a 1x1 conv to crgb <= 4 channels): the
 * incoming gradient  gy[n, c] = sum_k wp[k * round_up(C, 64) + c] * grgb[n, k]  is recomputed from the image gradient grgb
 * (N, crgb, HW) and toRGB's input-gradient pack wp (scale included) instead of being written by ganlab_conv_dgrad_f32 and
 * read back twice.  gz / gb / gnw carry the bits of that sequence given the same s1 / s2; s1 / s2 are fp64 sums in another
 * order (equal after rounding to fp32 up to ties).  C <= 16, HW % 4 == 0, HW >= 1024. */
int ganlab_instnorm_bwd_rgb_supported(int N, int C, int crgb, long long HW);
size_t ganlab_instnorm_bwd_reduce_rgb_workspace(int N, int C, long long HW);
int ganlab_instnorm_style_bwd_reduce_rgb_f32(const float* grgb, const float* wp, int crgb, const float* x,
                                             const float* mean, const float* rstd, float* s1, float* s2, int N, int C,
                                             long long HW, void* workspace, size_t workspace_bytes, void* stream);
int ganlab_instnorm_style_bwd_act_rgb_f32(const float* grgb, const float* wp, int crgb, const float* x, const float* mean,
                                          const float* rstd, const float* style, const float* s1, const float* s2,
                                          const float* noise, float* gz, float* gb, float* gnw, int N, int C, long long HW,
                                          int act, float slope, float bias_scale, void* workspace, size_t workspace_bytes,
                                          void* stream);
/* out[c] = scale * sum_{n,hw} a[n,c,hw] * (b ? b[n,hw] : 1)   (bias / noise-weight gradients) */
int ganlab_channel_sum_f32(const float* a, const float* b_n1hw, float* out, int N, int C, long long HW,
                           float scale, void* workspace, size_t workspace_bytes, void* stream);
size_t ganlab_channel_sum_workspace(int N, int C, long long HW);

/* ---- normalisation ---- */
/* InstanceNorm2d(eps, biased var) statistics per (n,c) plane: mean, rstd (custom_layers.py:98-99) */
int ganlab_instnorm_stats_f32(const float* x, float* mean, float* rstd, long long planes, long long HW,
                              float eps, void* stream);
/* the same statistics for few, long rows (LayerNorm([C,R,R]) of the ResNet critics, custom_layers.py:100-107: `rows` =
 * batch, M = C*R*R): several blocks per row, fp64 partial sums, fixed-order finish (deterministic). */
size_t ganlab_row_stats_workspace(long long rows, long long M);
int ganlab_row_stats_f32(const float* x, float* mean, float* rstd, long long rows, long long M, float eps,
                         void* workspace, size_t workspace_bytes, void* stream);
/* y = (x-mean)*rstd*(ys+1)+yb with style (N,2,C) (stylegan/architectures.py:524-526); style may be
 * NULL (plain InstanceNorm). */
int ganlab_instnorm_style_fwd_f32(const float* x, const float* mean, const float* rstd,
                                  const float* style, float* y, int N, int C, long long HW, void* stream);
/* s1[n,c] = sum gy ; s2[n,c] = sum gy * xhat */
int ganlab_instnorm_style_bwd_reduce_f32(const float* gy, const float* x, const float* mean,
                                         const float* rstd, float* s1, float* s2, long long planes,
                                         long long HW, void* stream);
/* gx = rstd*(ys+1)*(gy - s1/HW - xhat*s2/HW) */
int ganlab_instnorm_style_bwd_apply_f32(const float* gy, const float* x, const float* mean,
                                        const float* rstd, const float* style, const float* s1,
                                        const float* s2, float* gx, int N, int C, long long HW,
                                        void* stream);
/* PixelNorm over the channel dim (custom_layers.py:81-86): y = x*rsqrt(mean_c x^2 + eps) */
int ganlab_pixelnorm_fwd_f32(const float* x, float* y, int N, int C, long long HW, float eps, void* stream);
int ganlab_pixelnorm_bwd_f32(const float* gy, const float* x, float* gx, int N, int C, long long HW,
                             float eps, void* stream);

/* building blocks of BatchNorm2d / LayerNorm (ResNet GAN path, custom_layers.py:100-107): the
 * normalisations are composed from y = x*scale[c] + shift[c], elementwise products and channel sums,
 * each closed under differentiation, so the WGAN-GP double backward works through LayerNorm */
int ganlab_chan_affine_f32(const float* x, const float* scale, const float* shift, float* y, int N, int C,
                           long long HW, void* stream);
int ganlab_mul_f32(const float* a, const float* b, float* out, long long n, void* stream);
/* ---- fused LayerNorm([C,R,R]) of the ResNet critics, first and second order (csrc/norm.hip) ----------------
 * resnetgan/resblocks.py:15-121 -> NormalizeLayer('LayerNorm') = nn.LayerNorm (custom_layers.py:100-107).  A sample
 * is a row of M = C*R*R elements; mean / rstd come from ganlab_instnorm_stats_f32(planes = N, HW = M);
 * P_x(g) = rstd * (g - mean(g) - xhat * mean(g * xhat)) per row.
 *   ln_affine_fwd:   y = act((x - mean[n]) * rstd[n] * w[m] + b[m])                     (w, b nullable; act = GANLAB_ACT_LRELU
 *                    folds in the LeakyReLU / ReLU that follows the normalisation in every residual block,
 *                    resnetgan/resblocks.py:48-49)
 *   colscale:        out[n,m] = a[n,m] * w[m]                                           (ghat = gy * w)
 *   coldot:          o1[m] = sum_n a * f,  f = (x - mean[n]) * rstd[n] (mean given) or x;  o2[m] = sum_n a (nullable)
 *                    -> gw, gb of the backward; d/dw of the double backward
 *   ln_rowsums:      per row n, several blocks per row + a fixed-order finish (deterministic), out = [N][3]:
 *                    t = a*(wa ? wa[m] : 1):  s0 = sum t,  s1 = sum t*xhat,  s2 = sum a*b2*(w2 ? w2[m] : 1) (b2 nullable);
 *                    with yact (the fused layer's OUTPUT) the backward of that LeakyReLU is applied on load,
 *                    a <- a * lrelu'(yact), and the masked gradient is also stored to gz for the passes that follow
 *   ln_project:      out = (wo ? wo[m] : 1) * rstd[n] * (a*(wa ? wa[m] : 1) - s0/M - xhat*s1/M)   (= wo * P_x(a*wa))
 *   ln_bwdbwd_apply: out = c1[n] * xhat + c2[n] * pu + c3[n] * gx    (d/dx of the double backward); the row coefficients
 *                    are formed in the kernel from sums = ln_rowsums(gy, w) and usums = ln_rowsums(u, b2 = gy, w2 = w):
 *                    c1 = -rstd^2 (u2 - s0 u0 - s1 u1), c2 = -rstd s1, c3 = -rstd u1, every sum divided by M */
int ganlab_ln_affine_fwd_f32(const float* x, const float* mean, const float* rstd, const float* w, const float* b,
                             float* y, int N, long long M, int act, float slope, void* stream);
int ganlab_colscale_f32(const float* a, const float* w, float* out, int N, long long M, void* stream);
int ganlab_coldot_f32(const float* a, const float* x, const float* mean, const float* rstd, float* o1, float* o2,
                      int N, long long M, void* stream);
size_t ganlab_ln_rowsums_workspace(int N, long long M);
int ganlab_ln_rowsums_f32(const float* a, const float* wa, const float* x, const float* mean, const float* rstd,
                          const float* b2, const float* w2, float* out, int N, long long M, void* workspace,
                          size_t workspace_bytes, const float* yact, float* gz, float slope, void* stream);
int ganlab_ln_project_f32(const float* a, const float* wa, const float* x, const float* mean, const float* rstd,
                          const float* sums, const float* wo, float* out, int N, long long M, void* stream);
/* ln_bwd_cols: the first-order backward's projection AND parameter gradients in one pass over (a, x), thread per column:
 * gx = rstd[n] * (a*w[m] - s0[n]/M - xhat*s1[n]/M) (= ln_project with wa = w), gw[m] = sum_n a*xhat, gb[m] = sum_n a (= coldot) */
int ganlab_ln_bwd_cols_f32(const float* a, const float* w, const float* x, const float* mean, const float* rstd,
                           const float* sums, float* gx, float* gw, float* gb, int N, long long M, void* stream);
int ganlab_ln_bwdbwd_apply_f32(const float* x, const float* mean, const float* rstd, const float* pu, const float* gx,
                               const float* sums, const float* usums, float* out, int N, long long M, void* stream);
/* ---- fused BatchNorm2d (training mode, first order) of the ResNet generators (csrc/norm.hip) --------------------
 * resnetgan/resblocks.py:15-121 -> NormalizeLayer('BatchNorm') = nn.BatchNorm2d (custom_layers.py:100-107).  A row is
 * a channel (N segments of HW elements); workspace as ganlab_ln_rowsums_workspace(C, N*HW).
 *   bn_stats:     out[c] = {batch mean, biased batch variance, 0}    (fp64 partial sums, evaluated in fp64)
 *   bn_bwd_sums:  out[c] = {sum gy (= d/d bias), sum gy * xhat (= d/d weight), 0}; yact / gz / slope as in ln_rowsums
 *   bn_bwd_apply: gx = pre[c] * (gy - s0/L - xhat * s1/L), pre = rstd * weight, L = N*HW
 *   bn_apply:     y = act((x - mean[c]) * scale[c] + shift[c])  (centred form: keeps the rounding error at eps*|y|)
 *   bn_finalize:  from bn_stats' out: {mean[C], var[C], rstd[C] = rsqrt(var + eps), scale[C] = rstd * weight} into
 *                 out[4][C]; running_mean / running_var (may be NULL) move by ``momentum`` towards the batch mean /
 *                 UNBIASED variance (var * unbias, unbias = L/(L-1)), *batches (may be NULL) += 1 - everything
 *                 nn.BatchNorm2d.forward does besides normalising (torch/nn/modules/batchnorm.py), one launch */
int ganlab_bn_stats_f32(const float* x, float* out, int N, int C, long long HW, void* workspace, size_t workspace_bytes,
                        void* stream);
int ganlab_bn_apply_f32(const float* x, const float* mean, const float* scale, const float* shift, float* y, int N,
                        int C, long long HW, int act, float slope, void* stream);
int ganlab_bn_finalize_f32(const float* mom, const float* weight, float* running_mean, float* running_var,
                           long long* batches, float* out, int C, float eps, float momentum, float unbias,
                           void* stream);
int ganlab_bn_bwd_sums_f32(const float* gy, const float* x, const float* mean, const float* rstd, float* out, int N,
                           int C, long long HW, void* workspace, size_t workspace_bytes, const float* yact, float* gz,
                           float slope, void* stream);
int ganlab_bn_bwd_apply_f32(const float* gy, const float* x, const float* mean, const float* rstd, const float* sums,
                            const float* pre, float* gx, int N, int C, long long HW, void* stream);
/* nn.Tanh of the ResNet generators (resnetgan/architectures.py:55, :93) */
int ganlab_tanh_fwd_f32(const float* x, float* y, long long n, void* stream);
int ganlab_tanh_bwd_f32(const float* gy, const float* y, float* gx, long long n, void* stream);

/* ---- minibatch stddev statistic (custom_layers.py:117-140), contiguous groups of gs samples ---- */
/* stat[g] = mean_f sqrt(var_unbiased_i(x[g,i,f]) + eps),  f over F = C*H*W features */
int ganlab_mbstd_fwd_f32(const float* x, float* stat, int G, int gs, long long F, float eps, void* stream);
/* gx[g,i,f] = gstat[g]/(F(gs-1)) * (x-mu)/s */
int ganlab_mbstd_bwd_f32(const float* x, const float* gstat, float* gx, int G, int gs, long long F,
                         float eps, void* stream);
/* backward of ganlab_mbstd_bwd: given ggx (cotangent of gx) -> g_gstat[g] and g_x[g,i,f] */
int ganlab_mbstd_bwdbwd_f32(const float* x, const float* gstat, const float* ggx, float* g_gstat,
                            float* g_x, int G, int gs, long long F, float eps, void* stream);

/* ---- elementwise / reductions ---- */
/* out = a*x + b*y (y may be NULL -> out = a*x); fade-in blends progan/architectures.py:163-167,311-315 */
int ganlab_axpby_f32(const float* x, const float* y, float* out, long long n, float a, float b, void* stream);
/* out = a * gout[0] * (x ? x : 1): backward of the scalar reductions, gout stays on the device */
int ganlab_scale_dev_f32(const float* x, const float* gout, float* out, long long n, float a, void* stream);
/* out[n,:] = t[n]*a[n,:] + (1-t[n])*b[n,:]  (WGAN-GP interpolates, resnetgan/learner.py:793-796) */
int ganlab_lerp_rows_f32(const float* a, const float* b, const float* t, float* out, long long N, long long M,
                         void* stream);
/* out[0] = scale * sum x  |  scale * sum x^2 */
int ganlab_sum_f32(const float* x, float* out, long long n, float scale, int squared, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t ganlab_sum_workspace(long long n);
/* BCE-with-logits vs a constant target t, mean over n (progan/learner.py:793-800, :886-896) */
int ganlab_bce_logits_fwd_f32(const float* x, float* out, int n, float target, void* stream);
int ganlab_bce_logits_bwd_f32(const float* x, const float* gout, float* gx, int n, float target, void* stream);
/* hinge term of a constant-target loss: out[0] = mean(max(a + b*x, 0)); bwd: gx = gout[0] * (a + b*x > 0 ? b : 0) / n
 * (loss_D = hinge(1, -1)(D(real)) + hinge(1, +1)(D(fake)); piecewise linear: its second derivative is zero) */
int ganlab_hinge_fwd_f32(const float* x, float* out, int n, float a, float b, void* stream);
int ganlab_hinge_bwd_f32(const float* x, const float* gout, float* gx, int n, float a, float b, void* stream);
/* WGAN-GP style penalty on channel-norms (resnetgan/learner.py:817-825):
 * out[0] = scale * sum_{n,hw} (sqrt(sum_c g^2) - gamma)^2 ;  bwd: gg = gout*scale*2*(s-gamma)*g/s */
int ganlab_chnorm_penalty_fwd_f32(const float* g, float* out, int N, int C, long long HW, float gamma,
                                  float scale, void* workspace, size_t workspace_bytes, void* stream);
int ganlab_chnorm_penalty_bwd_f32(const float* g, const float* gout, float* gg, int N, int C, long long HW,
                                  float gamma, float scale, void* stream);

/* ---- optimiser (torch.optim.Adam as configured by backprop_utils.py:109-120; EWMA progan/learner.py:909-916) */
/* One fused Adam step over a flat parameter arena; bias corrections are passed in by the host. */
int ganlab_adam_f32(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                    float beta2, float eps, float wd, float bc1, float bc2, void* stream);
/* lagged = p*(1-beta) + lagged*beta */
int ganlab_ewma_f32(float* lagged, const float* p, long long n, float beta, void* stream);
/* counter-based N(0,1) generator (Philox4x32-10 + Box-Muller) for latents / per-layer noise */
int ganlab_randn_f32(float* out, long long n, uint64_t seed, uint64_t offset, void* stream);

/* ---- step-graph forms (gan_lab_amd/graphs.py GraphedStep; progan/learner.py:734-943 replayed as HIP graphs) ----
 * A captured launch replays with frozen arguments, so the per-step scalars live in a GANLAB_STEP_SCALARS_BYTES device
 * block: [0,8) the Philox stream position at the start of the replay, floats at byte 16: (lr, 1-beta1^t, 1-beta2^t) of
 * the critic's optimiser, then of the generator's.  One ordinary launch rewrites it before each replay. */
#define GANLAB_STEP_SCALARS_BYTES 64
int ganlab_step_scalars_size(void);
int ganlab_set_step_scalars(void* block, uint64_t rng_base, float f0, float f1, float f2, float f3, float f4, float f5,
                            void* stream);
/* ganlab_randn_f32 at stream position *base + delta (base: device uint64) */
int ganlab_randn_dev_f32(float* out, long long n, uint64_t seed, const void* base, uint64_t delta, void* stream);
/* ganlab_adam_f32 with (lr, bc1, bc2) read from device memory */
int ganlab_adam_dev_f32(float* p, const float* g, float* m, float* v, long long n, const float* lr_bc1_bc2, float beta1,
                        float beta2, float eps, float wd, void* stream);

/* ---- the other fused arena optimisers (csrc/optim.hip; optim.py FusedRMSprop / FusedSGD / FusedOptimisticAdam) ----------
 * One launch over a flat run of n floats each; 16-byte accesses where every buffer is 16-byte aligned, scalar ones for the
 * last n % 4 elements.  No atomics: results are bitwise reproducible.  g' = g + wd p throughout.
 * rmsprop (torch.optim.RMSprop, centered=False): sq = alpha sq + (1 - alpha) g'^2; d = g' / (sqrt(sq) + eps);
 *   momentum > 0: buf = momentum buf + d, p -= lr buf; momentum == 0: p -= lr d and `buf` may be NULL.
 * sgd (torch.optim.SGD, dampening 0, no Nesterov): momentum > 0: buf = first ? g' : momentum buf + g', p -= lr buf;
 *   momentum == 0: p -= lr g' and `buf` may be NULL.
 * oadam (optimistic Adam, Daskalakis et al. 2018, Algorithm 1): m, v, bc1, bc2 as in ganlab_adam_f32;
 *   d = (m / bc1) / (sqrt(v) rsqrt(bc2) + eps); p -= 2 lr d - lr prev; prev = d.
 * The *_dev forms read their per-step scalars from the same 3-float block ganlab_adam_dev_f32 reads:
 *   slot 0 = lr for all three; slots 1, 2 = (bc1, bc2) for oadam; slot 1 = `first` for sgd (1.0 on step 1, else 0.0; slot 2
 *   unused); rmsprop reads slot 0 only. */
int ganlab_rmsprop_f32(float* p, const float* g, float* sq, float* buf, long long n, float lr, float alpha, float eps, float wd,
                       float momentum, void* stream);
int ganlab_rmsprop_dev_f32(float* p, const float* g, float* sq, float* buf, long long n, const float* lr_x_x, float alpha,
                           float eps, float wd, float momentum, void* stream);
int ganlab_sgd_f32(float* p, const float* g, float* buf, long long n, float lr, float wd, float momentum, int first,
                   void* stream);
int ganlab_sgd_dev_f32(float* p, const float* g, float* buf, long long n, const float* lr_first_x, float wd, float momentum,
                       void* stream);
int ganlab_oadam_f32(float* p, const float* g, float* m, float* v, float* prev, long long n, float lr, float beta1, float beta2,
                     float eps, float wd, float bc1, float bc2, void* stream);
int ganlab_oadam_dev_f32(float* p, const float* g, float* m, float* v, float* prev, long long n, const float* lr_bc1_bc2,
                         float beta1, float beta2, float eps, float wd, void* stream);


/* ---- DiffAugment (Zhao et al. 2020): differentiable augmentation of the critic's inputs (csrc/augment.hip) ---------------
 * x, y: (N, 3, H, W), W % 4 == 0, N <= 65535.  params: (N, 8) rows (b, s, c, tx, ty, ox, oy, 0); policy: OR of the bits below,
 * applied in the order color (brightness x + b, saturation around the per-pixel channel mean, contrast around the sample
 * mean), translation by (tx, ty) rows / columns with zero fill, cutout of the ceil(H/2) x ceil(W/2) rectangle centred at
 * (ox, oy).  The color part needs a per-sample reduction: workspace of *_workspace() bytes (0 without color). */
#define GANLAB_DIFFAUG_COLOR 1
#define GANLAB_DIFFAUG_TRANSLATION 2
#define GANLAB_DIFFAUG_CUTOUT 4
/* the (N, 8) parameter rows from the Philox stream: sample n uses counters offset + 2n and offset + 2n + 1, whatever the
 * policy; u = (w >> 8) 2^-24, b = u - 0.5, s = 2u, c = 0.5 + u (rounded down), integers lo + floor(u (hi - lo + 1)) */
int ganlab_diffaug_params_f32(float* out, int N, int H, int W, uint64_t seed, uint64_t offset, void* stream);
/* ganlab_diffaug_params_f32 at stream position *base + delta (base: device uint64) */
int ganlab_diffaug_params_dev_f32(float* out, int N, int H, int W, uint64_t seed, const void* base, uint64_t delta,
                                  void* stream);
size_t ganlab_diffaug_fwd_workspace(int N, int H, int W, int policy);
size_t ganlab_diffaug_bwd_workspace(int N, int H, int W, int policy);
/* y = A(x) */
int ganlab_diffaug_fwd_f32(const float* x, const float* params, float* y, int N, int H, int W, int policy, void* workspace,
                           size_t workspace_bytes, void* stream);
/* gx = A^T(gy): the adjoint of the linear part of A */
int ganlab_diffaug_bwd_f32(const float* gy, const float* params, float* gx, int N, int H, int W, int policy,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- ADA (Karras et al. 2020): adaptive discriminator augmentation of the critic's inputs (csrc/ada.hip) ----------------
 * x, y: (N, 3, H, W), W % 4 == 0, N <= 65535.  params: (N, GANLAB_ADA_ROW) rows - M (6: 2x3, output pixel -> source position in
 * centred pixel units), G (4: the inverse of M[:, :2]), C (12: 3x4 color matrix), then the gate mask and the raw geometric draws
 * (quarter turns, tx, ty, isotropic z, pre-rotation, anisotropic z, post-rotation, shift zx, zy).  The transform is an affine
 * bilinear warp with zero fill followed by the color matrix; the policy only decides which gates the parameter draw may open.
 * state: 4 device floats (p, acc_sum, acc_n, calls) - the augmentation probability and the controller's accumulators. */
#define GANLAB_ADA_BLIT 1
#define GANLAB_ADA_GEOM 2
#define GANLAB_ADA_COLOR 4
#define GANLAB_ADA_ROW 32
#define GANLAB_ADA_COUNTERS 8
/* the parameter rows from the Philox stream: sample n uses counters offset + 8n .. offset + 8n + 7, whatever the policy; p is
 * read from state[0] on the device.  Word-to-parameter mapping: csrc/ada.hip, DESIGN.md "ADA" */
int ganlab_ada_params_f32(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed, uint64_t offset,
                          void* stream);
/* ganlab_ada_params_f32 at stream position *base + delta (base: device uint64) */
int ganlab_ada_params_dev_f32(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed,
                              const void* base, uint64_t delta, void* stream);
/* y = A(x) */
int ganlab_ada_fwd_f32(const float* x, const float* params, float* y, int N, int H, int W, void* stream);
/* gx = A^T(gy): the adjoint of the linear part of A, as a gather (G must be the inverse of M[:, :2]) */
int ganlab_ada_bwd_f32(const float* gy, const float* params, float* gx, int N, int H, int W, void* stream);
/* controller: acc_sum += sum(sign(logits)), acc_n += N, calls += 1; when interval > 0 and calls >= interval:
 * p = clamp(p + sign(acc_sum / acc_n - target) * step_size, 0, 1) and the other three are cleared.  interval <= 0 only
 * accumulates; N == 0 (logits may be null) only counts - together they let a host all-reduce sit between the two. */
int ganlab_ada_update_f32(float* state, const float* logits, int N, int interval, float step_size, float target,
                          void* stream);

/* ---- ADA's image-space groups: filtering, noise, cutout (csrc/ada_filter.hip) -----------------------------
 * Applied after ganlab_ada_fwd_f32: y = cutout(noise(filter(x))).  ext: (N, GANLAB_ADA_EXT_ROW) rows - g (4 band gains), sigma,
 * the cutout rectangle j0, j1, i0, i1 (columns [j0, j1), rows [i0, i1); empty when off), the gate mask (bit b = band b, bit 4 =
 * noise, bit 5 = cutout), the four band z, cx, cy.  The filter is the separable GANLAB_ADA_FILTER_TAPS-tap FIR
 * h = fp32(sum_b g_b F[b]) over the (4, 43) bank F with whole-sample reflection of any depth.  The gate mask decides what acts:
 * the filter runs when a band bit is set, sigma counts with bit 4, the rectangle with bit 5; a row with an empty mask is copied.
 * H >= 2, W % 4 == 0, 3 N <= 65535. */
#define GANLAB_ADA_FILTER 8
#define GANLAB_ADA_NOISE 16
#define GANLAB_ADA_CUTOUT 32
#define GANLAB_ADA_EXT_ROW 16
#define GANLAB_ADA_EXT_COUNTERS 4
#define GANLAB_ADA_FILTER_TAPS 43
/* the library's copy of the bank: 4 x 43 doubles, row-major, into host memory */
int ganlab_ada_filter_bank(double* out);
/* the ext rows from the Philox stream: sample n uses counters offset + 4n .. offset + 4n + 3, where offset is the position
 * right after the batch's main block (the caller adds its 8 N); policy: the whole mask, only the three new bits open gates */
int ganlab_ada_ext_params_f32(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed, uint64_t offset,
                              void* stream);
/* ganlab_ada_ext_params_f32 at stream position *base + delta (base: device uint64) */
int ganlab_ada_ext_params_dev_f32(float* out, int N, int H, int W, const float* state, int policy, uint64_t seed,
                                  const void* base, uint64_t delta, void* stream);
/* y = cutout(x' + sigma * noise), x' = filter(x); noise: (N, 3, H, W) standard normals or null (then none is added); x != y */
int ganlab_ada_ext_fwd_f32(const float* x, const float* ext, const float* noise, float* y, int N, int H, int W, void* stream);
/* gx = F^T (mask o gy): the adjoint as a gather in a fixed order (no atomics; bitwise reproducible); gy != gx */
int ganlab_ada_ext_bwd_f32(const float* gy, const float* ext, float* gx, int N, int H, int W, void* stream);

/* ---- sliced Wasserstein distance between Laplacian-pyramid patch descriptors (Karras et al. 2018; csrc/swd.hip)
 * Planes are fp32, H and W even.  f = [1,4,6,4,1]/16 with mirror boundary (the edge sample is not repeated). */
#define GANLAB_SWD_DESC 147
/* y (planes, H/2, W/2) = (f (x) f)(x)[::2, ::2] */
int ganlab_swd_down_f32(const float* x, float* y, long long planes, int H, int W, void* stream);
/* out (planes, H, W) = g0 - up(g1); g1: (planes, H/2, W/2); up = zeros at the odd positions, then (2f) (x) (2f) */
int ganlab_swd_band_f32(const float* g0, const float* g1, float* out, long long planes, int H, int W, void* stream);
/* band: (N, 3, S, S); pos: (N, n, 2) int32 centres (y, x), clamped to [3, S-4]; desc: (N n, 147) rows in (channel, dy, dx) order
 * (the caller passes the address of its first row); partials: (N, 6) doubles per image - sum of v per channel, then of v^2 */
int ganlab_swd_gather_f32(const float* band, const int* pos, float* desc, double* partials, int N, int n, int S, void* stream);
/* (images, 6) partials -> out[0..2] = per-channel mean, out[3..5] = population standard deviation over images * per_image
 * values per channel; fixed order */
int ganlab_swd_stats_f64(const double* partials, long long images, long long per_image, double* out, void* stream);
/* out (D, M), out[d][m] = sum_k dirs[d][k] (desc[m][k] - mean[c(k)]) / std[c(k)]; desc (M, 147), dirs (D, 147), stats as written
 * by ganlab_swd_stats_f64.  A zero std gives NaN. */
int ganlab_swd_project_f32(const float* desc, const float* dirs, const double* stats, float* out, long long M, int D,
                           void* stream);
/* ascending sort of each of the `segments` rows of an (segments, M) buffer; out must not alias in; segments * M < 2^32 - 1 */
size_t ganlab_swd_sort_workspace(int segments, long long M);
int ganlab_swd_sort_f32(const float* in, float* out, int segments, long long M, void* workspace, size_t workspace_bytes,
                        void* stream);
/* out[0] = sum |a - b| / (D M) over two (D, M) buffers, fp64, fixed order */
size_t ganlab_swd_distance_workspace(int D, long long M);
int ganlab_swd_distance_f64(const float* a, const float* b, double* out, int D, long long M, void* workspace,
                            size_t workspace_bytes, void* stream);
/* (N, n, 2) centres uniform in [3, S-4] from the Philox stream: image i uses counters offset + i ceil(n / 2) .. */
int ganlab_swd_positions_i32(int* out, int N, int n, int S, uint64_t seed, uint64_t offset, void* stream);
/* (D, 147) unit-norm Gaussian directions: direction d uses counters offset + 147 d .. offset + 147 d + 146 */
int ganlab_swd_directions_f32(float* out, int D, uint64_t seed, uint64_t offset, void* stream);

/* ---- multi-scale structural similarity between pairs of images (Wang et al. 2003; the diversity metric of Karras et al. 2018;
 * csrc/msssim.hip).  An evaluation holds P pairs of (3, R, R) fp32 images, R a power of two in [16, 16384], and
 * runs five levels of side S = R >> level.  The window of a level has min(11, S) taps, sigma = 1.5 taps / 11 (computed in double
 * on the host, rounded to fp32), and is applied in valid mode. */
#define GANLAB_MSSSIM_LEVELS 5
#define GANLAB_MSSSIM_WINDOW 11
/* bytes of the per-tile fp64 partials of all five levels of P pairs (0: refused) */
size_t ganlab_msssim_workspace(int P, int R);
/* One level of pairs first .. first + count - 1 of the evaluation: image a of pair first + j starts at a + j pair_stride floats
 * (b likewise; each image is a contiguous (3, S, S) block).  Writes the pairs' (cs, ssim) tile partials into their place in the
 * workspace and, unless next_a / next_b are NULL (they must be at the last level), the 2 x 2 mean ((x00 + x01) + (x10 + x11)) / 4 of
 * both images as (3, S/2, S/2) blocks next_pair_stride floats apart.  c1 = (0.01 L)^2, c2 = (0.03 L)^2. */
int ganlab_msssim_level_f32(const float* a, const float* b, long long pair_stride, float* next_a, float* next_b,
                            long long next_pair_stride, int first, int count, int P, int R, int level, float c1, float c2,
                            void* workspace, size_t workspace_bytes, void* stream);
/* After every level of every pair: table (P, 5, 2) doubles = (CS_i, SSIM_i), the means over channels and pixels clamped below at 0;
 * values (P) = prod_{i<4} CS_i^w_i x SSIM_4^w_4, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); out[0] = mean of values,
 * out[1..4] = mean CS_0..3, out[5] = mean SSIM_4, each summed over the pairs in index order.  fp64, fixed order. */
int ganlab_msssim_finish_f64(const void* workspace, size_t workspace_bytes, int P, int R, double* table, double* values,
                             double* out, void* stream);

/* ---- radial power spectrum of a set of images (Durall et al. 2020, Dzanic et al. 2020; csrc/spectrum.hip).
 * An evaluation holds N (3, R, R) fp32 images, R a power of two in [16, 1024] (any other R: GANLAB_EUNSUPPORTED).  Per image:
 * y = x w[i] w[j] (periodic Hann window, or none), P[u,v] = sum_c |DFT2(y_c)[u,v]|^2 / (3 R^2 W), W = (sum_i w[i]^2 / R)^2, and
 * A[k], k = 0 .. R/2, = the mean of P over the signed frequencies (ku, kv) in [-R/2, R/2)^2 with
 * (2k-1)^2 <= 4 (ku^2 + kv^2) < (2k+1)^2 (bin 0: DC alone).  The FFT is fp32 in LDS, every sum of |F|^2 is fp64 in a fixed order. */
#define GANLAB_SPECTRUM_MIN_RES 16
#define GANLAB_SPECTRUM_MAX_RES 1024
#define GANLAB_SPECTRUM_WINDOW_NONE 0
#define GANLAB_SPECTRUM_WINDOW_HANN 1
/* bytes of the N per-image profiles, (N, R/2 + 1) doubles (0: refused) */
size_t ganlab_spectrum_workspace(int N, int R);
/* bytes of the scratch one feed of count images needs: the window and twiddle tables, the half spectrum (3, R, R/2 + 1) complex
 * fp32 per image between the row and the column pass, and the per-tile fp64 bin sums (0: refused) */
size_t ganlab_spectrum_scratch(int count, int R);
/* Profiles of images first .. first + count - 1 of the evaluation into their rows of the workspace; image j is the contiguous
 * (3, R, R) block at x + j image_stride floats.  The scratch may be reused by the next call on the same stream. */
int ganlab_spectrum_feed_f32(const float* x, long long image_stride, int first, int count, int N, int R, int window,
                             void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* Once all N images are in: out[0 .. R/2] = S[k], the mean of A_n[k] over the images in index order; out[R/2+1 .. R+1] =
 * 10 log10(max(S[k], 1e-30)).  With workspace_b (a second evaluation of N images; else NULL) the same two rows of set b follow,
 * then spectrum = sqrt(mean_{k=1..R/2} (dB_b[k] - dB_a[k])^2) and hf = the same over k = R/4+1 .. R/2: 4 (R/2 + 1) + 2 doubles. */
int ganlab_spectrum_finish_f64(const void* workspace_a, const void* workspace_b, size_t workspace_bytes, int N, int R, double* out,
                               size_t out_bytes, void* stream);

/* ---- the power-spectrum regulariser (Durall et al. 2020; csrc/spectrum.hip): with the set profile S of N images
 * (their per-image profiles in a workspace filled by ganlab_spectrum_feed_f32), a target profile T (R/2 + 1 doubles) and the band
 * B = 1 .. R/2 (ALL) or R/4+1 .. R/2 (HF),  L = mean_{k in B} (ln max(S[k], 1e-30) - ln max(T[k], 1e-30))^2. */
#define GANLAB_SPECTRUM_BAND_ALL 0
#define GANLAB_SPECTRUM_BAND_HF 1
/* loss[0] = L as fp32; coef[k] = dL/dS[k] / (N members_k 3 R^2 W), R/2 + 1 doubles, 0 outside the band and where S[k] <= 1e-30:
 * the weight of every |F_c[u,v]|^2 of bin k in L.  fp64, fixed order. */
int ganlab_spectrum_reg_finish_f64(const void* workspace, size_t workspace_bytes, int N, int R, int window, int band,
                                   const double* target, float* loss, double* coef, void* stream);
/* target[k] = S[k] (first != 0), else decay target[k] + (1 - decay) S[k]; decay in [0, 1) */
int ganlab_spectrum_reg_target_f64(const void* workspace, size_t workspace_bytes, int N, int R, double decay, int first,
                                   double* target, void* stream);
/* bytes of the scratch the backward of count images needs: the tables and the half spectra (0: refused) */
size_t ganlab_spectrum_reg_scratch(int count, int R);
/* dx (count contiguous (3, R, R) blocks) = grad_loss[0] dL/dx of the count images at x + j image_stride: the half spectrum is
 * recomputed, weighted by coef[bin] and transformed back (dy_c = 2 R^2 Re IDFT2(G F_c), dx = dy w[i] w[j]).  grad_loss: one fp32
 * value on the device.  The scratch may be reused by the next call on the same stream. */
int ganlab_spectrum_reg_backward_f32(const float* x, long long image_stride, int count, int R, int window, const double* coef,
                                     const float* grad_loss, float* dx, void* scratch, size_t scratch_bytes, void* stream);

/* ---- real-image input path -----------------------------------------------------------
 * uint8 NHWC dataset images -> 2^k box downsample -> fp32 NCHW ((v/255 - mean[c]) / std[c]); replaces the host
 * chain PIL Image.resize(BOX) -> ToTensor -> Normalize (data_config.py:307-341, progan/learner.py:1099-1112).
 * The uint8 stage is bit-exact with PIL's two-pass rounding for power-of-two factors; `flip` (nullable,
 * one byte per image) mirrors the image horizontally (RandomHorizontalFlip, data_config.py:332-333).
 * GANLAB_EUNSUPPORTED unless factor is a power of two dividing Hs and Ws. */
int ganlab_u8_box_decode_f32(const unsigned char* in_nhwc, float* out_nchw, int N, int Hs, int Ws, int C, int factor,
                             const float* mean, const float* stdv, const unsigned char* flip, void* stream);

/* ---- LeakyReLU masks as bits ------------------------------------------------------------------------------------------
 * The critic's block conv -> bias -> LeakyReLU -> blur (progan/architectures.py:261-284) needs only sign(y) of the LeakyReLU
 * output y in its backward (nn.LeakyReLU backward: grad * (y > 0 ? 1 : slope)): the blur pass that reads y emits the sign
 * bits (bit e of the NCHW-linear element index, 32 per word; W % 32 == 0), the backward passes read 1/32 of the bytes and y
 * itself is not kept. */
int ganlab_mask_bits_supported(int H, int W);
int ganlab_blur3x3_bits_f32(const float* x, float* y, unsigned* bits, long long planes, int H, int W, void* stream);
int ganlab_blur_act_bwd_bits_f32(const float* g, const unsigned* ybits, float* out, float* gb, int N, int C, int H, int W,
                                 float slope, float bias_scale, void* workspace, size_t workspace_bytes, void* stream);
int ganlab_act_bwd_blur_bits_f32(const float* g, const unsigned* ybits, const float* noise, float* out, float* gb,
                                 float* gnw, int N, int C, int H, int W, float slope, float bias_scale, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* fromRGB (1x1, <= 3 input channels, progan/architectures.py:286-292) with its LeakyReLU mask as bits: the forward writes y and
 * the sign bits of y, the gradient kernels of ganlab_conv_{dgrad_act,fwd_mask,wgrad_act}_f32 read the bits instead of y */
int ganlab_conv_fwd_bits_f32(const float* x, const float* wp, const float* bias, float* y, unsigned* ybits,
                             const ganlab_conv_geom* g, float bias_scale, int act, float slope, void* stream);
/* The critic's  conv3x3 -> +bias -> LeakyReLU -> binomial blur  (progan/architectures.py:254-284) of a thin layer (<= 16 -> 16
 * channels, W % 64 == 0, H % 4 == 0) in ONE rolling-window kernel (csrc/conv_roll_blur.hip): y = blur(lrelu(conv + b)) and
 * the sign bits of the un-blurred activation (ybits may be NULL).  wp: GANLAB_PACK_FWD-packed weights. */
int ganlab_conv_fwd_blur_supported(const ganlab_conv_geom* g, const void* x, const void* y);
int ganlab_conv_fwd_blur_bits_f32(const float* x, const float* wp, const float* bias, float* y, unsigned* ybits,
                                  const ganlab_conv_geom* g, float bias_scale, float slope, void* stream);
/* The thin transposed stride-2 conv (32 low-resolution channels -> <= 16 high-resolution ones, Wl % 32 == 0) together with
 * the blur that follows it and what follows the blur (csrc/conv_s2_roll_blur.hip).  `g` is the UP layer (g->up) for the
 * generator's forward tail (stylegan/architectures.py:292-334, 497-526):
 *   y = act(blur(conv(up2(x * aff_s + aff_t), w)) + noise_w[c] * noise[n,hw] + bias[c] * bias_scale), mean / rstd = the
 *   InstanceNorm statistics of y (aff_s / aff_t NULL: plain input; wp: ganlab_conv_s2_pack_f32(up 1, transposed 0));
 * and the POOLED layer (g->pool) for the critic's backward (progan/architectures.py:254-284):
 *   gz = lrelu'(ybits) * blur(dgrad(gy, w)), gb[c] = bias_scale * sum gz (gb may be NULL) - the pooled conv's input gradient
 *   fused with the backward of the LeakyReLU -> blur in front of it (wp: what ganlab_conv_s2_dgrad_f32 takes). */
int ganlab_conv_s2_blur_supported(const ganlab_conv_geom* g);
size_t ganlab_conv_s2_blur_workspace(const ganlab_conv_geom* g);
int ganlab_conv_s2_fwd_blur_tail_f32(const float* x, const float* wp, const float* aff_s, const float* aff_t,
                                     const float* bias, const float* noise, const float* noise_w, float* y, float* mean,
                                     float* rstd, const ganlab_conv_geom* g, float bias_scale, int act, float slope, float eps,
                                     void* workspace, size_t workspace_bytes, void* stream);
int ganlab_conv_s2_dgrad_blur_act_bits_f32(const float* gy, const float* wp, const unsigned* ybits, float* gz, float* gb,
                                           const ganlab_conv_geom* g, float slope, float bias_scale, void* workspace,
                                           size_t workspace_bytes, void* stream);
/* The input gradient of the critic's first 3x3 conv (geometry g, thin: csrc/conv_roll_blur.hip) met by the backward of the
 * fromRGB layer in front of it (1x1 conv of the img_c <= 3 channel image + LeakyReLU, progan/architectures.py:232-237) inside
 * the kernel, for callers that do not need fromRGB's own input gradient: gz = dgrad(gy, w) * lrelu'(ybits) is never written;
 * gw_rgb[co][c] = scale * sum gz[co] * img[c], gb_rgb[co] = bias_scale * sum gz[co] (either may be NULL); acc_w / acc_b: add
 * to what they hold.  wp: what ganlab_conv_dgrad_f32 takes. */
int ganlab_conv_dgrad_rgb_sums_supported(const ganlab_conv_geom* g, int img_c);
size_t ganlab_conv_dgrad_rgb_sums_workspace(const ganlab_conv_geom* g);
int ganlab_conv_dgrad_rgb_sums_f32(const float* gy, const float* wp, const unsigned* ybits, const float* img, float* gw_rgb,
                                   float* gb_rgb, const ganlab_conv_geom* g, int img_c, float scale, float bias_scale,
                                   float slope, int acc_w, int acc_b, void* workspace, size_t workspace_bytes, void* stream);
int ganlab_conv_dgrad_act_bits_f32(const float* gy, const unsigned* ybits, const float* wp, float* gx,
                                   const ganlab_conv_geom* g, float slope, void* stream);
int ganlab_conv_fwd_mask_bits_f32(const float* x, const float* wp, const unsigned* ybits, float* out,
                                  const ganlab_conv_geom* g, float slope, void* stream);
int ganlab_conv_wgrad_act_bits_f32(const float* gy, const unsigned* ybits, const float* x, float* gw, float* gb,
                                   const ganlab_conv_geom* g, float scale, float bias_scale, float slope, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---- all weight re-layouts of a network in ONE launch (csrc/pack.hip) -------------------------------------------------
 * The packed forms ganlab_conv_pack_f32 / ganlab_conv_s2_pack_f32 / ganlab_conv_pack_bf16 produce, rebuilt for a whole
 * table of weights after the optimiser rewrote them (Conv2dEx.forward multiplies by wscale on every call,
 * custom_layers.py:202-211; here the scaled re-layout is cached between optimiser steps).  `descs_device`: device copy of
 * n_desc descriptors sorted by block0.  One thread re-lays out one weight position with all of its taps (36 contiguous
 * source bytes), so descriptor i owns blocks [block0, block0 + ceil(total / taps / 256)) with taps = ks*ks (PLAIN), 16
 * (S2: the K4 taps of the stride-2 kernels) or 9 (BF16). */
#define GANLAB_PACKKIND_PLAIN 0
#define GANLAB_PACKKIND_S2 1
#define GANLAB_PACKKIND_BF16 2
#define GANLAB_PACKKIND_X3 3     /* three-plane bf16 k-step images of csrc/conv_x3.hip (27*Cout*Cin bf16 elements) */
typedef struct ganlab_pack_desc {
  const float* src;      /* OIHW parameter */
  void* dst;             /* packed buffer of `total` elements (float, or bf16 for GANLAB_PACKKIND_BF16 / _X3) */
  int kind;              /* GANLAB_PACKKIND_* */
  int Cout, Cin, ks;
  int mode;              /* PLAIN / BF16: GANLAB_PACK_FWD or _DGRAD; S2: transpose flag */
  int up;                /* S2: 1 = up layer, 0 = down (pooled) layer */
  float scale;
  int reserved;
  long long total;
  long long block0;
} ganlab_pack_desc;
int ganlab_pack_desc_size(void);
int ganlab_pack_many(const ganlab_pack_desc* descs_device, int n_desc, long long total_blocks, void* stream);

/* ---- deferred InstanceNorm: "affine on load" consumers (csrc/mod.hip, template flag AFF in the conv kernels) ------------
 * The generator layer of stylegan/architectures.py:497-526 ends in b = a*s[n,c] + t[n,c] (InstanceNorm + AdaIN of the
 * activated tensor a; custom_layers.py:98-99 + stylegan/architectures.py:524-526).  These entry points let the CONSUMER of
 * b read a instead and apply the per-(sample, channel) affine while the patch goes from registers to LDS - elements in the
 * zero padding of b stay zero.  aff_s / aff_t: [N][Cin] floats.  Replaces the second pass of ganlab_instnorm_style_fwd_f32
 * followed by the plain kernel; the input gradient of such a layer is the plain ganlab_conv_dgrad_f32 / _s2_dgrad_f32 (it is
 * d loss / d b, which the InstanceNorm backward takes). */
/* s = rstd*(ys+1), t = yb - mean*s per (n, c); style = (N, 2C) = [ys | yb] or NULL */
int ganlab_in_affine_f32(const float* mean, const float* rstd, const float* style, float* s, float* t, int N, int C,
                         void* stream);
/* plain 3x3 'same' layer on planes >= 32 wide with more than 16 output channels: bit 0 = forward, bit 1 = weight gradient */
int ganlab_conv_aff_supported(const ganlab_conv_geom* g);
/* ganlab_conv_fwd_f32 on b = a*s + t */
int ganlab_conv_fwd_aff_f32(const float* x, const float* wp, const float* aff_s, const float* aff_t, const float* bias,
                            float* y, const ganlab_conv_geom* g, float bias_scale, int act, float slope, void* stream);
/* ganlab_conv_wgrad_f32 with b = a*s + t as the x operand (workspace: ganlab_conv_wgrad_workspace) */
/* The same layer one size up: a plain 3x3 generator layer (Cout > 16, W % 32 == 0, H % 8 == 0) with a deferred-InstanceNorm
 * input and its whole tail in the conv kernel's epilogue (stylegan/architectures.py:497-526): y = act(conv(x * aff_s + aff_t, w)
 * + noise_w * noise + bias * bias_scale), mean / rstd = InstanceNorm statistics of y.  ganlab_conv_fwd_aff_tail_chunks: tiles
 * per plane (workspace: N * Cout * tiles * 2 doubles), 0 where the form does not apply. */
int ganlab_conv_fwd_aff_tail_chunks(const ganlab_conv_geom* g);
int ganlab_conv_fwd_aff_tail_f32(const float* x, const float* wp, const float* aff_s, const float* aff_t, const float* bias,
                                 const float* noise, const float* noise_w, float* y, float* mean, float* rstd,
                                 const ganlab_conv_geom* g, float bias_scale, int act, float slope, float eps, void* workspace,
                                 size_t workspace_bytes, void* stream);
int ganlab_conv_wgrad_aff_f32(const float* gy, const float* x, const float* aff_s, const float* aff_t, float* gw,
                              const ganlab_conv_geom* g, float scale, void* workspace, size_t workspace_bytes, void* stream);
/* Upsample + conv3x3 (up = 1) with a deferred low-resolution input: bit 0 = forward, bit 1 = weight gradient */
int ganlab_conv_s2_aff_supported(const ganlab_conv_geom* g);
int ganlab_conv_s2_fwd_aff_f32(const float* x, const float* wp, const float* aff_s, const float* aff_t, const float* bias,
                               float* y, const ganlab_conv_geom* g, float bias_scale, int act, float slope, void* stream);
int ganlab_conv_s2_wgrad_aff_f32(const float* gy, const float* x, const float* aff_s, const float* aff_t, float* gw,
                                 const ganlab_conv_geom* g, float scale, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* thin 3x3 layer (Cin, Cout <= 16, W % 64 == 0, H % 4 == 0) that also finishes itself */
int ganlab_mod_conv_supported(const ganlab_conv_geom* g);
/* statistics chunks per (n, co) plane written by the forward: workspace = N*Cout*chunks*2 doubles */
int ganlab_mod_conv_stat_chunks(const ganlab_conv_geom* g);
/* y = act(conv(a*s + t, w) + bias*bias_scale + noise_w*noise) and, when mean / rstd are given, the InstanceNorm statistics
 * (biased variance, eps) of y from the same pass.  wp: ganlab_conv_pack_f32(GANLAB_PACK_FWD); aff_s / aff_t NULL: plain input. */
int ganlab_mod_conv_fwd_f32(const float* x, const float* wp, const float* aff_s, const float* aff_t, const float* bias,
                            const float* noise, const float* noise_w, float* y, float* mean, float* rstd,
                            const ganlab_conv_geom* g, float bias_scale, int act, float slope, float eps,
                            void* workspace, size_t workspace_bytes, void* stream);
/* toRGB (1x1, linear) of a deferred tensor: weff[n][ci][4] = scale*w[co][ci]*s[n,ci], beff[n][4] = bias*bias_scale + scale*w.t */
int ganlab_mod_torgb_prep_f32(const float* w, const float* bias, const float* s, const float* t, float* weff, float* beff,
                              int N, int Cin, int Cout, float scale, float bias_scale, void* stream);
/* gw (Cout, Cin) / gb (Cout) (either may be NULL) from ganlab_mod_torgb_cross_f32's N x 68 sums */
int ganlab_mod_torgb_wgrad_f32(const float* cross, const float* s, const float* t, float* gw, float* gb, int N, int Cin,
                               int Cout, float scale, float bias_scale, void* stream);
/* y[n,co] = sum_ci weff[n][ci][4] * x[n,ci] + beff[n][4]   (Cout <= 4) */
int ganlab_mod_torgb_fwd_f32(const float* x, const float* weff, const float* beff, float* y, int N, int Cin, int Cout,
                             long long HW, void* stream);
size_t ganlab_mod_torgb_cross_workspace(int N);
/* out[n][68]: [ci 16][4] = sum_px x[n,ci]*gy[n,co], then [64 + co] = sum_px gy[n,co]   (Cin <= 16, Cout <= 4) */
int ganlab_mod_torgb_cross_f32(const float* x, const float* gy, float* out, int N, int Cin, int Cout, long long HW,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- spectral normalisation of every weight of a critic, batched over the layers (csrc/spectral.hip) -------------------
 * torch.nn.utils.spectral_norm with one power iteration, for a parameter W viewed as Wm = (R, K) row-major:
 *   iterate:  t = Wm^T u ; v = t / max(|t|, eps) ; s = Wm v ; u = s / max(|s|, eps)
 *   always:   sigma = u^T Wm v ; W_sn = W / sigma
 *   backward: gW += (g_sn - <g_sn, W_sn> u v^T) / sigma            (u, v constants; accumulates)
 * `jobs_device`: device copy of n_layers jobs.  Every pointer is 16-byte aligned; w, w_sn, g_sn, gw hold R*K floats, u R,
 * v K, sigma 1; scratch: tpart ceil(R / GANLAB_SN_ROW_CHUNK) * K floats, s R, dpart ceil(R*K / GANLAB_SN_ELEM_BLOCK).
 * Job i owns, in its three block spaces, blocks [blk_t0, +ceil(R / ROW_CHUNK) * ceil(K / COL_TILE)), [blk_s0, +ceil(R / 4))
 * and [blk_e0, +ceil(R*K / ELEM_BLOCK)); jobs are sorted by each of them and blocks_t / blocks_s / blocks_e are the totals.
 * Launches per call: 4 (iterate) or 2 for a refresh, 2 for the backward, whatever n_layers is.  Fixed-order sums, no
 * atomics: bitwise reproducible.  Nothing is read back by the host (graph-capturable). */
#define GANLAB_SN_ROW_CHUNK 16
#define GANLAB_SN_COL_TILE 1024
#define GANLAB_SN_ELEM_BLOCK 2048
typedef struct ganlab_sn_job {
  const float* w;        /* the parameter (R*K floats, OIHW or (out, in)) */
  float* w_sn;           /* W / sigma: what the convolutions / linears read */
  const float* g_sn;     /* d loss / d W_sn */
  float* gw;             /* the parameter's gradient slot: accumulated into */
  float* u;
  float* v;
  float* sigma;
  float* tpart;
  float* s;
  float* dpart;
  int R, K;
  long long blk_t0, blk_s0, blk_e0;
} ganlab_sn_job;
int ganlab_sn_job_size(void);
int ganlab_sn_refresh(const ganlab_sn_job* jobs_device, int n_layers, long long blocks_t, long long blocks_s,
                      long long blocks_e, int iterate, float eps, void* stream);
int ganlab_sn_backward(const ganlab_sn_job* jobs_device, int n_layers, long long blocks_e, void* stream);

/* ---- BigGAN orthogonal regularisation of every weight of a network, batched over the layers (csrc/ortho.hip)
 * Brock et al. 2019, eq. 3, for a parameter W viewed as Wm = (R, K) row-major, M = (Wm Wm^T) o (1 - I):
 *   penalty = beta * sum(M^2) ;  gW += 4 * beta * M Wm            (the true derivative of the penalty; accumulates)
 * computed through the association with the smaller middle dimension m = min(R, K):
 *   GANLAB_ORTHO_ROW (R <= K): S = Wm Wm^T (R, R), diagonal zeroed at the store ; G = S Wm ; sum(M^2) = sum(S^2)
 *   GANLAB_ORTHO_COL (K <  R): S = Wm^T Wm (K, K), q[r] = |Wm[r,:]|^2 ; G = Wm S - q o Wm ; sum(M^2) = sum(S^2) - sum(q^2)
 * Both products run on the exact-fp32 MFMA over GANLAB_ORTHO_TILE^2 output tiles, operands staged through LDS and zero-padded at
 * the tails.  A layer with R == 1 has no off-diagonal element: the caller leaves it out of the table.
 * `jobs_device`: device copy of n_layers jobs.  Every pointer is 16-byte aligned; w and gw hold R*K floats, s m*m, q R (column
 * form; unused in row form), penalty 1, part n_part = T*T (+ ceil(R / GANLAB_ORTHO_QROWS) in column form) with
 * T = ceil(m / GANLAB_ORTHO_TILE).  Job i owns blocks [blk_g0, +n_part) of the Gram pass and [blk_a0, +ceil(R / TILE) * ceil(K / TILE))
 * of the apply pass; jobs are sorted by both and blocks_gram / blocks_apply are the totals.  3 launches whatever n_layers is
 * (Gram, apply, a one-block tail that adds the partials in index order into every job's `penalty` and into `total_out`, both
 * already times beta).  Fixed-order sums, no atomics: bitwise reproducible.  Nothing is read back by the host (graph-capturable). */
#define GANLAB_ORTHO_TILE 64
#define GANLAB_ORTHO_QROWS 4
#define GANLAB_ORTHO_ROW 0
#define GANLAB_ORTHO_COL 1
typedef struct ganlab_ortho_job {
  const float* w;        /* the parameter (R*K floats): read only */
  float* gw;             /* the parameter's gradient slot: accumulated into */
  float* s;              /* scratch: the m x m Gram matrix */
  float* q;              /* scratch, column form: squared row norms (R) */
  float* part;           /* scratch: n_part partial sums of the Gram pass */
  float* penalty;        /* out: beta * sum(M^2) of this layer */
  int R, K, form, n_part;
  long long blk_g0, blk_a0;
} ganlab_ortho_job;
int ganlab_ortho_job_size(void);
int ganlab_ortho_apply(const ganlab_ortho_job* jobs_device, int n_layers, long long blocks_gram, long long blocks_apply,
                       float beta, float* total_out, void* stream);

/* ---- SAGAN self-attention (Zhang et al. 2019; csrc/attention.hip) ----------------------------------------------
 * Channel-major operands as the 1x1 convolutions leave them: q (N, Dk, L), k (N, Dk, S), v (N, Dv, S); no 1/sqrt(d) scale.
 *   P[n,l,:] = softmax_s(sum_d q[n,d,l] k[n,d,s]) ; o[n,c,l] = sum_s v[n,c,s] P[n,l,s] ; lse[n,l] = logsumexp_s
 * fwd: one flash-style kernel on the exact-fp32 MFMA (online max / sum over key tiles) writes o (N, Dv, L) and lse (N, L);
 * nothing of size L x S is written.  bwd (first order): from q, k, v, o, lse, d_o it recomputes P per tile and writes dq, dk, dv
 * in three launches (D = rowsum(d_o * o) into the workspace; dq parallel over query tiles; dk, dv parallel over key tiles).
 * No atomics, fixed summation order: bitwise reproducible.  Stream-ordered, nothing is read back by the host.
 * Supported (ganlab_attn_supported): Dk % 4 == 0 in [4, 64], Dv % 16 == 0 in [16, 256], any N, L, S >= 1 (tails masked);
 * anything else returns GANLAB_EUNSUPPORTED. */
int ganlab_attn_supported(int N, int Dk, int Dv, int L, int S);
int ganlab_attn_fwd_f32(const float* q, const float* k, const float* v, float* o, float* lse, int N, int Dk, int Dv, int L,
                        int S, void* stream);
size_t ganlab_attn_bwd_workspace(int N, int L);
int ganlab_attn_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* d_o,
                        float* dq, float* dk, float* dv, int N, int Dk, int Dv, int L, int S, void* workspace,
                        size_t workspace_bytes, void* stream);
/* 2x2 max pool of `planes` (H, W) planes, H and W even (else GANLAB_EINVAL): y (planes, H/2, W/2) and a 2-bit argmax per output
 * (2 * dy + dx; on a tie the first of the four in row-major order, as in ATen), four outputs of the flat index per byte:
 * ganlab_maxpool2x2_bits_bytes bytes.  bwd is a gather: every input element reads its output's code. */
size_t ganlab_maxpool2x2_bits_bytes(long long planes, int H, int W);
int ganlab_maxpool2x2_f32(const float* x, float* y, void* bits, long long planes, int H, int W, void* stream);
int ganlab_maxpool2x2_bwd_f32(const float* gy, const void* bits, float* gx, long long planes, int H, int W, void* stream);
/* out = x + gamma[0] * y, gamma a one-element device tensor (its backward: dx = g, dy = ganlab_scale_dev_f32, dgamma =
 * ganlab_dot_f32(g, y)) */
int ganlab_gated_residual_f32(const float* x, const float* y, const float* gamma, float* out, long long n, void* stream);
/* out[0] = sum_i a[i] b[i]: fp64 products and partials, block partials added in index order */
size_t ganlab_dot_workspace(long long n);
int ganlab_dot_f32(const float* a, const float* b, float* out, long long n, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- class conditioning of the ResNet GAN (config.cgan = 'projection'; csrc/cond.hip) --------------------------
 * labels: int32 (N,) on the device; every kernel clamps them into [0, K) before indexing a (K, .) table.  No atomics, fixed
 * summation order (n ascending): bitwise reproducible.  Stream-ordered, nothing is read back by the host.
 * Conditional BatchNorm, weight / bias (K, C); mean / rstd (C): the batch statistics of ganlab_bn_stats_f32 +
 * ganlab_bn_finalize_f32(weight = NULL), or the running ones (eval mode).
 *   cbn_apply: y[n,c,:] = act((x - mean[c]) * (rstd[c] * weight[l_n,c]) + bias[l_n,c])   (bn_apply's centred form: a table of
 *              equal rows gives ganlab_bn_apply_f32's bits)
 *   cbn_bwd:   gz = gy * lrelu'(yact) (yact / gz both NULL: gz = gy); sums[c] = {sum ghat, sum ghat * xhat}, ghat = gz *
 *              weight[l_n,c]; gb[k,c] = sum_{n: l_n = k} sum_hw gz, gw[k,c] likewise of gz * xhat (every row written, zeros for
 *              an absent class); gx (may be NULL) = rstd[c] * (ghat - s0/L - xhat * s1/L), L = N*HW - with batch_stats = 0
 *              (eval mode) gx = rstd[c] * ghat.  Three launches; workspace ganlab_cbn_bwd_workspace(N, C) bytes (fp64 plane sums) */
int ganlab_cbn_apply_f32(const float* x, const float* mean, const float* rstd, const float* weight, const float* bias,
                         const int* labels, float* y, int N, int C, long long HW, int K, int act, float slope, void* stream);
size_t ganlab_cbn_bwd_workspace(int N, int C);
int ganlab_cbn_bwd_f32(const float* gy, const float* x, const float* mean, const float* rstd, const float* weight,
                       const int* labels, const float* yact, float* gz, float* gx, float* gw, float* gb, float* sums, int N,
                       int C, long long HW, int K, int batch_stats, float slope, void* workspace, size_t workspace_bytes,
                       void* stream);
/* The projection critic's class term, weight (K, F), f (N, F); three kernels that are each other's derivatives:
 *   proj_fwd:     out[n] = base[n] + sum_j weight[l_n,j] f[n,j]       (base may be NULL: 0)
 *   proj_dfeat:   out[n,j] = g[n] weight[l_n,j]
 *   proj_dweight: out[k,j] = sum_{n: l_n = k} g[n] f[n,j]             (every row written) */
int ganlab_proj_fwd_f32(const float* f, const float* weight, const int* labels, const float* base, float* out, int N,
                        long long F, int K, void* stream);
int ganlab_proj_dfeat_f32(const float* g, const float* weight, const int* labels, float* out, int N, long long F, int K,
                          void* stream);
int ganlab_proj_dweight_f32(const float* g, const float* f, const int* labels, float* out, int N, long long F, int K,
                            void* stream);
/* n integers uniform in [0, high), high <= 2^24, from the Philox stream: element e is word e % 4 of counter offset + e / 4 */
int ganlab_randint_i32(int* out, long long n, int high, uint64_t seed, uint64_t offset, void* stream);

/* ---- BigGAN hierarchical latents + shared class embedding for the ResNet GAN generator (config.hier_latent /
 * config.shared_embed; csrc/hier.hip).  No atomics, fixed summation order: bitwise reproducible.  Stream-ordered,
 * nothing is read back by the host (graph-capturable); the job table is uploaded once.
 * Modulation, batched over the linears of every norm: z (N, Lz) (NULL when Lz = 0), shared (K, E) and labels int32 (N,) (both
 * NULL when E = 0; labels are clamped into [0, K)).  Job j is a bias-free linear w (C, D = z_len + E) reading
 * cond[n,:] = [z[n, z_off : z_off + z_len], shared[l_n,:]], which is never materialised:
 *   hier_fwd: out[n, col + c] = one + scale * <w[c,:], cond[n,:]> into the (N, T) buffer `out`; one launch.  Job j owns blocks
 *             [blk_f0, + ceil(C / 64)) of grid.x; jobs are sorted by blk_f0 and blk_w0, blocks_fwd / blocks_dw are the totals.
 *   hier_bwd: from g (N, T): every job's dW[c,d] = scale * sum_n g[n, col + c] cond[n,d] WRITTEN to its `gw` (own_slots = 0)
 *             or `gw_own` (own_slots = 1) - job j owns blocks [blk_w0, + ceil(C * D / 256)); dz (N, Lz) (may be NULL), zero where
 *             no job reads z; dshared (K, E) (may be NULL; needs the (N, E) scratch `de`), every row written.  At most three
 *             launches whatever n_jobs is.
 * The caller guarantees z_off + z_len <= Lz and col + C <= T for every job. */
typedef struct ganlab_hier_job {
  const float* w;        /* the parameter (C * D floats): read only */
  float* gw;             /* its gradient slot in the arena (may be NULL: own_slots = 1 only) */
  float* gw_own;         /* its gradient slot in the table's own buffer */
  int C, z_off, z_len, col;
  float scale, one;
  long long blk_f0, blk_w0;
} ganlab_hier_job;
int ganlab_hier_job_size(void);
int ganlab_hier_fwd_f32(const ganlab_hier_job* jobs_device, int n_jobs, long long blocks_fwd, const float* z,
                        const float* shared, const int* labels, float* out, int N, long long T, int Lz, int E, int K,
                        void* stream);
int ganlab_hier_bwd_f32(const ganlab_hier_job* jobs_device, int n_jobs, long long blocks_dw, const float* g, const float* z,
                        const float* shared, const int* labels, float* dz, float* de, float* dshared, int N, long long T,
                        int Lz, int E, int K, int own_slots, void* stream);
/* Modulated BatchNorm: ganlab_cbn_* with per-sample rows instead of class tables.  gain / shift are (N, C) with row strides
 * (floats; views into the (N, T) buffer above), mean / rstd as for ganlab_cbn_apply_f32.
 *   mbn_apply: y[n,c,:] = act((x - mean[c]) * (rstd[c] * gain[n,c]) + shift[n,c])    (equal rows give ganlab_bn_apply_f32's bits)
 *   mbn_bwd:   as ganlab_cbn_bwd_f32 with ghat = gz * gain[n,c]; dshift[n,c] = sum_hw gz and dgain[n,c] = sum_hw gz * xhat are
 *              written with row stride grad_stride (both may be NULL).  Three launches; workspace ganlab_mbn_bwd_workspace. */
int ganlab_mbn_apply_f32(const float* x, const float* mean, const float* rstd, const float* gain, long long gain_stride,
                         const float* shift, long long shift_stride, float* y, int N, int C, long long HW, int act,
                         float slope, void* stream);
size_t ganlab_mbn_bwd_workspace(int N, int C);
int ganlab_mbn_bwd_f32(const float* gy, const float* x, const float* mean, const float* rstd, const float* gain,
                       long long gain_stride, const float* yact, float* gz, float* gx, float* dgain, float* dshift,
                       long long grad_stride, float* sums, int N, int C, long long HW, int batch_stats, float slope,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- the sampling side of the ResNet GAN: truncated-normal latents, the moving average of the averaged generator's BatchNorm
 * buffers (config.use_ewma_gen / config.truncation; csrc/sample.hip).  No atomics, every element a pure function
 * of its own inputs: bitwise reproducible whatever the launch geometry.  Stream-ordered, nothing is read back by the host.
 *   trunc_randn: n draws of the standard normal truncated to [-threshold, threshold] (threshold finite and > 0) by inverse CDF.
 *             Element i takes word i % 4 of Philox counter offset + i / 4 - the counters of ganlab_randn_f32, ceil(n / 4) of them:
 *             u = ((word >> 9) + 1/2) 2^-23 in (0, 1), x = sqrt(2) erfinv((2u - 1) erf(threshold / sqrt(2))), clamped to
 *             [-threshold, threshold].
 *   ewma_many: dst[i] = decay * dst[i] + (1 - decay) * src[i] (fp64 arithmetic, rounded once) for i < count of every job of the
 *             device-resident table, 0 <= decay < 1, n_jobs <= 65535; one launch.  decay = 0 copies src and does not read dst.
 *             dst and src of a job do not overlap; no two jobs share a dst. */
int ganlab_trunc_randn_f32(float* out, long long n, float threshold, uint64_t seed, uint64_t offset, void* stream);
typedef struct ganlab_ewma_job {
  float* dst;            /* the average: read (decay > 0) and written */
  const float* src;      /* the live values: read only */
  long long count;       /* floats */
} ganlab_ewma_job;
int ganlab_ewma_job_size(void);
int ganlab_ewma_many_f32(const ganlab_ewma_job* jobs_device, int n_jobs, float decay, void* stream);

/* ---- k-nearest-neighbour precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) between two
 * sets of fp32 feature rows (csrc/prdc.hip; composed in gan_lab_amd/prdc.py).  Rows are (rows, D) row-major, any
 * D >= 1, at most 2^30 rows (more: GANLAB_EUNSUPPORTED).  Squared distances are max(|q|^2 + |k|^2 - 2 q.k, 0) with the product on the
 * exact-fp32 MFMA; no N x M matrix is ever stored.  No atomics, nothing is read back by the host, stream-ordered, bitwise
 * reproducible.
 *   norms: out[i] = |x_i|^2, summed in fp64 in a fixed order and rounded once.
 *   knn:   out (N, k): per row the k smallest squared distances to the other rows of x, ascending; the row itself is excluded by
 *          index (a duplicate at another index counts).  1 <= k <= GANLAB_PRDC_MAX_K, k < N.  norms: ganlab_prdc_norms_f32 of x.
 *   cross: per query row j of (M, D) against the keys (N, D): count[j] = #{i: d2(j, i) <= radius}, the radius being radii[i] (N of
 *          them, radius_of_query = 0) or radii[j] (M of them, radius_of_query = 1); dmin[j] = min_i d2(j, i) and imin[j] its index,
 *          the lowest index of a tie. */
#define GANLAB_PRDC_MAX_K 16
int ganlab_prdc_norms_f32(const float* x, float* out, long long rows, int D, void* stream);
int ganlab_prdc_knn_f32(const float* x, const float* norms, float* out, long long N, int D, int k, void* stream);
int ganlab_prdc_cross_f32(const float* queries, const float* query_norms, const float* keys, const float* key_norms,
                          const float* radii, int radius_of_query, int* count, float* dmin, int* imin, long long M, long long N,
                          int D, void* stream);

/* ---- consistency regularisation of the ResNet GAN: bCR (Zhang et al. 2020) and zCR (Zhao et al. 2020) (config.cr_*;
 * csrc/cr.hip; composed in gan_lab_amd/consistency.py).  No atomics, every sum in a fixed order: bitwise
 * reproducible.  Stream-ordered, graph-capturable, nothing is read back by the host.
 *   cr_params:    row n of the (N, 4) int32 table = (flip, dx, dy, 0) from ONE Philox counter, offset + n (+ *base when base is not
 *                 NULL: the step-scalar block of a captured step): flip in {0, 1} (always 0 when `flip` is 0), dx, dy uniform
 *                 integers in [-shift, shift].  out is 16-byte aligned.
 *   cr_transform: y[n,c,i,j] = x[n,c,i-dy, f(j-dx)] with f(k) = W-1-k when the row's flip is set, else k, and 0 where i-dy or j-dx
 *                 leaves the image; any N, C, H, W >= 1; x and y do not overlap.  Values are moved or zeroed: bit-exact.
 *   cr_msd:       out[0] = (1/N) sum_n (a_n - b_n)^2: fp32 differences squared in fp32, summed in fp64 in a fixed order, rounded
 *                 once; one launch.  bwd: ga = (2/N)(a - b) gout[0], gb = -ga; one launch.
 *   cr_imsd:      the same mean over the n elements of two equal-shaped image batches; the forward keeps one fp64 partial per
 *                 workgroup in the workspace (ganlab_cr_imsd_workspace(n) bytes, 8-byte aligned) and a second one-workgroup launch
 *                 adds them in index order; the value does not depend on the operands' alignment.  bwd: one launch reads a and b
 *                 and writes ga and gb, which may be the two halves of one tensor (as a and b may be). */
int ganlab_cr_params_i32(int* out, int N, int shift, int flip, uint64_t seed, uint64_t offset, const void* base, void* stream);
int ganlab_cr_transform_f32(const float* x, const int* params, float* y, int N, int C, int H, int W, void* stream);
int ganlab_cr_msd_fwd_f32(const float* a, const float* b, float* out, int N, void* stream);
int ganlab_cr_msd_bwd_f32(const float* a, const float* b, const float* gout, float* ga, float* gb, int N, void* stream);
size_t ganlab_cr_imsd_workspace(long long n);
int ganlab_cr_imsd_fwd_f32(const float* a, const float* b, float* out, long long n, void* workspace, size_t workspace_bytes,
                           void* stream);
int ganlab_cr_imsd_bwd_f32(const float* a, const float* b, const float* gout, float* ga, float* gb, long long n, void* stream);

/* ---- Frechet distance and Kernel Inception Distance (Binkowski et al. 2018) between two sets of fp32 feature rows of any
 * embedding (csrc/frechet.hip, csrc/kid.hip; composed in gan_lab_amd/frechet.py and gan_lab_amd/kid.py).  Rows are
 * (rows, D) row-major.  Products on the exact-fp32 MFMA in chains of at most 64 terms (moments: 32), every longer sum in float64; no atomics,
 * nothing is read back by the host, stream-ordered, bitwise reproducible.  A bad argument returns GANLAB_EINVAL.
 *   moments_accum: sum[a] += sum_i (x_ia - c_a), gram[a][b] += sum_i (x_ia - c_a)(x_ib - c_b) over the n rows, c = pivot (D,) fp32,
 *                  subtracted in fp32 on load; sum (D,) and gram (D, D) are float64 and accumulated into: zero them before the
 *                  first launch.  gram is written in full (upper tiles and their mirrors) and stays exactly symmetric.
 *                  1 <= D <= 4096, 1 <= n <= 2^30.
 *   kid_rowsums:   out[i] = sum_j (gamma q_i.k_j + coef0)^3 over the N keys, for the M queries; out (M,) float64.
 *                  t = fmaf(gamma, dot, coef0) in fp32, its cube and the sums in float64.  exclude_diag = 1 leaves j == i out by
 *                  index (a duplicate row at another index counts) and requires M == N.  D >= 1, at most 2^30 rows per set. */
int ganlab_moments_accum_f32(const float* rows, long long n, int D, const float* pivot, double* sum, double* gram, void* stream);
int ganlab_kid_rowsums_f32(const float* q, long long M, const float* keys, long long N, int D, float gamma, float coef0,
                           int exclude_diag, double* out, void* stream);

/* ---- classifier-based class conditioning of the ResNet GAN critic: AC-GAN's cross-entropy (Odena et al. 2017), ContraGAN's
 * conditional contrastive loss 2C (Kang & Park 2020), ReACGAN's data-to-data cross-entropy D2D-CE (Kang et al. 2021)
 * (config.cgan = 'acgan' | 'contra' | 'reacgan'; csrc/cond_loss.hip; composed in gan_lab_amd/conditional.py).
 * labels: int32 (N,), clamped into [0, K).  Every loss is the mean over rows; gout is the device scalar cotangent of that mean.  No
 * atomics, every sum in a fixed order: bitwise reproducible.  Stream-ordered, graph-capturable, nothing is read back by the host.
 * 1 <= N <= 8192, 2 <= K <= 65536, 1 <= E <= 1024; outside: GANLAB_EUNSUPPORTED.
 *   class_ce:  z (N, K) logits.  fwd: loss[0] = mean_i (lse_i - z[i, y_i]), lse (N,) saved for the backward; one launch (one
 *              workgroup).  bwd: dz[i,k] = gout[0]/N (exp(z[i,k] - lse_i) - [k == y_i]); one launch.
 *   cl:        h (N, E) embeddings, proxy (K, E); both are normalised to unit rows (norm floor 1e-12) inside.  mode 0 = 2C,
 *              1 = D2D-CE (margin_pos, margin_neg; ignored by 2C); temperature > 0.  fwd: rows (4, N) = the per-row loss, D_i, M_i
 *              (2C; D2D-CE: u_i) and s_i, loss[0] their mean; two launches.  bwd: dh (N, E), dproxy (K, E), every row written
 *              (exact zeros for a class absent from the batch); workspace ganlab_cl_bwd_workspace(N, E, K) bytes, 4-byte aligned;
 *              three launches.  The derivative of a clamp is 0 at its kink. */
int ganlab_class_ce_fwd_f32(const float* z, const int* labels, float* loss, float* lse, int N, int K, void* stream);
int ganlab_class_ce_bwd_f32(const float* z, const int* labels, const float* lse, const float* gout, float* dz, int N, int K,
                            void* stream);
int ganlab_cl_supported(int N, int E, int K);
int ganlab_cl_fwd_f32(const float* h, const float* proxy, const int* labels, float* loss, float* rows, int N, int E, int K,
                      int mode, float temperature, float margin_pos, float margin_neg, void* stream);
size_t ganlab_cl_bwd_workspace(int N, int E, int K);
int ganlab_cl_bwd_f32(const float* h, const float* proxy, const int* labels, const float* rows, const float* gout, float* dh,
                      float* dproxy, int N, int E, int K, int mode, float temperature, float margin_pos, float margin_neg,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- projection of images into StyleGAN's latent space, W or W+ (csrc/project.hip; composed in
 * gan_lab_amd/project.py).  No atomics, every sum in a fixed order: bitwise reproducible.  Stream-ordered, nothing is read back by
 * the host.
 *   pyramid_mse:  x, t (N, C, R, R) fp32, 16-byte aligned; R a power of two in [4, 1024]; `weights`: `levels` non-negative HOST
 *                 floats, 1 <= levels <= min(6, log2(R) + 1).  d_0 = x - t, d_{l+1} = the 2x2 mean of d_l (fp32):
 *                 terms[n, l] = mean_{c,h,w} d_l[n]^2 (squares and sums in fp64, rounded once), loss[n] = sum_l weights[l]
 *                 terms[n, l] (from the fp64 terms), g = d loss[n] / d x = 2 / (C R^2) sum_l weights[l] up_l(d_l).  Two launches:
 *                 one workgroup per 32x32 tile of a plane (the plane below 32x32) reads x and t once, writes g once and one fp64
 *                 partial per (tile, level) into the workspace (ganlab_pyramid_mse_workspace bytes, 8-byte aligned); one
 *                 workgroup per sample adds them in index order.  Outside the ranges: GANLAB_EUNSUPPORTED.
 *   scale_rows:   out[n, :] = g[n, :] * s[n] over N rows of `per` floats (per % 4 == 0, 16-byte aligned); out is not g.
 *   w_moments:    ws (M, D): w_avg[d] = mean_i ws[i, d], w_std[0] = sqrt(sum_{i,d} (ws[i, d] - mean_d)^2 / M) - the StyleGAN2
 *                 projector's definition; two passes in fp64; workspace ganlab_w_moments_workspace(D) bytes, 8-byte aligned.
 *   project_step: one launch of one workgroup.  step[0] = k, the device-resident iteration count; hyper = 6 HOST doubles (lr0,
 *                 initial_noise_factor, lr_rampdown_length, lr_rampup_length, noise_ramp_length, num_steps).  With t = k /
 *                 num_steps: lr = lr0 (0.5 - 0.5 cos(pi min(1, (1 - t) / rampdown))) min(1, t / rampup); the gradient is
 *                 grad_ws (N, L, D) itself (w_plus = 1; w_opt, m, v, noise are (N, L, D)) or its sum over L in layer order
 *                 (w_plus = 0; they are (N, D)); Adam's update number k + 1 (betas 0.9 / 0.999, eps 1e-8, bias-corrected) of
 *                 w_opt, m, v; step[0] = k + 1; w_in (N, L, D) = w_opt + w_std[0] initial_noise_factor max(0, 1 - t' /
 *                 noise_ramp)^2 noise at t' = (k + 1) / num_steps, broadcast over L when w_plus = 0.  grad_ws = NULL: no update,
 *                 step[0] stays, w_in is written at t' = k / num_steps (the first forward's input). */
#define GANLAB_PYRAMID_MAX_LEVELS 6
size_t ganlab_pyramid_mse_workspace(int N, int C, int R, int levels);
int ganlab_pyramid_mse_f32(const float* x, const float* t, const float* weights, int levels, float* g, float* loss, float* terms,
                           int N, int C, int R, void* workspace, size_t workspace_bytes, void* stream);
int ganlab_scale_rows_f32(const float* g, const float* s, float* out, int N, long long per, void* stream);
size_t ganlab_w_moments_workspace(int D);
int ganlab_w_moments_f32(const float* ws, float* w_avg, float* w_std, long long M, int D, void* workspace, size_t workspace_bytes,
                         void* stream);
int ganlab_project_step_f32(float* w_opt, const float* grad_ws, float* m, float* v, int* step, const float* noise,
                            const float* w_std, float* w_in, int N, int L, int w_plus, int D, const double* hyper, void* stream);

/* ---- perceptual path length (csrc/ppl.hip; composed in gan_lab_amd/ppl.py).  No atomics, every sum in a fixed
 * order: bitwise reproducible.  Stream-ordered; the host reads nothing back.  Every argument is checked before any launch.
 *   ppl_endpoints: a, b (N, D) fp32 -> t (N,) and out (2, N, D): out[0] the point of the path from a to b at t, out[1] the point at
 *                  t + eps (eps a double in (0, 1); the sum is formed in double).  One launch, one workgroup per row;
 *                  1 <= D <= GANLAB_PPL_MAX_DIM, 1 <= N < 2^31.
 *                  sampling FULL: t[n] = (w >> 8) 2^-24 in [0, 1), w = word 0 of Philox4x32-10 on the counter (offset + n, 0, 0, 0)
 *                  (low, high 32 bits of offset + n first) under the key (low, high 32 bits of seed) - one counter per row, so
 *                  the draw of N rows is the prefix of any longer one from the same seed and offset.  sampling END: t = 0.
 *                  mode LERP:  a + (b - a) t per entry, in double from the fp32 operands, rounded once.
 *                  mode SLERP: ah = a / |a|, bh = b / |b|, d = clamp(<ah, bh>, -1, 1), c = bh - d ah, ch = c / |c|;
 *                  r = ah cos(t acos d) + ch sin(t acos d); out = r sqrt(D / |r|^2) (StyleGAN's slerp of normalised latents,
 *                  rescaled to the radius sqrt(D) of a normal latent).  Entries, |a|^2, |b|^2, <ah, bh>, |c|^2 and |r|^2 are
 *                  fp32 (fixed-order sums over the row's workgroup); acos, the angle, its sine and cosine and the final scale are
 *                  formed in double from those and rounded once.  Where |c|^2 < 2^-30 (parallel or antipodal rows), |a| = 0 or
 *                  |b| = 0, both points are ah sqrt(D), with ah = a where |a| = 0.  Finite for finite rows.
 *   row_sqdist:    out[n] = sum_j (x[n, j] - y[n, j])^2 over N rows of D floats: differences, squares and the sum in double,
 *                  rounded once to fp32.  x and y may be the two halves of one (2N, D) buffer.  D >= 1, 1 <= N < 2^31.
 *   trimmed_mean:  v (n,) fp32, 1 <= n < 2^31 -> record of 5 doubles (mean, lo, hi, kept, nonfinite).  The values are sorted
 *                  (rocPRIM radix sort into the workspace, ganlab_trimmed_mean_workspace(n) bytes; 0 = n refused);
 *                  lo = sorted[floor((n - 1) q_lo)], hi = sorted[ceil((n - 1) q_hi)], the products in double, rounded once
 *                  (numpy.percentile's 'lower' / 'higher'), 0 <= q_lo <= q_hi <= 1; kept = the number of
 *                  values with lo <= v <= hi (ties at either bound all count); mean = their fp64 sum over kept, the sum taken
 *                  over the sorted array in a fixed order.  With any NaN or infinity among the values: nonfinite = their number,
 *                  mean = lo = hi = NaN, kept = 0. */
#define GANLAB_PPL_MAX_DIM 4096
#define GANLAB_PPL_LERP 0
#define GANLAB_PPL_SLERP 1
#define GANLAB_PPL_FULL 0
#define GANLAB_PPL_END 1
int ganlab_ppl_endpoints_f32(const float* a, const float* b, float* t, float* out, long long N, int D, double eps, int mode,
                             int sampling, uint64_t seed, uint64_t offset, void* stream);
int ganlab_row_sqdist_f32(const float* x, const float* y, float* out, long long N, long long D, void* stream);
size_t ganlab_trimmed_mean_workspace(long long n);
int ganlab_trimmed_mean_f32(const float* v, long long n, double q_lo, double q_hi, double* record, void* workspace,
                            size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GANLAB_HIP_H */
