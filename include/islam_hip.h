/* islam_hip.h -- C ABI of libislam_hip.so: the MI355X (gfx950) implementation of iSLAM's bilevel
 * hot path.
 *
 * The reference (sair-lab/iSLAM @ 2024_10_08) has no FFI of its own: its hot path is Python on
 * PyTorch/PyPose plus four CuPy RawKernels.  Each entry point below therefore names the reference
 * Python/CUDA code it replaces (file:line under /root/reference); INTEGRATION.md shows the ctypes
 * stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (PyTorch tensors' data_ptr()),
 *     contiguous, row-major / NCHW; the library never frees or retains them;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued on it;
 *     islam_pvgo_run_chain[_reproj]() polls one 128-byte verdict per LM trial in pinned host memory (no stream
 *     synchronisation), islam_pvgo_solve_chain_timed() synchronises the stream; nothing else waits on the device;
 *   - return 0 on success, <0 on error: -1 bad argument, -2 HIP runtime error, -3 non-positive
 *     pivot in the block Cholesky (PyPose: "Linear solver failed. Breaking optimization step"),
 *     -4 unsupported graph topology;  islam_last_error() returns a thread-local message;
 *   - dtype codes: 0 = float32, 1 = float64.
 */
#ifndef ISLAM_HIP_H
#define ISLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISLAM_OK 0
#define ISLAM_EARG (-1)
#define ISLAM_EHIP (-2)
#define ISLAM_ENOTPD (-3)
#define ISLAM_ETOPO (-4)
#define ISLAM_F32 0
#define ISLAM_F64 1

const char* islam_last_error(void);
int islam_abi_version(void);

/* Measurement aid (no reference counterpart; bench.py's stereo_vio diagnostics): one wavefront runs `iters` dependent fp64 FMAs on
 * `stream` and writes out3[0] = elapsed ticks of the constant-rate wall clock (islam_wall_clock_khz), out3[1] = elapsed shader
 * cycles; shader MHz = out3[1] / out3[0] * wall kHz / 1e3.  Launched on a stream of its own it samples the clock the chip sustains
 * while other streams keep it busy.  out3: 3 x int64 in device memory. */
int islam_clock_probe(long long* out3, int iters, void* stream);
int islam_wall_clock_khz(int device);
/* Measurement aid (no reference counterpart; bench.py's roofline.latency_model, SURVEY 8(d) "t >= n_launch * t_launch + depth * t_block"):
 * `n` back-to-back launches of a kernel that does nothing (grid x block threads) on `stream` between one pair of events;
 * *us_per_launch = the period of a kernel in a chain of dependent launches on this platform.  Synchronises the stream. */
int islam_launch_cost_probe(int grid, int block, int n, float* us_per_launch, void* stream);

/* ---------------------------------------------------------------- PWC-Net front-end kernels */

/* 81-channel local correlation, forward.
 * Replaces Network/PWC/correlation.py:281-331 (_FunctionCorrelation.forward) and its two CUDA
 * kernels kernel_Correlation_rearrange (:8-33) + kernel_Correlation_updateOutput (:35-103):
 *   out[b,(dy+4)*9+(dx+4),y,x] = (1/C) sum_c f1[b,c,y,x] * f2[b,c,y+dy,x+dx],  dy,dx in [-4,4], zero pad.
 * f1,f2: (B,C,H,W) float32; out: (B,81,H,W) float32.
 * scratch: islam_corr81_scratch_bytes(B,C,H,W) bytes or NULL.  Small pyramid levels have too few tiles to fill the chip;
 * with scratch the channels are split over workgroups and summed in a fixed order (deterministic). */
size_t islam_corr81_scratch_bytes(int B, int C, int H, int W);
int islam_corr81_fwd(const float* f1, const float* f2, float* out, int B, int C, int H, int W, void* scratch, void* stream);
/* The same correlation followed by LeakyReLU(slope), written into channels [ooff, ooff + 81) of out = (B,otot,H,W): PWC-Net's
 * `corr = self.leakyRELU(corr)` and the torch.cat that follows (Network/PWC/PWCNet.py:225-227, 255-258) without the two extra passes. */
int islam_corr81_fwd_act(const float* f1, const float* f2, float* out, int otot, int ooff, float slope, int B, int C, int H, int W, void* scratch,
                         void* stream);

/* Correlation backward.  Replaces correlation.py:334-383 with kernels updateGradFirst (:105-167) and
 * updateGradSecond (:169-233).  g1 and/or g2 may be NULL (needs_input_grad false). */
int islam_corr81_bwd(const float* f1, const float* f2, const float* gout, float* g1, float* g2,
                     int B, int C, int H, int W, void* stream);

/* Backward warp + validity mask.  Replaces Network/PWC/PWCNet.py:170-206 (PWCDCNet.warp):
 * out = grid_sample(x, grid + flow*scale, bilinear, zeros, align_corners=True) * (grid_sample(1,..) >= 0.9999).
 * x,out: (B,C,H,W); flow: (B,2,H,W) float32.  `scale` is the per-level factor of PWCNet.py:259-268. */
int islam_warp_mask(const float* x, const float* flow, float scale, float* out, int B, int C, int H, int W,
                    void* stream);

/* Backward of islam_warp_mask (autograd of PWCNet.py:195-206; the mask is piecewise constant).
 * gx (B,C,H,W) and gflow (B,2,H,W) must be ZERO-INITIALISED by the caller (atomic scatter). */
int islam_warp_mask_bwd(const float* x, const float* flow, float scale, const float* gout, float* gx, float* gflow,
                        int B, int C, int H, int W, void* stream);
/* ConvTranspose2d(C, 2, kernel 4, stride 2, padding 1) + bias, fp32 NCHW: PWC-Net's `deconv%d` / `upfeat%d`
 * (Network/PWC/PWCNet.py:55-56 `deconv()`, layers :113-114 ff., uses :259-268).  x: (B,C,H,W); w: (C,2,4,4) as nn.ConvTranspose2d stores it;
 * the two output channels go to channels [coff, coff + 2) of y = (B,ytot,2H,2W).  Exact fp32 FMAs; channel sums in a fixed order. */
int islam_deconv4x4s2_to2_f32(const float* x, const float* w, const float* bias, float* y, int ytot, int coff, int B, int C, int H, int W,
                              void* stream);
/* PWC-Net's flow head + up-sampled features of one level in ONE pass over the level's DenseNet concatenation:
 *   flow = Conv2d(C, 2, kernel 3, padding 1)(x) + bf          (`predict_flow%d`, Network/PWC/PWCNet.py:112,122,132,142,152; no activation)
 *   up   = ConvTranspose2d(C, 2, 4, 2, 1)(x) + bu              (`upfeat%d`, as islam_deconv4x4s2_to2_f32), into channels [upoff, upoff+2) of
 *                                                               up = (B,uptot,2H,2W); wu == NULL: the head alone (level 2)
 * x: (B,C,H,W) fp32; wf: [C][2][3][3] fp32 (the Conv2d weight with its first two axes swapped); flow: (B,2,H,W).  Exact fp32 FMAs
 * (the reference's arithmetic; the matrix-core path rounded the head's operands to bf16), fixed summation order. */
int islam_flow_head_up_f32(const float* x, const float* wf, const float* bf, float* flow, const float* wu, const float* bu, float* up, int uptot,
                           int upoff, int B, int C, int H, int W, void* stream);
/* One level of PWC-Net's feature pyramid -- conv(k3, stride 2) + conv(k3) + conv(k3), each + bias + LeakyReLU(slope) -- in one
 * launch (Network/PWC/PWCNet.py:78-83 conv1a/conv1aa/conv1b, conv2a/conv2aa/conv2b; :16-20 `conv()`; used at :240-243).  bf16 operands
 * (round to nearest even), fp32 accumulation, fp32 bias / activation; intermediates stay in LDS.  x: (B,Cin,H,W) fp32 NCHW;
 * y: (B,C,(H-1)/2+1,(W-1)/2+1) fp32 NCHW; wA/wB/wC: bf16 [C][ceil(9*SC/32)*32], K index = (ky*3+kx)*SC + c, SC = 4 for Cin <= 4 else
 * Cin (wB, wC: SC = C), zero padded (islam_pyramid_packed_elems elements each; islam_amd/ops.py pack_pyramid_weight).
 * Built for (Cin, C) = (3, 16) and (16, 32); anything else is ISLAM_EARG. */
size_t islam_pyramid_packed_elems(int Cin, int Cout);
int islam_flow_pyramid_level(const float* x, const uint16_t* wA, const float* bA, const uint16_t* wB, const float* bB, const uint16_t* wC,
                             const float* bC, float* y, int B, int Cin, int H, int W, int C, float slope, void* stream);

/* Level 1 of the pyramid on the two frames of a pair tensor x (B, 6, H, W) fp32 = [frame 1 | frame 2] along the channels -- the input
 * PWCDCNet.forward splits (Network/PWC/PWCNet.py:224-226): y (2 B, 16, H/2, W/2), first frames first, as islam_flow_pyramid_level
 * gives for torch.cat((x[:, :3], x[:, 3:]), 0), without that copy. */
int islam_flow_pyramid_level_pair(const float* x, const uint16_t* wA, const float* bA, const uint16_t* wB, const float* bB, const uint16_t* wC,
                                  const float* bC, float* y, int B, int H, int W, float slope, void* stream);

/* 3x3 convolution (+ bias + LeakyReLU) of the frozen flow network on the matrix cores (implicit GEMM, bf16 operands,
 * fp32 accumulate).  Replaces cuDNN under Network/PWC/PWCNet.py:16-20 `conv()` (Conv2d k=3, padding = dilation, then
 * LeakyReLU(0.1)) for inference:  y[b, coff+n, ho, wo] = act(bias[n] + sum w[n,c,r,s] x[b, c, ho*stride + (r-1)*dil,
 * wo*stride + (s-1)*dil]),  act(v) = v >= 0 ? v : slope*v  (slope = 1: no activation).
 * x: channels [xoff, xoff+Cin) of a (B,xtot,H,W) fp32 NCHW buffer; y: channels [coff, coff+Cout) of a (B,ytot,Ho,Wo) fp32
 * NCHW buffer, Ho = (H-1)/stride+1 -- the DenseNet-style torch.cat of PWCNet.py:237-292 without a copy; bias (Cout) or NULL.
 * wpacked: bf16 bits, [9][CoutP][CinP] (tap = 3r+s; CoutP = Cout rounded up to 64, CinP = Cin rounded up to 16, zero padded),
 * islam_conv3x3_packed_elems(Cin, Cout) elements.  When Cin > 16 is not a multiple of 16 the LAST group of 16 channel slots holds
 * channels Cin-16 .. Cin-1 (the kernel's last chunk reads the last 16 channels of x), with zeros in the slots of channels the
 * previous group already holds; Cin <= 16 or a multiple of 16: slot c = channel c.  stride 1 or 2, dilation 1..16. */
size_t islam_conv3x3_packed_elems(int Cin, int Cout);
int islam_conv3x3_mfma(const float* x, const uint16_t* wpacked, const float* bias, float* y, int B, int Cin, int H, int W,
                       int Cout, int stride, int dilation, int xoff, int xtot, int coff, int ytot, float slope, void* stream);

/* Bilinear resize of a channels-last (NHWC) bf16 tensor: the F.upsample / F.interpolate calls of the frozen stereo network
 * (Network/PSM/submodule.py:124-155 SPP branches, Network/StereoNet7.py:100-146), ATen's upsample_bilinear2d arithmetic.
 * x (B,Hi,Wi,C), y (B,Ho,Wo,C) bf16 bits, C a multiple of 8; align_corners as in torch. */
int islam_resize_bilinear_nhwc_bf16(const uint16_t* x, uint16_t* y, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                    int align_corners, void* stream);
/* The same, written into channels [yoff, yoff+C) of a (B,Ho,Wo,ytot) tensor (ytot, yoff multiples of 8): bilinear resizing is
 * per channel, so the up-sampled concatenation of submodule.py:140-152 is assembled in place, piece by piece, without the
 * intermediate torch.cat and without copying the up-sampled tensor into the next concatenation. */
int islam_resize_bilinear_nhwc_bf16_into(const uint16_t* x, uint16_t* y, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                         int align_corners, int ytot, int yoff, void* stream);
/* torch.cat((F.interpolate(torch.cat(pieces, 1), (Ho, Wo), mode='bilinear'), tail), 1) in one launch: the `bigger` feature extractor of
 * StereoNet7 (Network/StereoNet7.py:36-46 -> Network/PSM/submodule.py:139-152 with the extra up-sampling and layer1's output joined).
 * srcs / chans: HOST arrays of n <= 8 device pointers to channels-last bf16 pieces (B, Hi, Wi, chans[k]) / their channel counts
 * (multiples of 8); tail (may be NULL with tailC = 0): (B, Ho, Wo, tailC); y: (B, Ho, Wo, sum(chans) + tailC).  Every sample is
 * islam_resize_bilinear_nhwc_bf16's arithmetic; whole pixels are written contiguously. */
int islam_upsample_cat_nhwc_bf16(const uint16_t* const* srcs, const int* chans, int n, const uint16_t* tail, int tailC, uint16_t* y,
                                 int B, int Hi, int Wi, int Ho, int Wo, int align_corners, void* stream);
/* The stereo pair as the feature extractor's batch (Network/StereoNet7.py:95-97 feeds left and right images through one
 * feature_extraction): x (B, H, W, C2) channels-last bf16 with the left image in channels [0, C2/2) and the right one behind it;
 * y (2B, H, W, 8): images [0, B) left, [B, 2B) right, channels [C2/2, 8) zero -- the input of the 3 -> 32 stride-2 first layer
 * (Network/PSM/submodule.py:63) on islam_conv_nhwc_bf16_s2 with its weights zero-padded to 8 input channels. */
int islam_stack_pair_pad8_nhwc_bf16(const uint16_t* x, uint16_t* y, int B, int C2, int H, int W, void* stream);
/* The same stacked batch AND the concatenated pair from the two fp32 NCHW images (B,c,H,W), c <= 4, in one pass: x6 (B,H,W,2c) bf16 =
 * torch.cat((left, right), 1).to(bfloat16) channels-last (Network/VONet.py:31-34), xs (2B,H,W,8) as above.  Round-to-nearest-even. */
int islam_stereo_pair_prepare_f32(const float* left, const float* right, uint16_t* x6, uint16_t* xs, int B, int c, int H, int W, void* stream);
/* y = add + resize(x) in one pass (hourglass.py:60-69 `up1 + up2(low3)`): the up-sampled value is rounded to bf16 before the add,
 * like the two separate ops.  add, y: (B,Ho,Wo,C). */
int islam_resize_bilinear_add_nhwc_bf16(const uint16_t* x, const uint16_t* add, uint16_t* y, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                        int align_corners, void* stream);
/* The same into channels [yoff, yoff+C) of y = (B,Ho,Wo,ytot): the hourglass's half of the decoder's concatenations
 * (Network/StereoNet7.py:129-138 `x = self.conv_c8(x); x = torch.cat((x, cat2), dim=1)` ...) is written in place. */
int islam_resize_bilinear_add_nhwc_bf16_into(const uint16_t* x, const uint16_t* add, uint16_t* y, int B, int C, int Hi, int Wi, int Ho,
                                             int Wo, int align_corners, int ytot, int yoff, void* stream);
/* MaxPool2d(2, 2) / F.max_pool2d(kernel_size=2) of a channels-last bf16 tensor (hourglass.py:52, StereoNet7.py:117-125), relu != 0:
 * of relu(x) (the two commute); (B,H,W,C) -> (B,H/2,W/2,C), C a multiple of 8. */
int islam_maxpool2_nhwc_bf16(const uint16_t* x, uint16_t* y, int B, int C, int H, int W, int relu, void* stream);

/* F.interpolate(x, scale_factor=0.5, mode='bilinear') of a channels-last bf16 image with C <= 8 (even) channels -- the half-resolution
 * stereo pair of Network/StereoNet7.py:101 -- written with 8 - C zero channels behind it into channels [yoff, yoff + 8) of a
 * (B,H/2,W/2,ytot) bf16 tensor (the padded tail of conv_c0's concatenated input): one launch instead of ATen's up-sampling kernel, a
 * slice copy and a zero fill; the same values as ATen bit for bit.  H, W even; ytot, yoff multiples of 8. */
int islam_half_image_into_nhwc_bf16(const uint16_t* x, uint16_t* y, int ytot, int yoff, int B, int C, int H, int W, void* stream);
/* AvgPool2d((k,k), stride=(k,k)) of a channels-last bf16 tensor (the SPP branches, submodule.py:103-122): fp32 accumulation, one
 * rounding; (B,H,W,C) -> (B,H/k,W/k,C). */
int islam_avgpool_nhwc_bf16(const uint16_t* x, uint16_t* y, int B, int C, int H, int W, int k, void* stream);

/* In-place epilogue of a bias-free convolution on a channels-last bf16 tensor: y <- act(bf16(y + bias[c]) [+ res]),
 * act = ReLU (relu != 0) or identity; res NULL or a tensor of y's shape.  One pass for the bias add, activation and residual
 * add around the convolutions of Network/PSM/hourglass.py:6-40 (Residual) and Network/StereoNet7.py:100-146.
 * y, res: (pixels, C) bf16 bits, C a multiple of 8; bias (C) fp32. */
int islam_bias_act_add_nhwc_bf16(uint16_t* y, const float* bias, const uint16_t* res, long long pixels, int C, int relu,
                                 void* stream);
/* The elementwise tail of the trainable pose head's convolutions (Network/VOFlowNet.py:42-157: conv + bias + ReLU, residual
 * blocks conv + bias + shortcut + ReLU), fp32 channels-last (pixels x C, C a multiple of 4), one launch each way:
 *   forward   y = act(x + bias[c] (+ res));  x may alias y
 *   backward  gx = gy * (y > 0) (relu) or gy;  gbias[c] = sum over pixels of gx (deterministic two-stage sum); gx may alias gy.
 * scratch: islam_bias_act_bwd_scratch_floats(pixels, C) floats; ticket: one zero-initialised word, left at zero. */
int islam_bias_act_f32_nhwc(const float* x, const float* bias, const float* res, float* y, long long pixels, int C, int relu,
                            void* stream);
long long islam_bias_act_bwd_scratch_floats(long long pixels, int C);
int islam_bias_act_bwd_f32_nhwc(const float* gy, const float* y, float* gx, float* gbias, float* scratch, unsigned* ticket,
                                long long pixels, int C, int relu, void* stream);

/* The trainable pose head, whole: VOFlowRes.forward_ (Network/VOFlowNet.py:185-194) over the feature embedding of config 1 (:110-157: three
 * plain convolutions, five stages of BasicBlocks :20-39 of 3/4/6/7/3 blocks at 64/128/128/256/256 channels, first block of a stage with
 * stride 2 and a 1x1 stride-2 convolution on its shortcut) and the two Linear heads (:84-92), and its backward (what
 * train.py:280-283's loss.backward() runs through this module) -- each ONE call that enqueues hand-written fp32 kernels (exact-fp32
 * matrix-core implicit GEMMs, csrc/pose_head.hip) on `stream`: no MIOpen / CK / ATen launch, deterministic summation orders.
 *   x        (B,H,W,4) fp32 channels-last: [flow(2), intrinsic layer(2)] (Network/VONet.py:36); B <= 16; the input's 1/64-size feature map
 *            (six times v -> (v - 1) / 2 + 1) must have 6 pixels: 2x3 for H = 65..128, W = 129..192 (448x640 images: H = 112, W = 160);
 *            3x2 and 1x6 are served as well, 6x1 (a level one pixel wide) is not
 *   params   the module's 120 parameters in state_dict order (feat_net.0.0.weight, feat_net.0.0.bias, ..., voflow_rot.2.bias), device pointers;
 *            convolution weights in channels_last memory ([Cout][ky][kx][Cin]), everything else contiguous
 *   out6     (B,6) = cat(trans, rot)
 *   workspace  islam_pose_head_workspace_bytes(B,H,W) bytes (0: unsupported shape), or more; holds every activation of the forward plus
 *            gradient buffers and split-K scratch.  Must be zero-filled ONCE before its first use (the split-K ticket words and a
 *            region of zeros: both sit at the same offsets for every shape, in front of everything a call writes, and every launch
 *            leaves them zero).  One workspace may then serve any sequence of shapes it is large enough for (the largest
 *            islam_pose_head_workspace_bytes of the sequence; the size grows with B, H and W) without being cleared in between.  The
 *            backward reads what the LAST forward on this workspace left there: that forward must have had the SAME (B,H,W) and x.
 * backward: grads[i] receives (accumulate = 0) or is incremented by (accumulate = 1) the gradient of parameter i, same layouts as params;
 * grad_out6 (B,6).  No gradient w.r.t. x is produced (the reference detaches the flow in front of the head's consumers only when the flow
 * net is frozen, TartanVO.py:109; a trainable flow net takes the eager autograd path in islam_amd/nets.py). */
size_t islam_pose_head_workspace_bytes(int B, int H, int W);
int islam_pose_head_forward(const float* x, const float* const* params, float* out6, void* workspace, size_t workspace_bytes, int B, int H,
                            int W, void* stream);
int islam_pose_head_backward(const float* x, const float* const* params, float* const* grads, const float* grad_out6, void* workspace,
                             size_t workspace_bytes, int B, int H, int W, int accumulate, void* stream);

/* Train-mode BatchNorm2d (+ ReLU, + residual add) on a channels-last bf16 tensor -- the BatchNorm layers of the "frozen"
 * stereo feature extractor, which the reference still runs with batch statistics (TartanVO.py:90-91; Network/PSM/
 * submodule.py:10-43):  y = act(bf16(x*scale[c] + shift[c]) [+ res]), scale = weight*rsqrt(var_biased + eps),
 * shift = bias - mean*scale; running_mean / running_var (unbiased) / num_batches_tracked updated as nn.BatchNorm2d does
 * (pass NULL to skip).  x, y, res: (pixels, C) bf16 bits (y may alias x), C = 8 * (a divisor of 256), at most 256; weight, bias, running_*:
 * fp32 (C); scratch: islam_bn_scratch_floats(C) floats.  Deterministic (fixed-order reduction). */
size_t islam_bn_scratch_floats(int C);
int islam_bn_train_nhwc_bf16(const uint16_t* x, uint16_t* y, const uint16_t* res, const float* weight, const float* bias,
                             float* running_mean, float* running_var, long long* num_batches_tracked, double momentum,
                             double eps, int relu, long long pixels, int C, float* scratch, void* stream);

/* Channels-last bf16 convolution of the frozen stereo feature extractor on the matrix cores (implicit GEMM, fp32 accumulate,
 * round-to-nearest-even output), with the surrounding train-mode BatchNorm folded into its two ends.  Replaces cuDNN under
 * Network/PSM/submodule.py:10-13 `convbn` (Conv2d k=3 p=1 / k=1 p=0, stride 1, bias=False, then BatchNorm2d), :66-155.
 *   y[b,ho,wo,n] = epi( sum w[n,c,r,s] * pre(x[b, ho+r-P, wo+s-P, c]) ),  P = ksize/2, zero padding, output size = input size
 *   pre(v) = v  (in_affine NULL)  or  relu(bf16(v*in_affine[c] + in_affine[Cin+c]))  -- the producer's BatchNorm + ReLU on load
 *   epi(a) = bf16(a), and with `stats` the per-channel sums of bf16(a) and bf16(a)^2 over all pixels (stats NULL: skipped);
 *            or  act( bf16( bf16(a + bias[n]) [+ res] ) ),  act = ReLU if `relu` & 1;  `relu` & 2: pre(v) = relu(v) (in_affine NULL).
 * x (B,H,W,Cin), res / y (B,H,W,Cout) bf16 bits, Cin and Cout multiples of 8; wpacked: bf16 [ksize*ksize][CoutP][CinP], CoutP =
 * Cout rounded up to 64, CinP = Cin rounded up to 32, zero padded (islam_conv_nhwc_packed_elems elements).
 * stats: islam_conv_nhwc_stats_floats(B,H,W,Cout) floats; on return its LAST 256*2*Cout floats hold the folded partial sums
 * ([256][2][Cout], fixed-order = deterministic) that islam_bn_finalize reads.  ksize 1 or 3. */
size_t islam_conv_nhwc_packed_elems(int Cin, int Cout, int ksize);
int islam_conv_nhwc_stat_blocks(int B, int H, int W, int Cout);
size_t islam_conv_nhwc_stats_floats(int B, int H, int W, int Cout);
int islam_conv_nhwc_bf16(const uint16_t* x, const uint16_t* wpacked, const float* in_affine, const float* bias, const uint16_t* res,
                         uint16_t* y, float* stats, int B, int Cin, int H, int W, int Cout, int ksize, int relu, void* stream);
/* islam_conv_nhwc_bf16 (no residual, no statistics) with the result written into channels [yoff, yoff + Cout) of a (B,H,W,ytot) bf16
 * tensor: straight into a concatenation under construction (Network/StereoNet7.py:103-105) instead of a dense tensor torch.cat copies.
 * ytot, yoff: multiples of 8.  `relu` as in islam_conv_nhwc_bf16. */
int islam_conv_nhwc_bf16_into(const uint16_t* x, const uint16_t* wpacked, const float* in_affine, const float* bias, uint16_t* y, int ytot,
                              int yoff, int B, int Cin, int H, int W, int Cout, int ksize, int relu, void* stream);

/* Conv2d(Cin, Cout, k, stride = 2, padding = k / 2) on the same kernel: layer2's stride-2 3x3 convbn and its stride-2 1x1 downsample
 * (Network/PSM/submodule.py:24-26, 76-85) and the 2x2 stride-2 form of StereoNet7's last transposed convolution at the pixels VONet keeps
 * (Network/StereoNet7.py:88-90, Network/VONet.py:33-34).  x (B,Hi,Wi,Cin) -> y (B,Ho,Wo,Cout), Ho <= (Hi + 2 (k/2) - k) / 2 + 1 (fewer rows /
 * columns may be asked for); k = 1, 2, 3; the other arguments as islam_conv_nhwc_bf16, `stats` sized by islam_conv_nhwc_s2_stats_floats
 * (its last 256*2*Cout floats are the folded sums). */
size_t islam_conv_nhwc_s2_stats_floats(int B, int Ho, int Wo, int Cout);
int islam_conv_nhwc_bf16_s2(const uint16_t* x, const uint16_t* wpacked, const float* in_affine, const float* bias, const uint16_t* res,
                            uint16_t* y, float* stats, int B, int Cin, int Hi, int Wi, int Cout, int Ho, int Wo, int ksize, int relu,
                            void* stream);

/* `convbn` in training mode up to the BatchNorm's [scale | shift] (Network/PSM/submodule.py:10-13): islam_conv_nhwc_bf16 with `stats`
 * followed by islam_bn_finalize as one call, bit for bit the same results (y raw convolution output, scale_shift 2*Cout floats, running
 * statistics updated like nn.BatchNorm2d; count = B*H*W).  Two launches behind the persistent kernels (their few rows of partial sums go
 * straight into the finalize), three behind the tile kernel.  counter: one int of device memory that is zero before the call and is left
 * zero (used by the ticketed variant only, ISLAM_BN_FINALIZE=1); calls that may run concurrently on different streams must not share it. */
int islam_conv_nhwc_bf16_bn(const uint16_t* x, const uint16_t* wpacked, const float* in_affine, uint16_t* y, float* stats, int B, int Cin,
                            int H, int W, int Cout, int ksize, int in_relu, const float* weight, const float* bias, float* running_mean,
                            float* running_var, long long* num_batches_tracked, double momentum, double eps, float* scale_shift,
                            int* counter, void* stream);
/* Which kernel serves the 128 -> 128, 64 -> 128 and 32 -> 32 3x3 layers (Network/PSM/submodule.py:66-155 feature_extraction: layer3 /
 * layer4, twelve per forward; firstconv / layer1, eight per forward) behind islam_conv_nhwc_bf16 / _into / _bn: 0 = the tile kernel, 1 (default;
 * ISLAM_CONV_WS presets it) = the persistent kernels of csrc/conv_ws.hip (weights in the register file, 32 x 4-pixel tiles) and
 * csrc/conv_ws32.hip (32 x 16-pixel tiles) when the image is whole tiles and has at least 1024 of them, 2 = the persistent kernels on
 * every whole-tile layer (tests, A/B runs).  Bit-identical outputs either way.  Returns the previous mode; any other argument only queries. */
int islam_conv_ws_mode(int mode);
/* Launches of the two persistent kernels since the library was loaded (host-side counters; a launch recorded into a HIP graph counts once,
 * at capture): out2[0] = conv3x3_ws_kernel (conv_ws.hip), out2[1] = conv3x3_ws32_kernel (conv_ws32.hip).  The parity tests of the stereo
 * feature extractor (Network/PSM/submodule.py:66-155) use it to prove which kernel produced the output they compare. */
int islam_conv_ws_launch_counts(long long* out2);
/* 3x3 stride-1 convolution of the flow net's DenseNet blocks (Network/PWC/PWCNet.py:16-20 `conv()` = Conv2d + LeakyReLU(0.1),
 * :237-292 the blocks) on the channels-last kernel.  x: bf16 channels [xoff, xoff + Cin) of a (B,H,W,xtot) MIRROR of the block's
 * concatenation buffer; the result goes as fp32 NCHW into channels [coff, coff + Cout) of y32 (B,ytot,H,W) -- what correlation /
 * warp / transposed convolutions / flow heads read -- and, when ymir != NULL, as bf16 into channels [moff, moff + Cout) of the
 * (B,H,W,mtot) mirror for the next convolution.  Same arithmetic as islam_conv3x3_mfma (operands rounded to bf16 nearest-even,
 * fp32 accumulation, bias, LeakyReLU(slope); slope 1: none).  wpacked: islam_conv_nhwc_packed_elems(Cin, Cout, 3) elements with
 * zero rows for padded input channels.  Cin, Cout, xtot, xoff, mtot, moff: multiples of 8.  y32 or ymir may be NULL (not both).
 * dilation d > 1 (the context layers dc_conv2-5): evaluated as d*d dense convolutions on the sub-grids (a::d, c::d) of the image;
 * H and W must be multiples of d. */
int islam_conv_nhwc_flow(const uint16_t* x, int xtot, int xoff, int Cin, const uint16_t* wpacked, const float* bias, float* y32, int ytot,
                         int coff, uint16_t* ymir, int mtot, int moff, int B, int H, int W, int Cout, int dilation, float slope, void* stream);
/* ConvTranspose2d(Cin, Cout, kernel 4, stride 2, padding 1) + bias (+ ReLU, relu = 1) of the frozen stereo net's decoder --
 * Network/StereoNet7.py:78-90 (deconv_c7_2, deconv_c7 ... deconv_c10) with the activation and concatenation of :121-136 -- on the
 * channels-last matrix-core kernel: four dense 2x2 convolutions, one per output parity class (a, c) of pixel (2y + a, 2x + c), taps
 * K[r][s] = W[:, :, 3 - 2r - a, 3 - 2s - c].  x: (B,H,W,Cin) bf16; wpacked: islam_deconv_nhwc_packed_elems(Cin, Cout) bf16 elements,
 * [class a*2+c][tap r*2+s][CoutP][CinP]; the result goes to channels [yoff, yoff + Cout) of y = (B,2H,2W,ytot) bf16 (the channel
 * slice of the concatenation the decoder builds next).  bf16 operands, fp32 accumulation, output rounded to nearest even.
 * Cin, Cout, ytot, yoff: multiples of 8. */
size_t islam_deconv_nhwc_packed_elems(int Cin, int Cout);
int islam_deconv4x4s2_nhwc_bf16(const uint16_t* x, const uint16_t* wpacked, const float* bias, uint16_t* y, int ytot, int yoff, int B, int Cin,
                                int H, int W, int Cout, int relu, void* stream);
/* The transposed convolution above / islam_conv_nhwc_bf16_s2 (kernel size 2) on torch.cat((x1, x2), 1) of two dense channels-last tensors
 * read where they lie (Network/StereoNet7.py:121-138: the decoder concatenates the previous stage's result with a skip tensor in front of
 * every transposed convolution): C1 a multiple of 32 (16 for _s2_cat), C2 of 8, wpacked as for Cin = C1 + C2; bit-identical. */
int islam_deconv4x4s2_nhwc_bf16_cat(const uint16_t* x1, int C1, const uint16_t* x2, int C2, const uint16_t* wpacked, const float* bias, uint16_t* y,
                                    int ytot, int yoff, int B, int H, int W, int Cout, int relu, void* stream);
int islam_conv_nhwc_bf16_s2_cat(const uint16_t* x1, int C1, const uint16_t* x2, int C2, const uint16_t* wpacked, const float* bias, uint16_t* y, int B,
                                int Hi, int Wi, int Cout, int Ho, int Wo, int ksize, int relu, void* stream);
/* One Residual module of the stereo net's hourglass stacks in ONE launch -- Network/PSM/hourglass.py:28-52 (`Residual.forward`),
 * instantiated by Network/PSM/hourglass.py:53-77 / Network/StereoNet7.py:56-90:
 *   y = conv3(relu(conv2(relu(conv1(relu(x)))))) + res ;  conv1 1x1 Cin -> h, conv2 3x3 h -> h (padding 1), conv3 1x1 h -> Cout,
 *   h = Cout / 2, every convolution with a bias; res = x when Cin == Cout, else skip_layer(x) computed by the caller
 *   (islam_conv_nhwc_bf16, 1x1 of the raw x).  The two h-channel intermediates never leave LDS; rounding points as the layer-by-layer
 *   path: t1 = relu(bf16(. + b1)), t2 = relu(bf16(. + b2)), y = bf16(bf16(. + b3) + res); bf16 operands, fp32 accumulation.
 * x (B,H,W,Cin), res / y (B,H,W,Cout) bf16 bits; Cin, Cout multiples of 64 up to 256 (Cout = 64 with Cin = 64 only: res must be x).
 * wpacked: islam_hg_residual_packed_elems(Cin, Cout) bf16 elements = the weights as MFMA A fragments (64 lanes x 8 bf16 each) in
 * the order the waves consume them (layout: csrc/hourglass.hip; built by islam_amd/ops.py pack_hg_residual); bias: fp32
 * [b1 (h) | b2 (h) | b3 (Cout)]. */
size_t islam_hg_residual_packed_elems(int Cin, int Cout);
int islam_hg_residual_nhwc_bf16(const uint16_t* x, const uint16_t* res, uint16_t* y, const uint16_t* wpacked, const float* bias, int B, int Cin,
                                int H, int W, int Cout, void* stream);
/* fp32 NCHW channels [soff, soff + C) of src (B,stot,H,W) -> bf16 (nearest-even) channels [doff, doff + C) of dst (B,H,W,dtot);
 * channels up to the next multiple of 8 are zeroed.  Fills the mirror with what the non-convolution producers wrote. */
int islam_nchw_f32_to_nhwc_bf16(const float* src, int stot, int soff, uint16_t* dst, int dtot, int doff, int B, int C, int H, int W,
                                void* stream);
/* The two halves of islam_bn_train_nhwc_bf16 for a producer that delivers the statistics itself: folded = [256][2][C] partial
 * sums, count = pixels; scale_shift (2*C floats) = [weight*rsqrt(var+eps) | bias - mean*scale]; running statistics updated like
 * nn.BatchNorm2d (NULL: skipped).  C <= 256.  Apply: y = act( bf16(x*scale[c] + shift[c]) [+ res] ), C a multiple of 8. */
int islam_bn_finalize(const float* folded, double count, const float* weight, const float* bias, float* running_mean,
                      float* running_var, long long* num_batches_tracked, double momentum, double eps, int C, float* scale_shift,
                      void* stream);
int islam_bn_apply_nhwc_bf16(const uint16_t* x, uint16_t* y, const uint16_t* res, const float* scale_shift, int relu,
                             long long pixels, int C, void* stream);

/* ---------------------------------------------------------------- edge mask */

/* Edge mask of the front-end, whole batch in one launch, no host round trip.
 * Replaces TartanVO.py:145-155: img0.cpu() (27.5 MB D2H at B=8) -> (img*255).astype(uint8) -> per image
 * cv2.resize(fx=fy=1/4) -> cv2.Canny(im, 50, 100) -> cv2.dilate(5x5 ones) -> `> 0` -> .cuda().
 * img (B,3,H,W) float32 in [0,1]; mask (B,h,w) uint8 in {0,1} with h,w = H/4,W/4 (downscale != 0; H,W multiples of 4)
 * or H,W.  low/high: Canny thresholds (50, 100).  h*w <= islam_edge_mask_max_pixels(): the quarter-resolution image lives
 * in the LDS of one CU (112x160 for the 448x640 input); larger -> ISLAM_EARG. */
int islam_edge_mask_max_pixels(void);
int islam_edge_mask(const float* img, uint8_t* mask, int B, int H, int W, int downscale, int low, int high, void* stream);

/* ---------------------------------------------------------------- stereo scale recovery */

/* Replaces the per-sample Python loop TartanVO.py:159-167 around dense_ba.py:88-176
 * (scale_from_disp_flow, disparity branch) for a whole batch in one launch.
 * disp (B,1,H,W), flow (B,2,H,W) in pixels at 1/4 res; pose7 (B,7) = the ENU motion [t,q];
 * intr4 (B,4) = fx,fy,cx,cy at 1/4 res; baseline (B); edge (B,H,W) uint8 or NULL; disp_th (B).
 * Outputs: scale (B) = (M^T w)/(M^T M); z (B,H,W); mask, dmask (B,H,W) uint8;
 * sums (B,18) float64: [0] M^T M, [1] M^T w, [2..16] the first-order sums the backward pass of
 * `scale` w.r.t. the pose needs (layout in scale_ls.hip), [17] number of masked pixels;
 * partial: scratch of B*ISLAM_SCALE_NBLK*18 doubles. */
#define ISLAM_SCALE_NBLK 16
#define ISLAM_SCALE_NSUM 18
int islam_scale_ls(const float* disp, const float* flow, const float* pose7, const float* intr4,
                   const float* baseline, const uint8_t* edge, const float* disp_th,
                   float* scale, float* z, uint8_t* mask, uint8_t* dmask, double* sums, double* partial,
                   int B, int H, int W, void* stream);
/* Same with a depth map in place of the disparity (dense_ba.py:125-131, `depth=` argument of scale_from_disp_flow):
 * depth_mask = 0 < depth <= fx*baseline, z = depth there. */
int islam_scale_ls_depth(const float* depth, const float* flow, const float* pose7, const float* intr4,
                         const float* baseline, const uint8_t* edge, float* scale, float* z, uint8_t* mask,
                         uint8_t* dmask, double* sums, double* partial, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------- dense reprojection: normal equations and pose refinement */

/* The dense reprojection residual of dense_ba.DenseReprojectionLoss (reference dense_ba.py:179-273), differentiated.
 * Inputs per link b = 0..B-1: depth (B,H,W) float32; flow (B,2,H,W) float32; mask (B,H,W) uint8 or NULL (all ones);
 * motion (B,7) float64 = [t, q xyzw], the body-frame motion (run_pvgo's vo_motions); rgb2imu (7) float64 = C, NULL: identity;
 * intr4 (B,4) float64 = fx, fy, cx, cy.
 *
 * Per link and pixel (u, v), all in float64:
 *   T = C^-1 motion_b C,   P = z ((u - cx)/fx, (v - cy)/fy, 1),   Q = T^-1 P
 *   valid = mask and Q_z > 0.1 and |Q_x/Q_z| <= 1 and |Q_y/Q_z| <= 1     (proj(..., return_mask=True), bounds inclusive)
 *   r = (fx Q_x/Q_z + cx - (flow_u + u),  fy Q_y/Q_z + cy - (flow_v + v)),   s = |r|^2
 * The perturbation is on the right of the body-frame motion, motion Exp(xi), xi = [rho, phi] (PyPose's order):
 *   T(xi) = T Exp(A xi), A = Ad(C^-1);   dQ/dxi_cam = [-I3, [Q]x];
 *   dr/dQ = [[fx/Q_z, 0, -fx Q_x/Q_z^2], [0, fy/Q_z, -fy Q_y/Q_z^2]];   J = dr/dQ dQ/dxi_cam A.
 * With a robust kernel rho(s), c = rho'(s) (robust_kind = ISLAM_ROBUST_NONE / _HUBER / _CAUCHY and robust_delta = d as defined at
 * islam_pvgo_robust below), summed over the valid pixels:
 *   H = sum c J^T J (6x6, symmetric to the bit),  g = sum c J^T r (6),  cost = sum rho(s),  l1 = sum |r_u| + |r_v|,  count = n.
 * l1 / n is DenseReprojectionLoss.__call__'s value; cost(xi) = cost + 2 g^T xi + xi^T H xi to second order; H / sigma_px^2 is
 * the information of that edge's VO residual Log(P^-1 X_i^-1 X_j) in the frame and row order of islam_pvgo_run_chain_info's
 * info_vo.  An empty mask gives H = 0, g = 0, count = 0.
 *
 * Outputs: out_H (B,6,6), out_g (B,6), out_cost, out_l1, out_count (B) (the count as a double), out_sums (B,30): the camera-frame
 * sums before A is applied, [0..20] the upper triangle of sum c Jc^T Jc in row-major order of the triangle, [21..26] sum c Jc^T r,
 * [27] cost, [28] l1, [29] count.  One workgroup row of ISLAM_DENSE_REPROJ_NBLK partial sums per link is reduced in fixed order
 * without atomics: the same inputs give the same bits.  scratch: islam_dense_reproj_scratch_bytes(B, 0) bytes; calls that may run
 * concurrently must not share it.  Only enqueues on `stream`.  ISLAM_EARG before any device work for B, H, W < 1 (or H*W > 2^30),
 * an unknown robust kind, robust_delta <= 0, a NULL pointer other than mask and rgb2imu. */
#define ISLAM_DENSE_REPROJ_NBLK 64
#define ISLAM_DENSE_REPROJ_NSUM 30
size_t islam_dense_reproj_scratch_bytes(int B, int iters_or_0);
int islam_dense_reproj_normal(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                              const double* rgb2imu, const double* intr4, int robust_kind, double robust_delta,
                              double* out_H, double* out_g, double* out_cost, double* out_l1, double* out_count,
                              double* out_sums, void* scratch, int B, int H, int W, void* stream);

/* Levenberg-Marquardt on these normal equations, `iters` evaluations, all on the device (two launches per evaluation, no host
 * wait in between).  Evaluation 0 reduces at `motion`; evaluation k >= 1 reduces at the link's trial pose.  After it, per link:
 *   1. the trial is accepted iff count_trial >= min_count, every sum is finite and cost_trial/count_trial < cost/count (the mean:
 *      the pixel set moves with the pose, and losing pixels must not count as progress);
 *   2. accepted: the trial's pose and sums become the link's state, lambda <- max(lambda/10, ISLAM_DENSE_REPROJ_LAMBDA_MIN);
 *      otherwise lambda <- min(10 lambda, ISLAM_DENSE_REPROJ_LAMBDA_MAX);  (lambda starts at `damping`)
 *   3. (H + lambda diag(H)) delta = -g by a 6x6 Cholesky;
 *   4. the next trial is state Exp(delta), its quaternion normalised.  (Not after the last evaluation.)
 * out_status (B): ISLAM_DENSE_REPROJ_FEW when, at `motion`, count < min_count or a sum is not finite; ISLAM_DENSE_REPROJ_NOTPD
 * when step 3 meets a non-positive pivot.  Such a link stops where it stands (FEW, and NOTPD at evaluation 0: the pose as
 * given; NOTPD later: the last accepted pose); the other links carry on.
 * Outputs: out_motion (B,7) and out_H .. out_sums AT it, as islam_dense_reproj_normal writes them there (the same bits);
 * out_lambda (B); out_accepted, out_rejected (B) int; trace (trace_cap,B) or NULL with trace_cap = 0: cost/count of evaluation
 * k < trace_cap (evaluation 0: the start).  scratch: islam_dense_reproj_scratch_bytes(B, iters).  ISLAM_EARG before any device
 * work for the cases of islam_dense_reproj_normal, iters < 1, damping < 0, min_count < 0, a NULL output, trace_cap > 0 with
 * a NULL trace. */
#define ISLAM_DENSE_REPROJ_OK 0
#define ISLAM_DENSE_REPROJ_FEW 1
#define ISLAM_DENSE_REPROJ_NOTPD 2
#define ISLAM_DENSE_REPROJ_LAMBDA_MIN 1e-12
#define ISLAM_DENSE_REPROJ_LAMBDA_MAX 1e12
int islam_dense_reproj_refine(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                              const double* rgb2imu, const double* intr4, int robust_kind, double robust_delta, int iters,
                              double damping, double min_count, double* out_motion, double* out_H, double* out_g,
                              double* out_cost, double* out_l1, double* out_count, double* out_sums, double* out_lambda,
                              int* out_accepted, int* out_rejected, int* out_status, double* trace, int trace_cap,
                              void* scratch, int B, int H, int W, void* stream);

/* The gradient of the refined pose with respect to depth and flow.
 *
 * islam_dense_reproj_vjp: for w (B,6) float64 in the body frame, [rho, phi], the derivative of Phi = w^T g (g as
 * islam_dense_reproj_normal returns it at `motion`) in every depth and flow value, with the pose and the valid set held fixed.
 * With w_cam = A w, per valid pixel (a, bq, cq, dq: the entries of dr/dQ above; c' = dc/ds):
 *   m = -w_cam,rho + Q x w_cam,phi,   q = dr/dQ m,   e = c q + 2 c' (q.r) r,   dQ = R ((u - cx)/fx, (v - cy)/fy, 1)  (R of T^-1)
 *   dPhi/dflow = -e,   dPhi/dz = e.(dr/dQ dQ) + c r.[ (d(dr/dQ)/dQ [dQ]) m + dr/dQ (dQ x w_cam,phi) ]
 *   c' = 0 without a kernel; Huber: -d / (2 s^(3/2)) for s > d^2, else 0; Cauchy: -1 / (d^2 (1 + s/d^2)^2).
 * grad_depth (B,H,W) and grad_flow (B,2,H,W), float32, are written in full: exactly 0 at every invalid pixel and over a whole link
 * whose status_or_null (B, int; NULL: all 0) is not 0.  All arithmetic is float64, rounded once at the store; no reduction and no
 * atomics: the same inputs give the same bits.
 *
 * islam_dense_reproj_ift_weights: the w for which that derivative is the gradient of a loss L on the pose a refinement ended at
 * (implicit function theorem: at the optimum xi*(theta) = -H^-1 g(theta) to first order, so dL = w^T dg with w = -H^-1 v).
 * grad_motion (B,7) = dL/d[t, q xyzw] at `motion` (B,7); v = dL/dxi on motion Exp(xi):  v_rho = R_motion^T dL/dt,
 * v_phi = 1/2 E^T dL/dq, E (4x3) = d(q (x, 1))/dx at 0;  H (B,6,6): the undamped matrix islam_dense_reproj_refine returns.
 * Using H for dg/dxi is the Gauss-Newton approximation: exact where the residual vanishes, off by terms proportional to the
 * residual elsewhere.  status_out (B): status_in_or_null's value where that is not 0, ISLAM_DENSE_REPROJ_NOTPD where the Cholesky
 * of H meets a non-positive pivot, else 0; w (B,6) is 0 for a link whose status_out is not 0.  One launch; the host never waits.
 *
 * Both return ISLAM_EARG before any device work for B (H, W) < 1 (or H*W > 2^30), an unknown robust kind, robust_delta <= 0, a NULL
 * pointer other than mask, rgb2imu and the incoming status. */
int islam_dense_reproj_vjp(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                           const double* rgb2imu, const double* intr4, int B, int H, int W, int robust_kind,
                           double robust_delta, const double* w, const int* status_or_null, float* grad_depth,
                           float* grad_flow, void* stream);
int islam_dense_reproj_ift_weights(const double* H, const double* motion, const double* grad_motion,
                                   const int* status_in_or_null, int B, double* w, int* status_out, void* stream);

/* Joint two-view dense bundle adjustment: the pose of a link AND one inverse depth per pixel, the stereo depth as a Gaussian prior,
 * the depths eliminated pixel by pixel.  Per link b and pixel i, with the symbols above: the unknown
 * inverse depth rho_i; the prior rho0_i = 1/depth_i, computed in float64 from the float32 map; the prior weight w_b > 0
 * (prior_weight (B) float64), w = sigma_px^2 / sigma_rho^2, so that the sums stay in px^2.
 *   P = (1/rho) ray,  ray = ((u - cx)/fx, (v - cy)/fy, 1),   Q = T^-1 P;   r, valid, s, c, rho_rob(s), Jq = dr/dQ, J_cam: as above
 *   jd = Jq R ray (-1/rho^2)                                  (2-vector dr/drho; R the rotation of T^-1)
 *   h_pd = c J_cam^T jd (6),   h_dd = c jd^T jd + w,   g_d = c jd^T r + w (rho - rho0)
 *   S_cam = sum_valid ( c J_cam^T J_cam - h_pd h_pd^T / h_dd ),   gs_cam = sum_valid ( c J_cam^T r - h_pd g_d / h_dd )
 *   cost  = sum_valid ( rho_rob(s) + w (rho - rho0)^2 );   l1, count: as above
 * A pixel whose input depth is not finite or is <= 0 has no usable prior: it is outside the valid set at every state and carries
 * rho = 0 in the state (so does, in islam_dense_ba_normal, a pixel whose given rho is not finite or is <= 0).  For a pixel that is
 * invalid for any other reason the same formulas hold with c = 0: h_pd = 0, h_dd = w, g_d = w (rho - rho0).  The 30 camera-frame
 * sums keep the layout above ([0..20] upper triangle of S_cam, [21..26] gs_cam, [27] cost, [28] l1, [29] count) and the final step
 * is unchanged: S = A^T S_cam A, g = A^T gs_cam.  S / sigma_px^2 is the depth-marginalised information of the edge in the frame and
 * row order of islam_pvgo_run_chain_info's info_vo; H - S is positive semi-definite and S -> H as w -> infinity.
 *
 * islam_dense_ba_normal: the sums at a given state (motion, inv_depth_or_null (B,H,W) float64; NULL: rho = rho0).  Outputs and
 * scratch (islam_dense_ba_scratch_bytes(B, H, W, 0)) as islam_dense_reproj_normal.  A link whose prior_weight is not > 0 gets NaN in
 * every output.
 *
 * islam_dense_ba_refine: the Levenberg-Marquardt of islam_dense_reproj_refine (schedule, accept rule on the mean cost, min_count,
 * finiteness, lambda bounds, status words) on the joint problem.  Only the pose block is damped, (S + lambda diag S) delta = -gs;
 * the depth block is not (w > 0 keeps h_dd positive, and S stays independent of lambda).  After the pose step every pixel gets
 *   drho = -(g_d + h_pd^T delta_cam) / h_dd,  delta_cam = A delta,  evaluated at the current state;
 * a trial rho that is not finite or is <= 0 leaves that pixel at its current rho; a pixel that is invalid at the current state goes
 * back to rho0.  Pose and inverse depths are accepted or rejected together.  The inverse depths live in two (B,H,W) buffers of the
 * scratch with one selector word per link; evaluation k >= 1 forms the trial rho and evaluates at it in one launch (two sweeps over
 * a workgroup's pixels), the final kernel flips the selector on acceptance; two launches per evaluation plus one copy of the result
 * into out_inv_depth at the end, no host wait.  out_status additionally: ISLAM_DENSE_REPROJ_BADPRIOR for a link whose prior_weight
 * is not > 0 (a device value: no read-back); that link's pose comes back as given, its inverse depths as the prior, its sums NaN.
 * Outputs: out_motion (B,7), out_inv_depth (B,H,W) float64 and out_S .. out_sums AT them: the same bits islam_dense_ba_normal
 * gives at (out_motion, out_inv_depth).  scratch: islam_dense_ba_scratch_bytes(B, H, W, iters).  ISLAM_EARG before any device work
 * for the cases of islam_dense_reproj_normal / _refine, a NULL prior_weight and a NULL out_inv_depth. */
#define ISLAM_DENSE_REPROJ_BADPRIOR 3
size_t islam_dense_ba_scratch_bytes(int B, int H, int W, int iters_or_0);
int islam_dense_ba_normal(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                          const double* rgb2imu, const double* intr4, const double* prior_weight,
                          const double* inv_depth_or_null, int robust_kind, double robust_delta, double* out_S, double* out_g,
                          double* out_cost, double* out_l1, double* out_count, double* out_sums, void* scratch, int B, int H,
                          int W, void* stream);
int islam_dense_ba_refine(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                          const double* rgb2imu, const double* intr4, const double* prior_weight, int robust_kind,
                          double robust_delta, int iters, double damping, double min_count, double* out_motion,
                          double* out_inv_depth, double* out_S, double* out_g, double* out_cost, double* out_l1,
                          double* out_count, double* out_sums, double* out_lambda, int* out_accepted, int* out_rejected,
                          int* out_status, double* trace, int trace_cap, void* scratch, int B, int H, int W, void* stream);

/* The gradient of the joint refinement with respect to depth and flow.  At the state islam_dense_ba_refine
 * returned -- motion T* (B,7), inv_depth rho* (B,H,W) -- the joint gradient G = [g_p; g_d] vanishes (g_p = A^T sum c J_cam^T r,
 * g_d,i as above).  For a loss L on the outputs, with v_p = dL/dxi on T* Exp(xi) (from grad_motion (B,7) = dL/d[t, q xyzw] by the
 * conversion of islam_dense_reproj_ift_weights) and v_d,i = dL/drho*_i (grad_inv_depth_or_null (B,H,W) float64; NULL: 0), the implicit
 * function theorem gives dL = lambda^T dG with H_full lambda = -v, H_full the Gauss-Newton matrix of the joint problem.  The depths
 * are eliminated pixel by pixel, as in the forward pass:
 *   u_cam = sum_valid h_pd,i v_d,i / h_dd,i                       (6 sums per link; 0 when no gradient arrives on inv_depth)
 *   S lambda_p = -(v_p - A^T u_cam)                               (S (B,6,6): the undamped matrix islam_dense_ba_refine returns)
 *   lambda_cam = A lambda_p
 *   valid pixel:                 lambda_d,i = -(v_d,i + h_pd,i^T lambda_cam) / h_dd,i
 *   invalid pixel with a prior:  lambda_d,i = -v_d,i / w          (the same formula at c = 0)
 *   pixel without a prior (depth not finite or <= 0): no gradient
 * and with Phi = lambda_p^T g_p + sum lambda_d,i g_d,i, the state, lambda and the valid set held fixed:
 *   q_i = J_cam,i lambda_cam + jd_i lambda_d,i,   e_i = c q_i + 2 c' (q_i.r_i) r_i        (c' as for islam_dense_reproj_vjp)
 *   dL/dflow_i = -e_i  (valid pixels; 0 elsewhere),   dL/ddepth_i = w lambda_d,i / depth_i^2  (every pixel with a prior)
 * The input depth enters only through the prior rho0 = 1/depth (dg_d/drho0 = -w, drho0/dz = -1/z^2), so both derivatives of Phi are
 * exact; a masked-out pixel gets dL/ddepth = -v_d / depth^2, the derivative of rho* = 1/depth.  H_full is the Gauss-Newton matrix:
 * exact where r = 0 and rho = rho0, off by terms proportional to the residuals elsewhere, and the formula assumes the refinement has
 * converged in pose and depths.  The start pose and prior_weight get no gradient.
 *
 * islam_dense_ba_ift_weights: lambda_p (B,6) float64.  u_cam is reduced like the sums above (NBLK rows of 6 per link by plain stores,
 * added in fixed order: the same inputs give the same bits), a launch that is skipped when grad_inv_depth_or_null is NULL; the
 * solve is one more.  scratch: islam_dense_ba_adjoint_scratch_bytes(B).  status_out (B): status_in_or_null's value where that is not
 * 0, ISLAM_DENSE_REPROJ_BADPRIOR where prior_weight is not > 0, ISLAM_DENSE_REPROJ_NOTPD where the Cholesky of S meets a
 * non-positive pivot, else 0; lambda_p is 0 for a link whose status_out is not 0.
 *
 * islam_dense_ba_vjp: grad_depth (B,H,W) and grad_flow (B,2,H,W), float32, written in full from lambda_p and grad_inv_depth_or_null:
 * exactly 0 where the formulas give 0 and over a whole link whose status_or_null (B; NULL: all 0) is not 0 or whose prior_weight is
 * not > 0.  All arithmetic is float64, rounded once at the store; one launch, no reduction, no atomics.
 *
 * Both return ISLAM_EARG before any device work for B, H, W < 1 (or H*W > 2^30), an unknown robust kind, robust_delta <= 0, and a
 * NULL pointer other than mask, rgb2imu, grad_inv_depth_or_null and the incoming status.  The host never waits. */
size_t islam_dense_ba_adjoint_scratch_bytes(int B);
int islam_dense_ba_ift_weights(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                               const double* rgb2imu, const double* intr4, const double* prior_weight, const double* inv_depth,
                               int robust_kind, double robust_delta, const double* S, const double* grad_motion,
                               const double* grad_inv_depth_or_null, const int* status_in_or_null, void* scratch, int B, int H,
                               int W, double* lambda_p, int* status_out, void* stream);
int islam_dense_ba_vjp(const float* depth, const float* flow, const uint8_t* mask, const double* motion, const double* rgb2imu,
                       const double* intr4, const double* prior_weight, const double* inv_depth, int robust_kind,
                       double robust_delta, const double* lambda_p, const double* grad_inv_depth_or_null,
                       const int* status_or_null, float* grad_depth, float* grad_flow, int B, int H, int W, void* stream);

/* Per-pixel prior weights and the posterior variance of the inverse depths.
 *
 * Weight map.  prior_scale (B,H,W) float32, m: the prior weight of pixel i of link b is w_i = prior_weight[b] * (double)m_i (one
 * rounding), and w_i stands wherever the definitions above write w: h_dd = c jd^T jd + w_i, g_d = c jd^T r + w_i (rho - rho0), the
 * cost term w_i (rho - rho0)^2.  A pixel has a usable prior iff its depth is finite and > 0 AND m_i is finite and > 0; otherwise it
 * is outside the valid set at every state and carries rho = 0, exactly like a pixel whose depth is <= 0.  BADPRIOR stays the
 * per-link verdict on prior_weight[b].  islam_dense_ba_normal_map / islam_dense_ba_refine_map are islam_dense_ba_normal / _refine
 * with prior_scale after prior_weight: the same launches (the partial kernel reads 4 B more per pixel and sweep), outputs, status
 * words and scratch (islam_dense_ba_scratch_bytes); a NULL prior_scale is ISLAM_EARG beside their other cases.  m = 1 everywhere
 * gives the sums of the entry points without a map.
 *
 * Posterior variance, at a state (motion, inv_depth_or_null; NULL: rho = rho0), in units of sigma_px^2, in the Gauss-Newton
 * approximation with the robust weight c (the approximation of S as an information):
 *   h_cam = J_cam^T e (6),  e = c jd,  h_dd = e.jd + w_i
 *   mode 0, marginal over the pose:    v_i = 1/h_dd + h_cam^T S_cam^-1 h_cam / h_dd^2
 *   mode 1, conditional on the pose:   v_i = 1/h_dd
 *   a pixel with a prior that is invalid at the state (c = 0):          v_i = 1/w_i
 *   no usable prior, or a state rho that is not finite or is <= 0:      v_i = NaN
 * S_cam: sums[0..20] of the same state (sums (B,30) as islam_dense_ba_normal / _refine return them; no mount transform is needed,
 * h^T S^-1 h is invariant under A).  var(rho_i) = sigma_px^2 v_i, and to first order sigma_depth,i = sqrt(var(rho_i)) / rho_i^2.  In
 * exact arithmetic 1/h_dd <= v_i <= 1/w_i.  prior_scale_or_null NULL: w_i = prior_weight[b].
 * islam_dense_ba_depth_var: two launches, no host wait, no atomics (a repeat gives the same bits).  The first (one workgroup per
 * link) forms out_status (B): status_or_null's value where that is not 0, ISLAM_DENSE_REPROJ_BADPRIOR where prior_weight is not > 0,
 * ISLAM_DENSE_REPROJ_NOTPD where one of the 21 sums is not finite or (mode 0) the Cholesky of S_cam meets a non-positive pivot, else
 * 0; in mode 0 it leaves S_cam^-1 in scratch (islam_dense_ba_depth_var_scratch_bytes(B)).  The second writes out_var (B,H,W)
 * float64 in full, one store per pixel; a link whose out_status is not 0 gets NaN at every pixel.  ISLAM_EARG before any device
 * work for a bad shape, an unknown robust kind, robust_delta <= 0, a mode other than 0 / 1, and a NULL pointer other than mask,
 * rgb2imu, prior_scale_or_null, inv_depth_or_null and status_or_null. */
int islam_dense_ba_normal_map(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                              const double* rgb2imu, const double* intr4, const double* prior_weight, const float* prior_scale,
                              const double* inv_depth_or_null, int robust_kind, double robust_delta, double* out_S, double* out_g,
                              double* out_cost, double* out_l1, double* out_count, double* out_sums, void* scratch, int B, int H,
                              int W, void* stream);
int islam_dense_ba_refine_map(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                              const double* rgb2imu, const double* intr4, const double* prior_weight, const float* prior_scale,
                              int robust_kind, double robust_delta, int iters, double damping, double min_count, double* out_motion,
                              double* out_inv_depth, double* out_S, double* out_g, double* out_cost, double* out_l1,
                              double* out_count, double* out_sums, double* out_lambda, int* out_accepted, int* out_rejected,
                              int* out_status, double* trace, int trace_cap, void* scratch, int B, int H, int W, void* stream);
size_t islam_dense_ba_depth_var_scratch_bytes(int B);
int islam_dense_ba_depth_var(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                             const double* rgb2imu, const double* intr4, const double* prior_weight,
                             const float* prior_scale_or_null, const double* inv_depth_or_null, const double* sums,
                             const int* status_or_null, int robust_kind, double robust_delta, int mode, double* out_var,
                             int* out_status, void* scratch, int B, int H, int W, void* stream);

/* The vector-Jacobian product of islam_dense_ba_depth_var: the TOTAL derivative of v in the state rho
 * (inv_depth), motion and flow.  S_cam is a function of that same state, not an independent input: sums are by contract the sums at
 * the state (islam_dense_ba_refine returns them bit-equal to islam_dense_ba_normal there), and no gradient on sums is taken or given.
 * Held fixed and read from the forward evaluation: which pixels are valid (the clauses of the front, a usable prior, rho finite and
 * > 0) and the branch of the Huber kernel.  prior_weight, prior_scale, intr4, the mount, the mask and the stored depth (which enters
 * only through "has a prior") get no gradient.
 * Notation at a valid pixel: (R, t) = T^-1, Q = R ray / rho + t, d = -R ray / rho^2, J_q = dr/dQ = [[a, 0, bq], [0, cq, dq]],
 * J = J_q [-I, [Q]x] (rows ju, jv), jd = J_q d, s = |r|^2, c = rho_rob'(s), c' = dc/ds, h_dd = c |jd|^2 + w_i.  With g_i the cotangent
 * of v_i (grad_var (B,H,W) float64; read at a valid pixel only, so it may be NaN elsewhere) and
 *   a = J^T jd (h_cam = c a),  k = |jd|^2,  q = a^T S_cam^-1 a,  y = c S_cam^-1 a,
 *   G = -sum_valid g_i y_i y_i^T / h_dd,i^2   (the cotangent of S_cam; mode 0 only, G = 0 in mode 1),   n = a^T G a,   tau = <G, J^T J>,
 * everything else is the gradient of one scalar per pixel at fixed S_cam^-1 and G,
 *   phi_i = g_i (1 / h_dd + c^2 q / h_dd^2) + c tau - c^2 n / h_dd      (mode 1: g_i / h_dd),
 * the last two terms being <G, J^T (c I - e e^T / h_dd) J>, the pixel's own share of S_cam:
 *   phi_h = -g / h_dd^2 - 2 g c^2 q / h_dd^3 + c^2 n / h_dd^2,   phi_c = 2 g c q / h_dd^2 + tau - 2 c n / h_dd + k phi_h,   phi_k = c phi_h,
 *   a~ = 2 (g c^2 / h_dd^2 S_cam^-1 - c^2 / h_dd G) a,   J~ = jd a~^T + 2 c J G,   jd~ = J a~ + 2 phi_k jd,   r~ = 2 c' phi_c r,
 * chained through J, jd and r = pi(Q) - (pixel + flow) to Q~, d~, then rho~ = -(Q~.R ray) / rho^2 + 2 (d~.R ray) / rho^3,
 * R~ = (Q~ / rho - d~ / rho^2) ray^T, t~ = Q~ (12 sums per link) and the flow cotangent -r~ (identically zero without a robust kernel).
 * Outputs, all written in full by plain stores (no memset, no atomics; a repeat gives the same bits): grad_inv_depth (B,H,W)
 * float64; grad_flow (B,2,H,W) float32 (rounded once at the store); grad_motion (B,7) float64 on the plain components [t, q xyzw] of
 * motion, the cotangent of (R, t) chained through the matrix of the quaternion, the inverse and the mount conjugation as the forward
 * pass writes them (no unit-norm assumption: the convention of islam_depth_propagate_vjp's grad_motion); out_status (B) as
 * islam_dense_ba_depth_var forms it.  A pixel whose v is 1 / w_i or NaN reaches no input: exact zeros.  A link whose out_status is
 * not 0: zeros everywhere, its seven entries of grad_motion included.
 * At most four launches on `stream`, no host wait: depth_var_factor_kernel on sums (the forward call's bits, so nothing has to be
 * saved), in mode 0 depth_var_adj_partial_kernel (the 21 sums of G, one row per workgroup), depth_var_vjp_kernel (the pixel pass and the
 * 12 pose sums), depth_var_pose_kernel (one workgroup per link).  scratch: islam_dense_ba_depth_var_vjp_scratch_bytes(B) bytes.
 * ISLAM_EARG before any device work under the rules of islam_dense_ba_depth_var, and for a NULL inv_depth, grad_var or output. */
size_t islam_dense_ba_depth_var_vjp_scratch_bytes(int B);
int islam_dense_ba_depth_var_vjp(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                 const double* rgb2imu_or_null, const double* intr4, const double* prior_weight,
                                 const float* prior_scale_or_null, const double* inv_depth, const double* sums,
                                 const int* status_or_null, int robust_kind, double robust_delta, int mode, const double* grad_var,
                                 double* grad_inv_depth, float* grad_flow, double* grad_motion, int* out_status, void* scratch, int B,
                                 int H, int W, void* stream);

/* The gradient of the joint refinement with the exact (Newton) Hessian and per-pixel prior weights.  The
 * adjoint system of islam_dense_ba_ift_weights / islam_dense_ba_vjp above, with the Gauss-Newton blocks replaced by one half of the
 * Hessian of the cost in the same per-pixel elimination; all fp64.  The state is what islam_dense_ba_refine(_map) returned: T*, rho*;
 * (R, t) = T^-1 in the camera frame, the chart T* Exp(xi), so Q(xi, rho) = Exp(-xi_cam^)(R ray / rho + t) with xi_cam = A xi exactly.
 * Per valid pixel, with the quantities defined above:
 *   J_q = dr/dQ = [[a, 0, bq], [0, cq, dq]]      D_p = [-I, [Q]x] (3x6)      J_cam = J_q D_p
 *   dR = R ray      d = -dR / rho^2      jd = J_q d
 *   M  = c I_2 + 2 c' r r^T                      y = c r      n = J_q^T y  (3)
 *   B  = -iz (n e_z^T + e_z n^T)                 (the Hessian in Q of y^T pi(Q); iz = 1 / Q_z)
 *   K  = J_q^T M J_q + B                         (3x3, symmetric)
 *   n_pp = D_p^T K D_p + C      C_rho,phi = [n]x / 2,  C_phi,rho = -[n]x / 2,  C_phi,phi = (n Q^T + Q n^T) / 2 - (n.Q) I_3,  C_rho,rho = 0
 *   n_pd = D_p^T K d + [0 ; n x d]
 *   n_dd = d^T K d - (2 / rho) (n.d) + w_i
 * C comes from the second-order term xi^ xi^ / 2 of Exp(-xi^).  The Gauss-Newton blocks are these with K -> c J_q^T J_q and every term
 * in n dropped.  w_i = prior_weight[b], or prior_weight[b] * (double)m_i under prior_scale_or_null (B,H,W) float32 with the rule
 * above: a pixel has a usable prior iff its depth and m_i are finite and > 0.  The valid set and the Huber branch are held fixed.
 *   S_N,cam = sum_valid ( n_pp - n_pd n_pd^T / n_dd )        u_cam = sum_valid n_pd v_d / n_dd
 *   S_N = A^T S_N,cam A          S_N lambda_p = -( v_p - A^T u_cam )          lambda_cam = A lambda_p
 *   valid pixel:                 lambda_d = -( v_d + n_pd^T lambda_cam ) / n_dd
 *   invalid pixel with a prior:  lambda_d = -v_d / w_i                        no usable prior: no gradient
 *   q = J_cam lambda_cam + jd lambda_d     e = c q + 2 c' (q.r) r
 *   dL/dflow = -e  (valid pixels; 0 elsewhere)               dL/ddepth = w_i lambda_d / depth^2  (every pixel with a usable prior)
 * Fallback: a valid pixel whose n_dd is not > 0 (NaN included) takes its three Gauss-Newton blocks (c J_cam^T J_cam, h_pd, h_dd)
 * instead, in the reduction and in the streaming pass alike, and is counted per link (fallback_count (B) int32).
 *
 * islam_dense_ba_newton_weights: two launches, no host wait, no atomics.  The first reduces 28 sums per link (the 21 of the upper
 * triangle of S_N,cam, the 6 of u_cam -- zeros when grad_inv_depth_or_null is NULL -- and the fallback count) as NBLK rows by plain
 * stores into scratch (islam_dense_ba_newton_scratch_bytes(B)); a link whose incoming status is not 0 or whose prior_weight is not > 0
 * stores zeros without reading its pixels.  The second adds the rows in fixed order and writes lambda_p (B,6), S_newton_or_null
 * (B,6,6; body frame, symmetric to the bit; NULL: not wanted), fallback_count (B) and status_out (B): status_in_or_null's value where
 * that is not 0, ISLAM_DENSE_REPROJ_BADPRIOR where prior_weight is not > 0, ISLAM_DENSE_REPROJ_NOTPD where S_N is not finite or its
 * Cholesky meets a non-positive pivot, else 0; lambda_p is 0 for a link whose status_out is not 0.  S_N is the Hessian of the
 * marginalised cost, not an information matrix: it need not be positive definite away from a minimum.
 * islam_dense_ba_newton_vjp: grad_depth (B,H,W) and grad_flow (B,2,H,W), float32, written in full: exactly 0 where the formulas give
 * 0 and over a whole link whose status_or_null is not 0 or whose prior_weight is not > 0.  One launch, rounded once at the store.
 * Both return ISLAM_EARG before any device work for B, H, W < 1 (or H*W > 2^30), an unknown robust kind, robust_delta <= 0, and a
 * NULL pointer other than mask, rgb2imu, prior_scale_or_null, grad_inv_depth_or_null, S_newton_or_null and the incoming status. */
size_t islam_dense_ba_newton_scratch_bytes(int B);
int islam_dense_ba_newton_weights(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                  const double* rgb2imu, const double* intr4, const double* prior_weight,
                                  const float* prior_scale_or_null, const double* inv_depth, int robust_kind, double robust_delta,
                                  const double* grad_motion, const double* grad_inv_depth_or_null, const int* status_in_or_null,
                                  void* scratch, int B, int H, int W, double* lambda_p, double* S_newton_or_null,
                                  int* fallback_count, int* status_out, void* stream);
int islam_dense_ba_newton_vjp(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                              const double* rgb2imu, const double* intr4, const double* prior_weight,
                              const float* prior_scale_or_null, const double* inv_depth, int robust_kind, double robust_delta,
                              const double* lambda_p, const double* grad_inv_depth_or_null, const int* status_or_null,
                              float* grad_depth, float* grad_flow, int B, int H, int W, void* stream);

/* Depth propagation: the inverse depths rho and variances s (1/m^2, real variances: sigma_px^2 v of
 * islam_dense_ba_depth_var) of the first frame of link b carried into the pixel grid of its second frame and fused there with that
 * frame's own measurement.  All device arithmetic is fp64, every operation rounded on its own (nothing is contracted).  With (R, t) =
 * T^-1 of motion[b] and rgb2imu as above, (fx, fy, cx, cy) = intr4[b] for both frames, source pixel i = v W + u, ray (xh, yh, 1) =
 * ((u - cx) / fx, (v - cy) / fy, 1), rho = inv_depth[b,i], s = var_inv_depth[b,i]:
 *   a = R[2,:].ray,  Q = R ray / rho + t,  rho' = 1 / Q.z,  J = a rho'^2 / rho^2 (= drho'/drho),  s' = J^2 s + process_var[b],
 *   u2 = fx Q.x / Q.z + cx,  v2 = fy Q.y / Q.z + cy,  iu = (int)floor(u2 + 0.5),  iv = (int)floor(v2 + 0.5).
 * Source i is a candidate for target j = iv W + iu iff the link's incoming status is 0 (or status_or_null is NULL), the mask (if
 * given) is set at i, rho and s are finite and > 0, Q.z > 0.1, 0 <= iu < W, 0 <= iv < H, and s' is finite.  Z-buffer: the winner at
 * j is the candidate with the largest key (bits of (float)rho', 0xFFFFFFFF - i), compared lexicographically: the nearest surface, the
 * smaller source index on equal fp32 keys; key 0: nothing landed.  Measurement (optional; depth_next and var_next (B,H,W) float32, the
 * depth of the second frame and the variance of its inverse depth, both or neither): present at j iff depth_next and var_next are
 * finite and > 0; rho_m = 1 / depth_next, s_m = var_next.  Fusion at j:
 *   both present:  d = rho' - rho_m;  gate > 0 and d^2 > gate^2 (s' + s_m): gated, the measurement alone;  otherwise
 *                  rho_f = (rho' s_m + rho_m s') / (s' + s_m),  s_f = s' s_m / (s' + s_m);
 *   one present: that one;  none: rho_f = 0, s_f = NaN ("no prior at this pixel").
 * Outputs, all written in full: out_inv_depth, out_var (B,H,W) float64 = rho_f, s_f; out_depth (B,H,W) float32 = 1 / rho_f where
 * rho_f > 0, else the bits of depth_next (0 without one); out_source (B,H,W) int32: the winning source index, -1 for none; out_flags
 * (B,H,W) uint8: bit 0 propagated present, bit 1 measurement present, bit 2 gated out; out_status (B): status_or_null's value where
 * that is not 0, ISLAM_DENSE_REPROJ_BADPRIOR where process_var[b] is negative or not finite (formed on the device), else 0; a link
 * whose out_status is not 0 propagates nothing and gets the measurement alone at every pixel.
 * islam_depth_propagate: one hipMemsetAsync of the key buffer (scratch, islam_depth_propagate_scratch_bytes(B, H, W) = B H W 8 bytes
 * rounded up) and two launches on `stream`, no host wait: depth_splat_kernel (one 64-bit atomic maximum per candidate; a maximum does
 * not depend on the order of arrival, so a repeat gives the same bits) and depth_fuse_kernel (plain stores).  ISLAM_EARG before any
 * device work for B, H, W < 1 or H*W > 2^30 (which keeps every source index below 2^32 - 1), a NULL pointer other than mask_or_null,
 * rgb2imu_or_null, status_or_null, depth_next_or_null and var_next_or_null, depth_next without var_next or the reverse, and a gate
 * that is negative or not finite. */
size_t islam_depth_propagate_scratch_bytes(int B, int H, int W);
int islam_depth_propagate(const double* inv_depth, const double* var_inv_depth, const uint8_t* mask_or_null, const double* motion,
                          const double* rgb2imu_or_null, const double* intr4, const int* status_or_null, const double* process_var,
                          const float* depth_next_or_null, const float* var_next_or_null, double gate, double* out_inv_depth,
                          double* out_var, float* out_depth, int* out_source, uint8_t* out_flags, int* out_status, void* scratch,
                          int B, int H, int W, void* stream);

/* The vector-Jacobian product of islam_depth_propagate.  The map is piecewise smooth: the target pixel
 * (iu, iv), the z-buffer winner and the row of the fusion table (the gate decision included) are constant on a piece and get no
 * derivative; source (out_source) and flags (out_flags) of the forward call say which piece a target is on, and the arithmetic of that
 * piece is differentiated exactly, in fp64.  Since (u2, v2) only select a target, rho' and s' depend on the pose through a and t_z
 * (= t[2]) alone:
 *   drho'/drho = J,  drho'/da = -rho'^2 / rho,  drho'/dt_z = -rho'^2,
 *   dJ/drho = 2 J (J / rho' - 1 / rho),  dJ/da = (rho'^2 / rho^2)(1 - 2 a rho' / rho),  dJ/dt_z = -2 J rho',
 *   ds'/ds = J^2,  ds'/dx = 2 J s dJ/dx  for x in (rho, a, t_z);
 * fusion, with D = s' + s_m and rho_m = 1 / depth_next:
 *   both, not gated:  drho_f/drho' = s_m / D,  drho_f/drho_m = s' / D,  drho_f/ds' = (rho_m - rho_f) / D,  drho_f/ds_m = (rho' - rho_f) / D,
 *                     ds_f/ds' = s_m^2 / D^2,  ds_f/ds_m = s'^2 / D^2;
 *   gated, or measured only:  rho_f = rho_m, s_f = s_m;   propagated only:  rho_f = rho', s_f = s';   nothing: no input is reached;
 *   drho_m/ddepth_next = -rho_m^2,  ds_m/dvar_next = 1.
 * Cotangents (float64 (B,H,W), NULL: zero): grad_out_inv_depth on rho_f, grad_out_var on s_f; an entry is read only where flags is not
 * 0, so it may be NaN where nothing is known.  Outputs, all written in full by plain stores (no memset, no atomics; a repeat gives the
 * same bits): grad_inv_depth, grad_var_inv_depth (B,H,W) float64 on rho and s, exactly 0 at a source pixel that did not win its target
 * (read from source, never re-derived); grad_motion (B,7) float64 on the plain components [t, q xyzw] of motion, the cotangent of (R20,
 * R21, R22, t_z) chained through the matrix of the quaternion, the inverse and the mount conjugation as the forward pass writes them;
 * grad_depth_next, grad_var_next (B,H,W) float32 (both or neither; rounded once at the store).  out_status: the forward call's; a
 * link whose entry is not 0 propagated nothing: its grad_inv_depth, grad_var_inv_depth and grad_motion are exact zeros, and its
 * measurement rows still pass their gradient on.  process_var, gate, intr4, the mount and the mask get no gradient (the mask is not
 * needed: source carries the winners).  scratch: islam_depth_propagate_vjp_scratch_bytes(B) bytes (B x 64 rows of four partial sums).
 * Two launches on `stream`, no host wait: depth_prop_vjp_kernel (every pixel as a target and as a source; the four pose sums reduced
 * in a fixed order) and depth_prop_pose_kernel (one workgroup per link).  ISLAM_EARG before any device work for a bad shape (as
 * above), a NULL pointer other than rgb2imu_or_null, depth_next_or_null, var_next_or_null, the two cotangents and the two measurement
 * gradients, depth_next without var_next or the reverse (likewise their gradients), and a measurement gradient without a measurement. */
size_t islam_depth_propagate_vjp_scratch_bytes(int B);
int islam_depth_propagate_vjp(const double* inv_depth, const double* var_inv_depth, const double* motion, const double* rgb2imu_or_null,
                              const double* intr4, const double* process_var, const float* depth_next_or_null,
                              const float* var_next_or_null, const int* source, const uint8_t* flags, const int* out_status,
                              const double* grad_out_inv_depth_or_null, const double* grad_out_var_or_null, double* grad_inv_depth,
                              double* grad_var_inv_depth, double* grad_motion, float* grad_depth_next_or_null,
                              float* grad_var_next_or_null, void* scratch, int B, int H, int W, void* stream);

/* Regularisation of a propagated map: occlusion removal, hole filling and smoothing of the inverse depths rho
 * and variances s (B,H,W) float64 that islam_depth_propagate returned without a measurement, then the fusion table above.  All device
 * arithmetic is fp64, every operation rounded on its own.  A window is the (2r+1)^2 square around a pixel clipped at the image border,
 * walked row by row, which is the order of every sum.  valid0(k): rho_k and s_k finite and > 0.  compat(k,j): (rho_k - rho_j)^2 <=
 * reg_gate^2 (s_k + s_j).
 *   1. removal (occl_radius): for a valid0 j, over k != j in the window, n_sup = #{valid0, compat}, n_occ = #{valid0, not compat,
 *      rho_k > rho_j}; j is removed iff n_occ >= occl_min and n_occ > n_sup.  valid1 = valid0 and not removed.
 *   2. filling (fill_radius): for a j in the image that is not valid1, a = the valid1 neighbour with the largest rho (the first in
 *      the window's order among equals), the cluster = {valid1 k : compat(k,a)}, n its size; if n >= fill_min, with w_k = 1 / s_k,
 *      Sw = sum w_k:  rho_j = mean = (sum w_k rho_k) / Sw,  s_j = fill_inflate (n / Sw + (sum w_k (rho_k - mean)^2) / Sw), the second
 *      sum a pass of its own with terms w_k ((rho_k - mean)(rho_k - mean)).  Only stage-1 values are read.  valid2 = valid1 or filled.
 *   3. smoothing (smooth_radius): for a valid2 j, over the valid2 k of the window (j included) with compat(k,j), on stage-2 values,
 *      w_k = 1 / (s_k + dist_var[b] (du^2 + dv^2)):  rho_j <- (sum w_k rho_k) / (sum w_k);  s_j stays.
 *   4. the fusion table of islam_depth_propagate on (rho_j, s_j, present = valid2) with depth_next, var_next and gate.
 * A radius of 0 leaves its stage out; with the three radii 0 and no measurement a map that holds (0, NaN) at its holes is returned
 * bit for bit.  Outputs as islam_depth_propagate's, all written in full.  out_flags: bit 0 valid2, bits 1 and 2 as above, bit 3 (8)
 * filled, bit 4 (16) removed by stage 1 (both where a removed pixel was filled again).  out_source: source_or_null's entry where the
 * pixel is valid1, else -1 (all -1 without a source map).  out_status (B): status_or_null's value where that is not 0,
 * ISLAM_DENSE_REPROJ_BADPRIOR where dist_var[b] (1/m^2 per px^2) is negative or not finite (formed on the device), else 0; a link
 * whose out_status is not 0 gets the measurement alone at every pixel.
 * One launch on `stream` (depth_regularize_kernel: a 32 x 8 tile with a halo of the three radii in LDS, plain stores, no atomics, so a
 * repeat gives the same bits), no host wait, no scratch: islam_depth_regularize_scratch_bytes returns 0 and scratch may be NULL.
 * ISLAM_EARG before any device work for a bad shape (as above), a NULL pointer other than source_or_null, status_or_null,
 * depth_next_or_null, var_next_or_null and scratch, depth_next without var_next or the reverse, a radius outside 0..2, occl_min or
 * fill_min < 1, fill_inflate < 1 or not finite, reg_gate not finite or not > 0, and a gate that is negative or not finite. */
size_t islam_depth_regularize_scratch_bytes(int B, int H, int W);
int islam_depth_regularize(const double* inv_depth, const double* var_inv_depth, const int* source_or_null, const int* status_or_null,
                           const double* dist_var, const float* depth_next_or_null, const float* var_next_or_null, double gate,
                           int occl_radius, int occl_min, int fill_radius, int fill_min, double fill_inflate, int smooth_radius,
                           double reg_gate, double* out_inv_depth, double* out_var, float* out_depth, int* out_source,
                           uint8_t* out_flags, int* out_status, void* scratch, int B, int H, int W, void* stream);

/* The vector-Jacobian product of islam_depth_regularize, on the piece its forward pass chose, in fp64.  Held
 * fixed (piecewise constant, no derivative): valid0 and every compat decision; the removed set of stage 1; for each filled hole j its
 * anchor a_j, its cluster C_j and n_j = |C_j|; the filled set; each pixel's smoothing set N3(j) (the valid2 k of the window with
 * compat(k,j) on stage-2 values, j included); the row of the fusion table and the gate decision.  dist_var, gate, the stage arguments
 * and the prior weights get no gradient.  The sets are recomputed from inv_depth, var_inv_depth and the stage arguments with the
 * forward's own device functions; the row of the fusion table is read from flags (the forward call's out_flags).  With (g_rho, g_s)
 * the cotangents of out_inv_depth and out_var, read only where (flags & 3) != 0 (elsewhere they may be NaN), NULL meaning zero:
 *   4. fusion: the table of islam_depth_propagate_vjp on (rho3_j, s2_j, measurement) gives g3rho_j, g3s_j and grad_depth_next,
 *      grad_var_next (float32, one rounding each, drho_m/ddepth_next = -rho_m^2).
 *   3. smoothing: rho3_j = (sum_{k in N3(j)} w_kj rho2_k) / S_j, w_kj = 1 / (s2_k + dist_var (du^2 + dv^2)), S_j = sum w_kj, s passes
 *      through.  For a valid2 k, over the valid2 j of k's window with compat(k,j) (compat is symmetric on the same bits):
 *        g2rho_k = sum_j g3rho_j w_kj / S_j,   g2s_k = g3s_k - sum_j g3rho_j w_kj^2 (rho2_k - rho3_j) / S_j;   smooth_radius 0: g2 = g3.
 *   2. filling: at a filled j, w_k = 1 / s_k, S = sum_{C_j} w_k, e_k = rho_k - rho2_j, f = fill_inflate, s2_j = f (n_j + sum w_k e_k^2) / S:
 *        drho2_j/drho_k = w_k / S,          drho2_j/ds_k = -w_k^2 e_k / S,
 *        ds2_j/drho_k = 2 f w_k e_k / S,    ds2_j/ds_k = w_k^2 (s2_j - f e_k^2) / S
 *      (the terms through the mean inside the scatter carry sum w_k e_k = 0 and are dropped).  For a valid1 k: g1_k = g2_k plus the sum
 *      of these over the filled j within fill_radius with compat(k, a_j);  fill_radius 0: g1 = g2 on valid1.
 *   1. removal: grad_inv_depth_k = g1rho_k, grad_var_inv_depth_k = g1s_k at valid1 pixels, exact zeros at every other pixel (holes,
 *      removed pixels whether refilled or not, inputs that are not finite or not positive).
 * A link with a status (status_or_null's entry not 0, or dist_var[b] negative or not finite) gets exact zeros on both state gradients;
 * its measurement rows still pass their gradient (the "measured only" row).  All outputs are written in full by plain stores, every sum
 * is one thread's over a window in row-major order: no atomics, no memset, a repeat gives the same bits.  scratch:
 * islam_depth_regularize_vjp_scratch_bytes(B, H, W) bytes (eleven float64 maps and one byte map between the kernels).  At most three
 * launches on `stream`, no host wait: depth_reg_front_kernel (stages 1-3 recomputed on the forward's tile, the fusion table
 * differentiated), depth_reg_smooth_adj_kernel (stage 3; left out for smooth_radius 0) and depth_reg_fill_adj_kernel (stages 2 and 1,
 * the final stores).  ISLAM_EARG before any device work under the rules of islam_depth_regularize, for a NULL flags, output or scratch
 * pointer, grad_depth_next without grad_var_next or the reverse, and a measurement gradient without a measurement. */
size_t islam_depth_regularize_vjp_scratch_bytes(int B, int H, int W);
int islam_depth_regularize_vjp(const double* inv_depth, const double* var_inv_depth, const int* status_or_null, const double* dist_var,
                               const float* depth_next_or_null, const float* var_next_or_null, double gate, int occl_radius,
                               int occl_min, int fill_radius, int fill_min, double fill_inflate, int smooth_radius, double reg_gate,
                               const uint8_t* flags, const double* grad_out_inv_depth_or_null, const double* grad_out_var_or_null,
                               double* grad_inv_depth, double* grad_var_inv_depth, float* grad_depth_next_or_null,
                               float* grad_var_next_or_null, void* scratch, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------- IMU pre-integration */

/* Replaces the frame loop of imu_integrator.py:116-158 and pp.module.IMUPreintegrator.forward
 * (integrate + predict; the reference discards the covariance PyPose propagates beside them: islam_imu_preint_cov below computes it).
 * dt (S), gyro (S,3), acc (S,3): the batch slice (already bias-corrected / denoised);
 * seg (nframes+1) int64: sample offset of each frame boundary inside the slice;
 * init_pos(3), init_rot(4), init_vel(3); motion_mode as imu_integrator.py:69-80.
 * max_frame_samples = max_i (seg[i+1]-seg[i]) (known on the host from rgb2imu_sync).
 * Outputs: world mode nframes+1 rows (row 0 = init), motion mode nframes rows.
 * scratch: at least islam_imu_scratch_bytes(S, nframes, dtype) bytes.  Calls that may run CONCURRENTLY (different streams) must not share
 * a scratch buffer: it holds the hand-off counter between the two workgroups of the world-row kernel.  If that hand-off ever times out
 * (bounded wait), out_pos / out_vel are filled with NaN rather than left half-written. */
size_t islam_imu_scratch_bytes(int64_t S, int nframes, int dtype);
int islam_imu_preint(const void* dt, const void* gyro, const void* acc, const int64_t* seg, int nframes,
                     int64_t S, int max_frame_samples, const void* init_pos, const void* init_rot,
                     const void* init_vel, double gravity, int motion_mode, void* out_pos, void* out_rot,
                     void* out_vel, void* scratch, int dtype, void* stream);

/* Both call forms of IMUModule.integrate on one frame range from ONE pass (the reference's loop calls integrate twice per batch with
 * the same range and init['rot']: train.py:200-215 -> imu_integrator.py:69-164): world_* get nframes + 1 rows (row 0 = the initial
 * state), motion_* nframes rows (every frame from p = v = 0).  Bit-identical to islam_imu_preint(motion_mode = 0) followed by
 * islam_imu_preint(motion_mode = 1); same scratch size. */
int islam_imu_preint_both(const void* dt, const void* gyro, const void* acc, const int64_t* seg, int nframes, int64_t S,
                          int max_frame_samples, const void* init_pos, const void* init_rot, const void* init_vel, double gravity,
                          void* world_pos, void* world_rot, void* world_vel, void* motion_pos, void* motion_rot, void* motion_vel,
                          void* scratch, int dtype, void* stream);

/* Backward of islam_imu_preint w.r.t. the gyro and accelerometer samples: what PyPose's autograd returns through
 * pp.module.IMUPreintegrator when the denoiser runs with grad enabled (imu_integrator.py:107-113,146-153 with eval=False;
 * the IMU-target epoch of train.py:177-179,207-212 -- SURVEY F6).  fwd_scratch: the scratch buffer of the forward call on the
 * same inputs (holds incre_r, the frame-start rotations and the per-frame sums).  g_pos (rows,3), g_rot (rows,4), g_vel (rows,3):
 * gradients of the forward's outputs (rows as in the forward: nframes in motion mode, nframes+1 in world mode), any may be NULL
 * (= zero); g_rot is in PyPose's convention: a left-perturbation tangent vector in slots 0..2, slot 3 ignored.
 * g_gyro, g_acc: (S,3), every row of a non-empty frame is written (rows of samples outside all frames are left untouched:
 * zero-initialise).  scratch: islam_imu_preint_bwd_scratch_bytes(nframes) bytes.  Arithmetic in float64 for either dtype. */
size_t islam_imu_preint_bwd_scratch_bytes(int nframes);
int islam_imu_preint_bwd(const void* dt, const void* gyro, const void* acc, const int64_t* seg, int nframes, int64_t S,
                         double gravity, int motion_mode, const void* fwd_scratch, const void* g_pos, const void* g_rot,
                         const void* g_vel, void* g_gyro, void* g_acc, void* scratch, int dtype, void* stream);

/* Covariance of the pre-integration: what pp.module.IMUPreintegrator(prop_cov=True) propagates beside the increments (PyPose is external:
 * the definition below is the contract, its match to PyPose is unpinned).  Error state [dphi, dv, dp] (Forster's ordering): dphi is the
 * right perturbation of the pre-integrated rotation DR, dv and dp are expressed in the body frame at the start of the pre-integration.
 * For sample j with d = dt_j, w = gyro_j, a = acc_j (as handed to the integrator, gravity NOT removed), DR_j the rotation accumulated in
 * front of it and dr = Exp(w d):
 *   A_j = [ dr^T 0 0 ; -DR_j [a]x d  I  0 ; -DR_j [a]x d^2/2  I d  I ],  Bg_j = [ Jr(w d) d ; 0 ; 0 ],  Ba_j = [ 0 ; DR_j d ; DR_j d^2/2 ],
 *   Sigma_{j+1} = A_j Sigma_j A_j^T + Bg_j diag(sg2) Bg_j^T + Ba_j diag(sa2) Ba_j^T.
 * gyro_cov, acc_cov: HOST arrays of three per-sample (discrete) variances; gyro_cov_s / acc_cov_s: optional (S,3) device arrays of the I/O
 * dtype with per-sample variances that replace them (NULL: the constants).  dt, gyro, acc, seg, max_frame_samples: as islam_imu_preint.
 * motion_mode != 0: out_cov has nframes rows, row i = the recurrence over samples [seg[i], seg[i+1]) from Sigma = 0, DR = I (a frame
 * without samples: zero).  motion_mode == 0: nframes + 1 rows, row 0 = init_cov (81 doubles in device memory, its symmetric part is
 * taken; NULL: zero), row k = the recurrence over ALL samples [seg[0], seg[k]) from init_cov with DR accumulated since seg[0] -- the
 * dead-reckoning uncertainty in the body frame of the window's start (a frame without samples repeats the row in front of it).  The
 * result does not depend on the initial rotation, position, velocity or gravity.
 * out_cov: rows x 9 x 9 float64, every row exactly symmetric; the arithmetic is float64 for either dtype.  nframes == 0 is legal.
 * scratch: islam_imu_preint_cov_scratch_bytes(S, nframes) bytes (world mode; motion mode uses none).  Log-depth: the samples of a frame
 * are reduced by one wavefront, the frames by a multi-level scan (csrc/imu_cov.hip); no workgroup waits for another. */
size_t islam_imu_preint_cov_scratch_bytes(int64_t S, int nframes);
int islam_imu_preint_cov(const void* dt, const void* gyro, const void* acc, const int64_t* seg, int nframes, int64_t S,
                         int max_frame_samples, const double gyro_cov[3], const double acc_cov[3], const void* gyro_cov_s,
                         const void* acc_cov_s, const double* init_cov, int motion_mode, double* out_cov, void* scratch, int dtype,
                         void* stream);

/* Bias Jacobians of the pre-integration: J = d[dphi, dv, dp] / d[b_g | b_a], 9x6 by rows, of a FURTHER bias b
 * subtracted from every sample (sample - b), evaluated at b = 0.  The samples are as handed to the integrator (already bias-corrected /
 * denoised).  The dphi rows are the right perturbation of DR (DR(b) = DR Exp(J_phig b) to first order), the dv and dp rows are in the
 * body frame at the start of the pre-integration.  With A_j, Bg_j, Ba_j as defined for islam_imu_preint_cov above:
 *   J_{j+1} = A_j J_j - [ Bg_j | Ba_j ],  J_0 = 0.
 * Gravity plays no part: islam_imu_preint subtracts gravity in a gyro-dependent body frame, and the gyro-bias sensitivity of that term
 * is not part of J (the covariance leaves it out for the same reason).
 * dt, gyro, acc, seg, max_frame_samples, dtype: as islam_imu_preint_cov.
 * motion_mode != 0: nframes rows, row i = the recurrence over samples [seg[i], seg[i+1]) from J = 0, DR = I (a frame without samples:
 * exact zeros).  motion_mode == 0: nframes + 1 rows, row 0 = init_jac (54 doubles in device memory, NULL: zero; its (dphi, b_a) block is
 * ignored and written as zero), row k = the recurrence over ALL samples [seg[0], seg[k]) from init_jac with DR accumulated since seg[0]
 * (a frame without samples repeats the row in front of it bit for bit).  To continue a window [0, m) over [m, n) with a second call,
 * whose elements live in the body frame at sample m: hand it init_jac = diag(I, W^T, W^T) J_m and take diag(I, W, W) times its rows,
 * W = the rotation DR accumulated over [0, m) (the v and p ROWS are rotated, the dphi rows are not).
 * out_jac: rows x 9 x 6 float64, the (dphi, b_a) block exactly 0.0; float64 arithmetic from the up-cast samples for either dtype.
 * nframes == 0 is legal; a second call gives the same bits (fixed association order, no atomics).
 * scratch: islam_imu_preint_bias_jac_scratch_bytes(S, nframes) bytes (world mode; motion mode uses none).  The frame-reduce /
 * multi-level-scan structure is islam_imu_preint_cov's (csrc/imu_bias_jac.hip); no workgroup waits for another. */
size_t islam_imu_preint_bias_jac_scratch_bytes(int64_t S, int nframes);
int islam_imu_preint_bias_jac(const void* dt, const void* gyro, const void* acc, const int64_t* seg, int nframes, int64_t S,
                              int max_frame_samples, const double* init_jac, int motion_mode, double* out_jac, void* scratch, int dtype,
                              void* stream);

/* First-order correction of pre-integrated increments for a bias change (dbg, dba: HOST arrays of three; the samples lose a further
 * bias): per row, with the row's J of islam_imu_preint_bias_jac,
 *   DR' = DR Exp(J_phig dbg) (quaternion xyzw, renormalised),  dv' = dv + J_vg dbg + J_va dba,  dp' = dp + J_pg dbg + J_pa dba.
 * jac (rows, 9, 6) float64; rot (rows, 4), vel, pos (rows, 3) and the outputs in the I/O dtype (float64 arithmetic); the outputs may
 * alias the inputs.  The increments must be in the START-BODY frame of their row.  islam_imu_preint(motion_mode = 1) returns, for
 * frame i, rot = DR_i as is, but vel = R0_i dv_i and pos = R0_i dp_i, where R0_i = init_rot DR_0 ... DR_{i-1} is the rotation at the
 * start of frame i (row i of the world-mode rotations of the same stream): only frame 0 of a call with the identity init_rot is in its
 * start-body frame already.  The caller rotates vel and pos by R0_i^T before this call and by R0_i after it (rot passes unchanged).
 * With gravity != 0 those rows also hold the integrated gravity term, which the correction leaves as it is (see above). */
int islam_imu_bias_correct(const double* jac, const void* rot, const void* vel, const void* pos, int rows, const double dbg[3],
                           const double dba[3], void* out_rot, void* out_vel, void* out_pos, int dtype, void* stream);

/* Closed-form gyro-bias step from rotation residuals: dbg = argmin sum_i w_i | Log(DR_i^T DRref_i) - J_phig,i dbg |^2 over the rows,
 * H = sum_i w_i J_phig,i^T J_phig,i.  rot_imu: the pre-integrated relative rotations (rows, 4) xyzw in the I/O dtype, rot_ref: the
 * relative rotations the caller trusts (VO, PVGO-optimised), jac (rows, 9, 6) float64 of the same rows, weight (rows) float64 device
 * memory or NULL = all ones.  out_dbg: 3 doubles, out_H: 9 doubles or NULL (device memory).  The gyro bias to subtract from the samples
 * becomes bias + dbg.  A row whose weight is zero takes no part, exactly as if it were not there (the rows that count are compacted in
 * row order and summed in a fixed order, no atomics: a second call gives the same bits).  A row of non-zero weight whose residual or
 * weight is not finite is excluded and counted.
 * Returns the number of excluded rows (>= 0), or ISLAM_ENOTPD when H is singular (a Cholesky pivot <= 1e-13 of its diagonal entry;
 * out_dbg is then zero, out_H is still written), or ISLAM_EARG.  The call synchronises the stream (one 8-byte read-back).
 * scratch: islam_imu_gyro_bias_solve_scratch_bytes(rows) bytes. */
size_t islam_imu_gyro_bias_solve_scratch_bytes(int rows);
int islam_imu_gyro_bias_solve(const double* jac, const void* rot_imu, const void* rot_ref, const double* weight, int rows,
                              double* out_dbg, double* out_H, void* scratch, int dtype, void* stream);

/* Gravity, accelerometer bias and velocities from pre-integrated increments and trusted poses, in closed form (DESIGN.md section 3.13;
 * the linear visual-inertial alignment of ORB-SLAM-VI / VINS-Mono).  n = rows intervals i = 0 .. n-1 between n + 1 poses.  Given
 *   R_i, p_i   world rotation (xyzw) and position of the IMU BODY at pose i = 0 .. n (VO or PVGO; the caller applies rgb2imu),
 *   d_i        the duration of interval i,
 *   dv_i, dp_i the gravity-free pre-integrated increments of interval i in the body frame at its start (islam_imu_preint motion rows
 *              with gravity 0, rotated by R0_i^T as described for islam_imu_bias_correct),
 *   Jv_i = J_va,i, Jp_i = J_pa,i   the 3x3 blocks (rows 3:6 and 6:9, columns 3:6) of the row's islam_imu_preint_bias_jac Jacobian,
 * the unknowns are the gravity g (the world acceleration: v' = R a + g), a further accelerometer bias b (sample - b) and the world
 * velocities v_0 .. v_n:
 *   p_{i+1} = p_i + v_i d_i + g d_i^2 / 2 + R_i (dp_i + Jp_i b)        (P_i)
 *   v_{i+1} = v_i + g d_i + R_i (dv_i + Jv_i b)                        (V_i)
 * (P_i) defines v_i for i < n; put into (V_i) it leaves, for every pair of consecutive intervals i = 0 .. n-2, three equations in
 * x = [g; b] alone:
 *   A_i x = r_i,   A_i = [ -(d_i + d_{i+1}) / 2 I  |  R_i Jp_i / d_i - R_{i+1} Jp_{i+1} / d_{i+1} - R_i Jv_i ],
 *   r_i = (p_{i+1} - p_i) / d_i - (p_{i+2} - p_{i+1}) / d_{i+1} + R_{i+1} dp_{i+1} / d_{i+1} - R_i dp_i / d_i + R_i dv_i.
 * x = argmin sum_i w_i | L_i^-1 (A_i x - r_i) |^2,  H = sum_i w_i A_i^T C_i^-1 A_i (6x6),  c = sum_i w_i A_i^T C_i^-1 r_i.
 * weight: (rows - 1) float64 per pair, NULL = all ones.  cov: the (rows, 9, 9) islam_imu_preint_cov motion rows S_i (error state
 * [phi, v, p], subscripts name its 3x3 blocks) or NULL; with them C_i = L_i L_i^T is the pair's covariance
 *   C_i = R_{i+1} S_{i+1}^pp R_{i+1}^T / d_{i+1}^2 + R_i ( S_i^pp / d_i^2 - (S_i^pv + S_i^vp) / d_i + S_i^vv ) R_i^T,
 * without them C_i = I.  Neighbouring pairs share interval i + 1; their correlation is neglected.  jac NULL: b is not estimated, the
 * system is 3x3 in g and the b outputs are exact zeros.  The velocities follow by back-substitution: v_i, i < n, from (P_i), v_n from
 * (V_{n-1}); a pose whose own interval has d <= 0 takes (P), (V) of the interval in front of it, and NaN if that has d <= 0 as well.
 * gravity_norm = G > 0: gravity of known magnitude, on the same quadratic form x^T H x - 2 x^T c with no second pass over the data:
 * gh = g / |g| of the free solve; four times: b1 = normalise(e - (e . gh) gh) with e the coordinate axis of the smallest |gh . e|
 * (lowest index on a tie), b2 = gh x b1, the 5x5 (2x2 without jac) projection of (H, c) onto g = G gh + [b1 b2] u solved for (u, b),
 * gh <- normalise(G gh + [b1 b2] u); the outputs are g = G gh and the b of the last round.  gravity_norm = 0: the free solve.
 * A pair takes part if its weight is finite and non-zero, its A_i, r_i are finite, its d are > 0 and, with cov, C_i factorises (a
 * Cholesky pivot <= 1e-13 of its diagonal entry fails, as in islam_imu_gyro_bias_solve).  A pair of weight zero takes no part,
 * whatever its data holds, and is not counted; any other pair that does not take part is excluded and counted.
 * rot_ref (rows + 1, 4), pos_ref (rows + 1, 3), dts (rows), dvel, dpos (rows, 3) in the I/O dtype; jac (rows, 9, 6), cov, weight
 * float64; float64 arithmetic for either dtype.  out_x: 6 doubles [g, b]; out_H: 36 doubles or NULL; out_vel: (rows + 1, 3) doubles
 * or NULL (all device memory).  Returns the number of excluded pairs (>= 0), or ISLAM_ENOTPD when H (or its 3x3 / 5x5 / 2x2 form)
 * fails the pivot rule or no pair takes part (rows <= 1 included): out_x and out_vel are then zeros, out_H is still written; or
 * ISLAM_EARG.  The sum runs in an order that depends on rows alone, without atomics: a second call gives the same bits, and a pair of
 * weight zero gives the bits of the same call with other data behind that weight.  The call synchronises the stream (one 8-byte
 * read-back).  scratch: islam_imu_gravity_bias_solve_scratch_bytes(rows) bytes. */
size_t islam_imu_gravity_bias_solve_scratch_bytes(int rows);
int islam_imu_gravity_bias_solve(const void* rot_ref, const void* pos_ref, const void* dts, const void* dvel, const void* dpos,
                                 const double* jac, const double* cov, const double* weight, int rows, double gravity_norm, double* out_x,
                                 double* out_H, double* out_vel, void* scratch, int dtype, void* stream);

/* Lever arm and metric scale in the closed-form alignment (the visual-inertial alignment of VINS-Mono,
 * LinearAlignment in its initial_aligment.cpp, which solves the scale and takes the lever arm as known).  The reference has no
 * counterpart: it reads rgb2imu_pose (T_IL) from the dataset.  It is islam_imu_gravity_bias_solve for a caller who has CAMERA
 * positions and not yet the translation of the mount, or positions up to a scale.  The mount is body <- camera, T_IL = (R_x, t); with
 *   Rc_i, q_i  world rotation and position of the CAMERA at pose i = 0 .. n (VO; q_i possibly up to the scale s),
 * the body poses are R_i = Rc_i R_x^T and p_i = s q_i - R_i t.  Put into (P_i), (V_i) above, with the velocities v_i of the BODY
 * eliminated in the same way, every pair of consecutive intervals i = 0 .. n-2 leaves three equations in x = [g(3); b(3); t(3); s]:
 *   A_i [g; b] + T_i t - s Q_i = m_i,   A_i as above,
 *   T_i = (R_{i+1} - R_i) / d_i - (R_{i+2} - R_{i+1}) / d_{i+1},
 *   Q_i = (q_{i+1} - q_i) / d_i - (q_{i+2} - q_{i+1}) / d_{i+1},
 *   m_i = R_{i+1} dp_{i+1} / d_{i+1} - R_i dp_i / d_i + R_i dv_i.
 * solve_lever, solve_scale (0 or 1 each, not both 0: that case is islam_imu_gravity_bias_solve on body positions) say which of t and
 * s are unknowns.  t not solved: t = 0, the columns T_i are exact zeros.  s not solved: s = 1, the column -Q_i is exact zeros and Q_i
 * joins the right-hand side.  jac NULL: b = 0 as above.  The unknowns that are solved (3 to 10, in the order g, b, t, s) minimise
 * sum_i w_i | L_i^-1 (Y_i [x; -1]) |^2 with Y_i = [A_i | T_i | -Q_i | rhs_i]; weight, cov, C_i = L_i L_i^T, the pivot rule, the pairs
 * that take part and their count are exactly islam_imu_gravity_bias_solve's.  The normal matrix (up to 10x10) is solved by Cholesky
 * under the same pivot rule.  gravity_norm = G > 0: the same four rounds on the same (H, c), with b1, b2 as above and the (n-1) x (n-1)
 * projection onto g = G gh + [b1 b2] u solved for u and every other unknown.  The velocities of the body follow by back-substitution,
 *   v_i = ( s (q_{k+1} - q_k) - (R_{k+1} - R_k) t - g d_k^2 / 2 - R_k (dp_k + Jp_k b) ) / d_k,   k = i,
 * and for a pose whose own interval is missing or has d <= 0: k = i - 1, plus g d_k + R_k (dv_k + Jv_k b); NaN if that has d <= 0 too.
 * rot_body (rows + 1, 4) xyzw: the world rotation of the BODY, R_i = Rc_i R_x^T (the caller conjugates, R_x e.g. from
 * islam_imu_extrinsic_rot_solve); pos_cam (rows + 1, 3): q_i; dts, dvel, dpos, jac, cov, weight as for islam_imu_gravity_bias_solve.
 * Without rotation between the poses T_i = 0 and t is unobservable (ISLAM_ENOTPD); without acceleration s is.
 * out_x: 10 doubles [g, b, t, s]; unknowns that are not solved are exactly 0.0 (b, t) and exactly 1.0 (s).  out_H: 100 doubles or NULL,
 * the 10x10 normal matrix, symmetric, exact zeros in the rows and columns of unknowns that are not solved.  out_vel: (rows + 1, 3)
 * doubles or NULL (all device memory).  Returns the number of excluded pairs (>= 0), or ISLAM_ENOTPD when the normal matrix (or its
 * projection) fails the pivot rule or no pair takes part (rows <= 1 included): all ten of out_x and out_vel are then zeros, out_H is
 * still written; or ISLAM_EARG, before any device work: the argument errors of islam_imu_gravity_bias_solve, solve_lever or
 * solve_scale not 0 or 1, both 0.  Same bits on a second call and behind a weight of zero, as above.  The call synchronises the stream
 * (one 8-byte read-back).  scratch: islam_imu_lever_scale_solve_scratch_bytes(rows) bytes (528 B per pair). */
size_t islam_imu_lever_scale_solve_scratch_bytes(int rows);
int islam_imu_lever_scale_solve(const void* rot_body, const void* pos_cam, const void* dts, const void* dvel, const void* dpos,
                                const double* jac, const double* cov, const double* weight, int rows, int solve_lever, int solve_scale,
                                double gravity_norm, double* out_x /*10*/, double* out_H /*100, optional*/,
                                double* out_vel /*(rows + 1) * 3, optional*/, void* scratch, int dtype, void* stream);

/* Camera-IMU extrinsic rotation from pairs of relative rotations, in closed form (the rotation calibration of
 * VINS-Mono, CalibrationExRotation in its initial_ex_rotation.cpp).  The reference has no counterpart: it reads rgb2imu_pose (T_IL) from
 * the dataset, and every other solve of this header assumes it.  For pair i = 0 .. rows-1
 *   qb_i   the IMU's relative rotation over frame i (DR_i, the rotation of islam_imu_preint's motion rows), xyzw,
 *   qc_i   the camera's relative rotation over the same frame (VO), xyzw.
 * A rigid mount q (the rotation of T_IL: body motion = T_IL camera motion T_IL^-1) satisfies qb_i (x) q = q (x) qc_i, that is
 * M_i q = 0 with M_i = L(qb_i) - R(qc_i), where L(a) p = a (x) p and R(a) p = p (x) a are the 4x4 matrices of the quaternion product.
 * Before use every input quaternion is normalised and negated if its w < 0: conjugate rotations have the same angle, so the two sides
 * of a pair then have equal w, and a sign flip of an input does not change M_i.  A quaternion of zero or non-finite norm makes its
 * pair invalid.
 *   A = sum_i w_i rho_i M_i^T M_i   (4x4, symmetric, positive semi-definite)
 *   q = the unit eigenvector of the smallest eigenvalue of A, with w >= 0
 * out_eig holds the eigenvalues of A ascending, l0 <= l1 <= l2 <= l3; they are the observability diagnosis: when all rotations share
 * one axis the null space is two-dimensional and l1 ~ l0 (a scale-free test is (l1 - l0) / l3).  A degenerate but non-empty problem
 * is not an error: the caller reads the eigenvalues.
 * rho_i is a Huber weight on the angular residual: 1 in round 0; with delta > 0 and rounds = K >= 1 the solve is repeated K more
 * times with rho_i = min(1, delta / theta_i), theta_i = angle(qb_i^-1 (x) q^ (x) qc_i (x) q^^-1) under the previous round's q^, the
 * angle taken as 2 atan2(|vec|, |w|).  delta = 0: one round, rounds is ignored.
 * weight: (rows) float64 or NULL = all ones.  A pair of weight exactly zero takes no part, whatever its data holds, and is not counted;
 * a pair with a negative or non-finite weight or an invalid quaternion is excluded and counted.
 * rot_imu, rot_cam (rows, 4) in the I/O dtype; float64 arithmetic for either dtype.  out_q: 4 doubles; out_eig: 4 doubles; out_res:
 * rows doubles or NULL: theta_i under the final q, NaN for an invalid quaternion, computed for pairs of weight zero too (all device
 * memory).  Returns the number of excluded pairs (>= 0); ISLAM_ENOTPD when no pair takes part (rows = 0 included): out_q, out_eig and
 * out_res are then zeros; ISLAM_EARG, before any device work, for a NULL out_q / out_eig / scratch, NULL rot_imu / rot_cam with
 * rows > 0, rows < 0, a bad dtype, a negative or non-finite delta, rounds < 0.  The sums run in an order that depends on rows alone,
 * without atomics: a second call gives the same bits, and a pair of weight zero gives the bits of the same call with other data behind
 * that weight.  Cost: (K + 1) x (2 or 3) launches plus one for out_res.  The call synchronises the stream (one 8-byte read-back).
 * scratch: islam_imu_extrinsic_rot_solve_scratch_bytes(rows) bytes. */
size_t islam_imu_extrinsic_rot_solve_scratch_bytes(int rows);
int islam_imu_extrinsic_rot_solve(const void* rot_imu, const void* rot_cam, const double* weight, int rows, double delta, int rounds,
                                  double* out_q, double* out_eig, double* out_res, void* scratch, int dtype, void* stream);

/* Camera-IMU time offset and gyro bias from relative rotations, in closed form (the rotation-only temporal
 * calibration that Kalibr uses as its initial guess, the td state of VINS-Mono restricted to rotations).  The reference has no
 * counterpart: it trusts the dataset's synchronisation (rgb2imu_sync), and so does every other solve of this header.  Conventions are
 * islam_imu_gyro_bias_solve's.  Row i is a frame:
 *   DR_i     rot_imu, the pre-integrated relative rotation over the samples [seg[i], seg[i+1]), that is over IMU time [t_i, t_{i+1}],
 *   DRref_i  rot_ref, the relative rotation of the body the caller trusts (VO or PVGO, conjugated into the body frame) between the two
 *            images STAMPED t_i and t_{i+1}.
 * If an image stamped t was really taken at t + td on the IMU's clock, DRref_i is the body's rotation over [t_i + td, t_{i+1} + td].
 * Let ws_i and we_i be the body angular rates at the two boundaries of row i; under the integrator's own zero-order hold these are the
 * samples that START there, gyro[seg[i]] and gyro[seg[i+1]] (rate_start, rate_end).  Then, for 0 <= td <= the duration of those
 * samples, exactly
 *   DR_i(td) = Exp(-ws_i td) DR_i Exp(we_i td) = DR_i Exp(u_i td + O(td^2)),   u_i = we_i - DR_i^T ws_i,
 * and with DR(b) = DR Exp(J_phig b) of islam_imu_preint_bias_jac that gives three equations per row, linear in x = [dbg(3); td]:
 *   e_i = Log(DR_i^T DRref_i) = J_phig,i dbg + u_i td,
 *   x = argmin sum_i w_i rho_i | e_i - Y_i x |^2,   Y_i = [J_phig,i | u_i] (3x4),   H = sum_i w_i rho_i Y_i^T Y_i (4x4).
 * td is observable only where the angular rate changes: with a constant rate about a fixed axis u_i = 0 and the pivot of td fails.
 * solve_bias = 0: td alone is solved, dbg is exactly 0.0, the bias rows and columns of out_H are exact zeros and jac is not read (it
 * may be NULL).  The unknowns that are solved (4 or 1) are compacted and solved by Cholesky under islam_imu_gyro_bias_solve's pivot
 * rule (a pivot <= 1e-13 of its diagonal entry fails; for the 1x1 case a pivot <= 0 fails).
 * rho_i is a Huber weight on the residual: 1 in round 0; with delta > 0 and rounds = K >= 1 the solve is repeated K more times with
 * rho_i = min(1, delta / |e_i - Y_i x^|) under the previous round's x^.  delta = 0: one round, rounds is ignored.
 * weight: (rows) float64 or NULL = all ones.  A row counts with a finite non-zero weight and finite e_i, u_i, J_phig,i.  A row of weight
 * exactly zero takes no part, whatever its data holds, and is not counted; a row with a negative or non-finite weight, or non-finite
 * data behind a non-zero weight, is excluded and counted.
 * jac (rows, 9, 6) float64; rot_imu, rot_ref (rows, 4) xyzw, rate_start, rate_end (rows, 3) in the I/O dtype; float64 arithmetic for
 * either dtype.  out_x: 4 doubles [dbg, td]; out_H: 16 doubles or NULL, symmetric; out_res: rows doubles or NULL: | e_i - Y_i x | under
 * the final x, NaN for a row with non-finite data, computed for rows of weight zero too (all device memory).  The gyro bias to subtract
 * from the samples becomes bias + dbg; td is added to the camera's stamps.
 * Returns the number of excluded rows (>= 0); ISLAM_ENOTPD on a pivot failure in any round or when no row takes part (rows = 0
 * included): out_x and out_res are then zeros, out_H is still written; ISLAM_EARG, before any device work, for a NULL rot_imu / rot_ref
 * / rate_start / rate_end with rows > 0, a NULL out_x or scratch, a NULL jac with solve_bias = 1 (and rows > 0), rows < 0, a bad dtype,
 * solve_bias not 0 or 1, a negative or non-finite delta, rounds < 0.  The sums run in an order that depends on rows alone, without
 * atomics: a second call gives the same bits, and a row of weight zero gives the bits of the same call with other data behind that
 * weight.  Cost: (K + 1) x (2 or 3) launches plus one for out_res.  The call synchronises the stream (one 8-byte read-back).
 * scratch: islam_imu_time_offset_solve_scratch_bytes(rows) bytes (120 B per row). */
size_t islam_imu_time_offset_solve_scratch_bytes(int rows);
int islam_imu_time_offset_solve(const double* jac /*(rows,9,6) or NULL iff solve_bias==0*/, const void* rot_imu, const void* rot_ref,
                                const void* rate_start, const void* rate_end /*(rows,3), I/O dtype*/, const double* weight /*rows or NULL*/,
                                int rows, int solve_bias, double delta, int rounds, double* out_x /*4: dbg, td*/,
                                double* out_H /*16 or NULL*/, double* out_res /*rows or NULL*/, void* scratch, int dtype, void* stream);

/* The pre-integrated rotations of a window moved by tau, without re-integrating: out_rot_i = Exp(-ws_i tau) (x) rot_i (x) Exp(we_i tau),
 * renormalised (exact under the zero-order hold for 0 <= tau <= the duration of the two boundary samples).  It is to the time offset
 * what islam_imu_bias_correct is to the bias: a Gauss-Newton round of islam_imu_time_offset_solve starts from a sub-sample offset.
 * rot (rows, 4) xyzw, rate_start, rate_end (rows, 3), out_rot (rows, 4) in the I/O dtype (float64 arithmetic); out_rot may alias rot;
 * tau: a host double.  ISLAM_EARG for rows < 0, a bad dtype, a non-finite tau, a NULL pointer with rows > 0.  Does not synchronise. */
int islam_imu_time_shift(const void* rot, const void* rate_start, const void* rate_end, int rows, double tau, void* out_rot, int dtype,
                         void* stream);

/* ---------------------------------------------------------------- PVGO (pose-velocity graph optimisation) */

typedef struct {
    double w[4];          /* information scalars: lw0^2 (VO), lw1^2 (dvel), lw2^2 (IMU rot), lw3^2 (transvel); pvgo.py:125-129 */
    double radius;        /* TrustRegion(radius=..), pvgo.py:170 */
    double vmin, vmax;    /* LM(min=1e-4), max=1e32 default: diagonal clamp */
    double high, low, up, down, factor, rmin, rmax;   /* ppost.TrustRegion defaults 0.5,1e-3,2,0.5,0.5,1e-6,1e16 */
    int reject;           /* LM reject=16 default */
    int max_steps;        /* StopOnPlateau(steps=10) */
    int patience;         /* StopOnPlateau(patience=3) */
    double decreasing;    /* StopOnPlateau(decreasing=1e-3) */
    int seg_len[2];       /* partitioned block-Cholesky: interior nodes per segment at level 0 / 1 (0 = auto) */
} islam_pvgo_params;

typedef struct {
    int steps;            /* optimizer.step() calls made */
    int trials;           /* damped solves (inner while-loop iterations) over all steps */
    int status;           /* ISLAM_OK or ISLAM_ENOTPD (step broken like PyPose) */
    double loss;          /* final unweighted loss */
    double damping;       /* final damping */
} islam_pvgo_result;

#define ISLAM_PVGO_MAX_LEVELS 6   /* levels of the partitioned block Cholesky; plan arrays hold 3*ISLAM_PVGO_MAX_LEVELS ints */

void islam_pvgo_default_params(islam_pvgo_params* p);
size_t islam_pvgo_workspace_bytes(int N);

/* Whole LM loop on a canonical chain graph (links[k] = [k, k+1], E = N-1), float64.
 * Replaces pvgo.py:168-180: PoseVelGraph + pp.optim.LM(Cholesky, TrustRegion) + StopOnPlateau.
 * nodes (N,7), vels (N,3): in = initial values, out = optimised (NOT yet aligned, see islam_pvgo_align);
 * poses (N-1,7) VO motions; drots (N-1,4), dtrans (N-1,3), dvels (N-1,3), dts (N-1).
 * trace: optional HOST buffer of 3*trace_cap doubles receiving (loss, damping, accepted) per trial. */
int islam_pvgo_run_chain(double* nodes, double* vels, const double* poses, const double* drots,
                         const double* dtrans, const double* dvels, const double* dts, int N,
                         const islam_pvgo_params* prm, void* workspace, size_t workspace_bytes,
                         islam_pvgo_result* result, double* trace, int trace_cap, void* stream);

/* Sparse reprojection factor, the optional 5th residual of the graph (pvgo.py:53-61,130-143,163-165 with
 * dense_ba.py:276-305 SparseReprojectionLoss and pypose reprojerr/point2pixel):
 *   err[k][j] = pixel(K, T_k^-1 * points[k][j]) - targets[k][j],  T_k = rgb2imu^-1 (X_k^-1 X_{k+1}) rgb2imu,
 * weight (loss_weight[4]/K)^2 per row.  Link k couples only nodes k, k+1, so the system stays block-tridiagonal. */
typedef struct {
    const double* points;     /* (N-1, K, 3) device: SparseReprojectionLoss.point3d (camera frame of node k) */
    const double* targets;    /* (N-1, K, 2) device: SparseReprojectionLoss.target (pixels in frame k+1) */
    int K;                    /* SparseReprojectionLoss.N keypoints per link */
    double fx, fy, cx, cy;    /* SparseReprojectionLoss.K */
    double rgb2imu[7];        /* camera->IMU pose [t, q xyzw] */
    double weight;            /* (loss_weight[4]/K)^2, pvgo.py:131 */
    int compat_first_motion;  /* 1: replicate pvgo.py:57 `motion[0] = 0.1` (link 0 becomes a constant residual) */
} islam_pvgo_reproj;

#define ISLAM_REPROJ_REC 32   /* doubles per link written by islam_pvgo_reproj_reduce */

/* islam_pvgo_run_chain with the reprojection factor (reproj == NULL: identical to islam_pvgo_run_chain). */
int islam_pvgo_run_chain_reproj(double* nodes, double* vels, const double* poses, const double* drots,
                                const double* dtrans, const double* dvels, const double* dts, int N,
                                const islam_pvgo_params* prm, const islam_pvgo_reproj* reproj, void* workspace,
                                size_t workspace_bytes, islam_pvgo_result* result, double* trace, int trace_cap,
                                void* stream);
/* Robust kernels on the chain LM: what PyPose's pp.optim.LM(kernel=...) with pp.optim.kernel.Huber / Cauchy and its
 * FastTriggs corrector stand for.  The factor groups are the four model outputs, in the order of w[]: 0 VO (6 rows per link),
 * 1 velocity, 2 IMU rotation, 3 translation-velocity (3 rows each).  For a factor with residual r, s = |r|^2 (unweighted):
 *   loss (accept test, TrustRegion, StopOnPlateau) = sum rho(s);  its rows of J^T W J, J^T W r and of the trust-region term
 *   are scaled by c = rho'(s) at the linearisation point (= r and J scaled by sqrt(c)).
 *   ISLAM_ROBUST_NONE:   rho = s
 *   ISLAM_ROBUST_HUBER:  rho = s (s <= d^2), 2 d sqrt(s) - d^2 otherwise
 *   ISLAM_ROBUST_CAUCHY: rho = d^2 log(1 + s / d^2)
 * Damping, diagonal clamp, reject limit and StopOnPlateau are unchanged. */
#define ISLAM_ROBUST_NONE 0
#define ISLAM_ROBUST_HUBER 1
#define ISLAM_ROBUST_CAUCHY 2
typedef struct {
    int kind[4];          /* ISLAM_ROBUST_* per factor group */
    double delta[4];      /* kernel scale d > 0 (ignored for ISLAM_ROBUST_NONE) */
} islam_pvgo_robust;

/* islam_pvgo_run_chain under robust kernels (robust == NULL or all ISLAM_ROBUST_NONE: identical to islam_pvgo_run_chain).
 * Runs the launch-per-stage loop (like the reprojection factor).  ISLAM_EARG for an unknown kind or d <= 0. */
int islam_pvgo_run_chain_robust(double* nodes, double* vels, const double* poses, const double* drots,
                                const double* dtrans, const double* dvels, const double* dts, int N,
                                const islam_pvgo_params* prm, const islam_pvgo_robust* robust, void* workspace,
                                size_t workspace_bytes, islam_pvgo_result* result, double* trace, int trace_cap,
                                void* stream);
/* Per-factor information matrices.  The reference hands PyPose one information matrix per factor
 * (pvgo.py:133-162 stacks (E,6,6) and (M,3,3) tensors, :178 passes them as weight=) and only ever fills them with loss_weight^2 I;
 * here every factor k carries its own symmetric positive SEMI-definite Omega_k:
 *   A = sum_k J_k^T Omega_k J_k,  b = -sum_k J_k^T Omega_k r_k  (the Jacobians of islam_pvgo_run_chain, unchanged).
 * Everything else of the LM is unchanged: the diagonal clamp [vmin, vmax], cumulative damping, the reject limit, TrustRegion,
 * StopOnPlateau, and the accept-test loss and trust-region term, which stay UNWEIGHTED as they are under scalar weights.
 * Omega_k = w[g] I for every factor is islam_pvgo_run_chain; Omega_k = 0 removes factor k from the step.
 * Device layout, component-major like `lin` (entry c of factor k at [c * count + k]), M = N - 1:
 *   info_vo (21, M): the upper triangle of the 6x6 of VO factor k, rows ordered [rho, phi], row-major order of the triangle;
 *   info_imu (18, M): the 6-entry upper triangles [00 01 02 11 12 22] of [velocity | IMU rotation | translation-velocity].
 * prm->w is ignored for the assembly.  info_vo == info_imu == NULL: exactly islam_pvgo_run_chain; exactly one of them NULL:
 * ISLAM_EARG before any device work.  Runs the launch-per-stage loop with one more launch (info_build_kernel) per linearisation. */
int islam_pvgo_run_chain_info(double* nodes, double* vels, const double* poses, const double* drots, const double* dtrans,
                              const double* dvels, const double* dts, int N, const islam_pvgo_params* prm,
                              const double* info_vo, const double* info_imu, void* workspace, size_t workspace_bytes,
                              islam_pvgo_result* result, double* trace, int trace_cap, void* stream);
/* General topology: the multipliers c of every VO edge from vo (24,E) (islam_pvgo_linearize_edges) -> c_vo (E), and of the three
 * IMU-side factors of every link from lin (42,M) -> c_imu (3,M) [velocity | rotation | translation-velocity]; rho_part
 * ((max(E,M)+63)/64) = partial sums of rho over both.  c_vo / c_imu may be NULL (loss only). */
int islam_pvgo_robust_weights(const double* vo, int E, const double* lin, int M, const islam_pvgo_robust* robust,
                              double* c_vo, double* c_imu, double* rho_part, void* stream);

/* Stage-level: per-link reduction over the K keypoints at nodes (dx == NULL) or at Exp(dx)*nodes (dx (N,9)):
 * red (N-1, ISLAM_REPROJ_REC) = [ J^T J upper triangle (21, row-major) | J^T r (6) | r^T r (1) | pad ], J = d err / d eta
 * for the left perturbation T_k <- Exp(eta) T_k (unweighted). */
int islam_pvgo_reproj_reduce(const double* nodes, const double* dx, int N, const islam_pvgo_reproj* reproj,
                             double* red, void* stream);

/* Stage-level entry points (same kernels the loop above launches; exported for parity tests/profiling). */
/* residuals + Jacobian blocks per link -> lin (42 x M, component-major), loss_part (nblocks) */
int islam_pvgo_linearize(const double* nodes, const double* vels, const double* poses, const double* drots,
                         const double* dtrans, const double* dvels, const double* dts, int N,
                         double* lin, double* loss_part, void* stream);
/* block-tridiagonal normal equations: Hd (N,9,9), Ho (N-1,9,9) [rows k, cols k+1], rhs (N,9) = -J^T W r, diag clamped */
int islam_pvgo_build_normal(const double* lin, const double* dts, int N, const double w[4], double vmin, double vmax,
                            double* Hd, double* Ho, double* rhs, void* stream);
/* islam_pvgo_build_normal with robust multipliers per link for groups 1-3: c_imu (3, N-1) [velocity | rotation |
 * translation-velocity] (islam_pvgo_robust_weights) scale w[1], w[2], w[3] of link k. */
int islam_pvgo_build_normal_scaled(const double* lin, const double* dts, int N, const double w[4], const double* c_imu,
                                   double vmin, double vmax, double* Hd, double* Ho, double* rhs, void* stream);
/* islam_pvgo_build_normal with one information matrix per factor (semantics and layout: islam_pvgo_run_chain_info; pvgo.py:133-162,178):
 * info_vo (21, N-1) or NULL (no VO group, like w[0] = 0), info_imu (18, N-1).  Per link k with A_k = [[G, C],[0, G]]: the pose block
 * S = A_k^T O0 A_k + O3 on rho-rho + B^T O2 B on phi-phi enters Hd of both nodes and -S the coupling; O1 + dt^2 O3 (node k) and O1
 * (node k+1) the velocity blocks; dt O3 the rho-v block of node k; -dt O3 and -O1 the v-rho and v-v blocks of the coupling. */
int islam_pvgo_build_normal_info(const double* lin, const double* dts, int N, const double* info_vo, const double* info_imu,
                                 double vmin, double vmax, double* Hd, double* Ho, double* rhs, void* stream);
/* The IMU factors of a link as ONE correlated factor: a symmetric positive semi-definite 9x9 Omega_k on the
 * stacked residual r9 = [rv; er; rt] (velocity, IMU rotation, translation-velocity: the order of w[1..3]).  Device layout
 * info_imu9 (45, N-1): the upper triangle of each 9x9 in row-major order of the triangle, component-major like `lin`.  With the
 * unchanged Jacobians J_i, J_j of link k = (i, j): Hd[i] += J_i^T O J_i, Hd[j] += J_j^T O J_j, Ho[k] += J_i^T O J_j, rhs = -J^T O r9;
 * the VO group (info_vo (21, N-1) or NULL), the clamp and every other rule are those of islam_pvgo_build_normal_info /
 * islam_pvgo_run_chain_info, whose arguments these two take.  Omega_k = blockdiag(O1, O2, O3) is exactly the (18, N-1) form. */
int islam_pvgo_build_normal_info9(const double* lin, const double* dts, int N, const double* info_vo, const double* info_imu9,
                                  double vmin, double vmax, double* Hd, double* Ho, double* rhs, void* stream);
int islam_pvgo_run_chain_info9(double* nodes, double* vels, const double* poses, const double* drots, const double* dtrans,
                               const double* dvels, const double* dts, int N, const islam_pvgo_params* prm,
                               const double* info_vo, const double* info_imu9, void* workspace, size_t workspace_bytes,
                               islam_pvgo_result* result, double* trace, int trace_cap, void* stream);
/* Hd.diag += Hd.diag*damping (in place, cumulative), then solve -> dx (N,9).  status (device int[4]). */
int islam_pvgo_solve_chain(double* Hd, const double* Ho, const double* rhs, double damping, int N,
                           const int seg_len[2], void* workspace, size_t workspace_bytes, double* dx, void* stream);
/* Stream-ordered variant for iterative methods (islam_amd/pvgo_dense.py: preconditioner of the loop-closure solver): enqueue
 * only -- no read-back, no synchronisation.  islam_pvgo_solve_status synchronises the stream, returns ISLAM_ENOTPD if any solve
 * enqueued on this workspace since the previous status call met a non-positive pivot, and re-initialises the workspace's
 * status / hand-off words; call it once before the first enqueue on a fresh workspace. */
int islam_pvgo_solve_chain_enqueue(double* Hd, const double* Ho, const double* rhs, double damping, int N,
                                   const int seg_len[2], void* workspace, size_t workspace_bytes, double* dx, void* stream);
int islam_pvgo_solve_status(int N, void* workspace, size_t workspace_bytes, void* stream);
/* Profiling variant: HIP events around every launch of one solve (on `stream`).  ms[i] = duration of launch i
 * (eliminate level 0..L-1, then back-substitution L-2..0; at most 2*ISLAM_PVGO_MAX_LEVELS-1 entries),
 * plan[3*l..] = (nodes, segment length, segments) for l < ISLAM_PVGO_MAX_LEVELS, plan[3*ISLAM_PVGO_MAX_LEVELS] = first
 * level solved inside the single-workgroup top kernel (3*ISLAM_PVGO_MAX_LEVELS+1 ints). */
int islam_pvgo_solve_chain_timed(double* Hd, const double* Ho, const double* rhs, double damping, int N,
                                 const int seg_len[2], void* workspace, size_t workspace_bytes, double* dx,
                                 float* ms, int* plan, int* nlaunch, void* stream);
/* Measurement hook: exactly the level-0 up-sweep launch of islam_pvgo_solve_chain (same kernel, grid, arguments) and
 * nothing else -- bench.py times a burst of these for the roofline figure.  Hd's diagonal is damped in place. */
int islam_pvgo_eliminate_level0(double* Hd, const double* Ho, const double* rhs, double damping, int N,
                                const int seg_len[2], void* workspace, size_t workspace_bytes, void* stream);
/* Measurement hook: the LM loop's dominant launch in its steady state -- trial step + loss / trust-region sums of a trial
 * (pvgo.py:26-64, ppost.TrustRegion), the linearisation at the trial point and the level-0 elimination of the next damped solve
 * (pp.optim.LM's J^T W J + Cholesky) in ONE kernel (trial_elim_kernel) -- after one linearisation and one solve of the given
 * problem: `launches` back-to-back launches between one pair of HIP events on `stream`; *us_per_launch = average period.
 * info[0..2] = (level-0 segment length, segments, workgroups).  ISLAM_EARG when the fused loop does not cover this N. */
int islam_pvgo_trial_elim_burst(const double* nodes, const double* vels, const double* poses, const double* drots,
                                const double* dtrans, const double* dvels, const double* dts, int N,
                                const islam_pvgo_params* prm, void* workspace, size_t workspace_bytes, int launches,
                                float* us_per_launch, int* info, void* stream);
/* ---- marginal covariances of a chain (no reference counterpart: new capability).
 * A = J^T W J is the UNDAMPED Gauss-Newton matrix of the graph at a state: islam_pvgo_linearize + islam_pvgo_build_normal with
 * vmin = 0, vmax = +inf (no damping, no diagonal clamp), plus the reprojection factor's node blocks when it is used.  Per node
 * the solver's dx ordering [rho (3), phi (3), v (3)]; the pose part is the left perturbation X <- Exp([rho, phi]) X of the
 * retraction.  The graph has a 6-DoF gauge (a common left perturbation of all poses is in the null space of J); it is fixed
 * by an ANCHOR node a: the 6 pose rows and columns of node a are removed from A, A is inverted, and the anchor's pose rows and
 * columns of Sigma are zero.  anchor = -1: no gauge fix, the matrix must be positive definite on its own.
 * Sd (N,9,9) = diagonal blocks, So (N-1,9,9) = blocks (k,k+1) of (Hd,Ho anchored)^-1 (rows node k, columns node k+1, the
 * layout of Ho); Hd, Ho are not modified.  ISLAM_ENOTPD if the anchored matrix is not positive definite (Sd, So then zero).
 * Partitioned selected inversion on the solver's level tree: one up-sweep and one down-sweep launch per level below the top,
 * one launch for the top level and one to finish (a chain the plan keeps on one level, such as N = 9: one launch in all).  seg_len as for islam_pvgo_solve_chain.
 * Argument errors (N < 1, anchor outside [-1, N), workspace too small) return ISLAM_EARG before any HIP call. */
size_t islam_pvgo_marginals_workspace_bytes(int N);
int islam_pvgo_marginals(const double* Hd, const double* Ho, int N, int anchor, const int seg_len[2],
                         void* workspace, size_t workspace_bytes, double* Sd, double* So, void* stream);
/* Stream-ordered variant: enqueue only, no read-back and no synchronisation; status (device int, may be NULL) receives
 * ISLAM_OK or ISLAM_ENOTPD when the call has run. */
int islam_pvgo_marginals_enqueue(const double* Hd, const double* Ho, int N, int anchor, const int seg_len[2],
                                 void* workspace, size_t workspace_bytes, double* Sd, double* So, int* status, void* stream);
/* The level plan of islam_pvgo_marginals, in the format of islam_pvgo_plan (the last int: the top level); returns the level
 * count.  Launches per call: 2 * levels (up- and down-sweep of every level below the top, the top, the finishing launch);
 * one for a one-level plan. */
int islam_pvgo_marginals_plan(int N, const int seg_len[2], int* plan9);
/* ---- multi-GPU building blocks (islam_amd/dist_pvgo.py; no reference counterpart: the reference is single-GPU).
 * plan9 (3*ISLAM_PVGO_MAX_LEVELS+1 ints) receives (nodes, segment length, segments) per level (unused = 0) and, last,
 * the first level that runs inside the single-workgroup top kernel; returns the level count. */
int islam_pvgo_plan(int N, const int seg_len[2], int* plan9);
/* Sharding with an interface-only exchange: a rank owns a contiguous range of the segments of the
 * exchange level xl -- the highest level below the root with at least `world` segments -- and everything below it between the
 * two outer separators of that range.  islam_pvgo_shard_ranges: out[0] = xl, out[1] = P_xl, out[2+2l], out[3+2l] = first
 * segment / number of segments owned at level l (2 + 2*ISLAM_PVGO_MAX_LEVELS ints).  upsweep: levels 0..xl over the rank's own
 * segments; Hd/Ho/rhs are LOCAL level-0 arrays (row 0 = global node `node0`), `exchange` (351*P_xl doubles, array-major like the
 * level-0 products) is zeroed and the rank's rows written: summing it over the ranks is the ONLY data-path collective of a
 * solve (P_xl = 23 at N=5001: 64.6 KB, against 2.34 MB for the level-0 products).  downsweep: the levels above xl from the
 * summed buffer (redundantly), then the local back-substitution; dx is LOCAL like Hd.  Factors live in `workspace`
 * (islam_pvgo_workspace_bytes(N), the same buffer for both calls, ZERO-INITIALISED once by the caller: the product rows of
 * other ranks' segments are read as zero contributions). */
int islam_pvgo_shard_ranges(int N, const int seg_len[2], int world, int rank, int* out);
int islam_pvgo_shard_upsweep(double* Hd, const double* Ho, const double* rhs, double damping, int N, const int seg_len[2], int world,
                             int rank, int node0, void* workspace, size_t workspace_bytes, double* exchange, int* flags,
                             void* stream);
int islam_pvgo_shard_downsweep(const double* exchange, int N, const int seg_len[2], int world, int rank, int node0, void* workspace,
                               size_t workspace_bytes, double* dx, int* flags, void* stream);
/* The whole sharded LM loop in the library, on RCCL (islam_amd/csrc/pvgo_dist.hip): every rank passes the SAME full-size
 * inputs (device, float64: nodes (N,7), vels (N,3) in/out -- the full solution on every rank --, poses (N-1,7), drots (N-1,4),
 * dtrans, dvels (N-1,3), dts (N-1)) and works on its stretch of the chain.  Graphs the fused trial + elimination kernel covers
 * (those islam_pvgo_run_chain fuses, without the reprojection factor): ONE all-reduce per LM trial -- the interface blocks of the
 * next solve (351 doubles per segment of the exchange level) + [sum r^2 | sum JD.(2R+JD) | failed | 18 doubles per cut: the two
 * ranks' parts of the cut node's diagonal] -- with the trial step, the linearisation and the level-0 elimination in one launch
 * under a speculated damping; a rejected or re-damped trial costs one more solve with its own all-reduce (ISLAM_SHARD_FUSED=0:
 * off).  Otherwise per LM trial two all-reduces (the interface blocks;
 * [sum r^2 | sum JD.(2R+JD) | failed | 10-double halo per rank]); accept /
 * reject, TrustRegion and StopOnPlateau replicated on the DEVICE (every rank decides on the same summed scalars), the host
 * runs one trial ahead and reads 128-byte verdicts from pinned memory -- no stream synchronisation inside the loop; the
 * collectives of a cancelled run-ahead trial still execute, identically on every rank.  reproj (may be NULL): the sparse
 * reprojection factor of islam_pvgo_run_chain_reproj over the WHOLE graph; a rank reduces the keypoints of its own links.  comm: an ncclComm_t made
 * with islam_dist_comm_init (rank 0 creates the 128-byte id with islam_dist_unique_id and broadcasts it -- e.g. with
 * torch.distributed) or NULL for world == 1.  workspace: islam_pvgo_workspace_bytes(N); scratch:
 * islam_pvgo_sharded_scratch_bytes(N, world).  exchanged_bytes (may be NULL): bytes handed to the collectives of the trials.
 * The _cb variant takes the all-reduce as a callback (in-place sum of `count` doubles at `buf`, stream-ordered on `stream`;
 * return 0): the tests drive several ranks as threads on one GPU through it. */
typedef int (*islam_allreduce_fn)(void* user, double* buf, size_t count, void* stream);
int islam_dist_unique_id(void* out128);
int islam_dist_comm_init(const void* id128, int world, int rank, void** comm);
int islam_dist_comm_destroy(void* comm);
/* What RCCL itself says about a communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): bench.py prints `ranks` as
 * rccl_ranks_seen so that a multi-GPU record proves the collectives ran over that many ranks.  comm == NULL (world 1): 1, 0, the
 * current device.  Any of the three outputs may be NULL. */
int islam_dist_comm_info(void* comm, int* ranks, int* rank, int* device);
size_t islam_pvgo_sharded_scratch_bytes(int N, int world);
int islam_pvgo_run_chain_sharded(void* comm, int world, int rank, double* nodes, double* vels, const double* poses, const double* drots,
                                 const double* dtrans, const double* dvels, const double* dts, int N, const islam_pvgo_params* prm,
                                 const islam_pvgo_reproj* reproj, void* workspace, size_t workspace_bytes, void* scratch,
                                 size_t scratch_bytes, islam_pvgo_result* res, long long* exchanged_bytes, void* stream);
int islam_pvgo_run_chain_sharded_cb(islam_allreduce_fn fn, void* user, int world, int rank, double* nodes, double* vels,
                                    const double* poses, const double* drots, const double* dtrans, const double* dvels, const double* dts,
                                    int N, const islam_pvgo_params* prm, const islam_pvgo_reproj* reproj, void* workspace,
                                    size_t workspace_bytes, void* scratch, size_t scratch_bytes, islam_pvgo_result* res,
                                    long long* exchanged_bytes, void* stream);
/* Trial step on M links (M+1 node rows): retract on a copy, residuals, partial sums part[2*nblk] =
 * (sum r^2, sum JD.(2R+JD)) per 64-link block (ppost.TrustRegion.update's denominator is -sum). */
int islam_pvgo_trial(const double* nodes, const double* vels, const double* dx, const double* poses, const double* drots,
                     const double* dtrans, const double* dvels, const double* dts, const double* lin, int M,
                     double* nodes_t, double* vels_t, double* part, void* stream);
/* X <- Exp(sign*dx[:, :6]) * X ; v += sign*dx[:, 6:]  (LieTensor.add_) */
int islam_pvgo_retract(const double* nodes, const double* vels, const double* dx, double sign, int N,
                       double* nodes_out, double* vels_out, void* stream);

/* VO factors on ARBITRARY edges (loop closures; pvgo.py:36-39): out (24,E) component-major =
 * e(6) | G(9) | C(9) with d e/d delta_j = [[G,C],[0,G]], d e/d delta_i = -that.  Used by the dense general-topology
 * path (islam_amd/pvgo_dense.py). */
int islam_pvgo_linearize_edges(const double* nodes, const int64_t* edges, const double* poses, int E, double* out,
                               void* stream);
/* General-topology normal equations without ever forming J: A (9N x 9N row-major, fully written) and rhs (9N) from
 *   - the block-tridiagonal IMU part Hd, Ho (N,9,9), rhs_chain (N,9)  (islam_pvgo_build_normal with w[0] = 0, no clamp),
 *   - the VO factors of arbitrary edges `vo` (24,E) from islam_pvgo_linearize_edges, weight w0.
 * node_ptr (N+1), node_adj (2E) = CSR of the edge ends per node, entry = 2*edge + end (end 0 = i, 1 = j), so every
 * diagonal block and right-hand side is summed in a fixed order (bit-reproducible); off-diagonal VO blocks are added
 * with one atomic per entry.  Replaces PyPose's dense J^T W J (pp.optim.LM) on the loop-closure path. */
int islam_pvgo_assemble_dense(const double* Hd, const double* Ho, const double* rhs_chain, const double* vo,
                              const int64_t* edges, const int64_t* node_ptr, const int64_t* node_adj, double w0,
                              int N, int E, double* A, double* rhs, void* stream);
/* islam_pvgo_assemble_dense with a robust multiplier per VO edge: edge e enters with weight w0 * c_vo[e]
 * (c_vo from islam_pvgo_robust_weights). */
int islam_pvgo_assemble_dense_scaled(const double* Hd, const double* Ho, const double* rhs_chain, const double* vo,
                                     const double* c_vo, const int64_t* edges, const int64_t* node_ptr,
                                     const int64_t* node_adj, double w0, int N, int E, double* A, double* rhs, void* stream);
/* islam_pvgo_assemble_dense with one information matrix per VO edge (pvgo.py:133-162,178; layout: islam_pvgo_run_chain_info):
 * info_vo (21,E); edge e adds A_e^T O_e A_e to the diagonal blocks of its two nodes (CSR order, no atomics), -A_e^T O_e A_e to the
 * blocks (i, j) and (j, i) (one atomic per entry), and -+A_e^T O_e e to the right-hand side.  Hd, Ho, rhs_chain: the IMU part from
 * islam_pvgo_build_normal_info with info_vo = NULL. */
int islam_pvgo_assemble_dense_info(const double* Hd, const double* Ho, const double* rhs_chain, const double* vo,
                                   const double* info_vo, const int64_t* edges, const int64_t* node_ptr,
                                   const int64_t* node_adj, int N, int E, double* A, double* rhs, void* stream);
/* The same normal equations in band + off-band form, A = B + R (islam_amd/pvgo_dense.py): B block-tridiagonal
 * in the chain solver's arrays, R the 6x6 blocks of the K edges that couple nodes more than one apart.
 * islam_pvgo_band_assemble works IN PLACE on Hd, Ho (N,9,9) and rhs (N,9), which hold the IMU part (islam_pvgo_build_normal with
 * w[0] = 0, _scaled or _info with info_vo = NULL; no clamp).  Edge e = (i, j), i != j, of `vo` (24,E) adds S_e to the pose blocks of
 * Hd[i] and Hd[j] in the CSR order of node_ptr / node_adj (as islam_pvgo_assemble_dense), -+ its gradient to rhs[i] / rhs[j], and,
 * where |i - j| = 1, -S_e to Ho[min(i, j)] whichever way the edge points; every block is written by one lane, several edges on one
 * node pair accumulate in CSR order, and there are no atomics: the same inputs give the same bits.  S_e = w0 J^T J; with c_vo (E)
 * w0 c_vo[e] J^T J; with info_vo (21,E) J^T Omega_e J (w0 unused); c_vo and info_vo may not both be given.  The edges must be valid
 * (indices in [0, N), no self-loop): the caller checks them on the host.
 * off_idx (K): the indices of the off-band edges, ascending; out: io, jo (K) their ends and So (K,6,6) their S_e.  K = 0: all four NULL.
 * islam_pvgo_band_matvec: y (N,9) = A p in one launch, y = Hd p + Ho p+ + Ho^T p- and, on the pose rows, y_i -= So p_j and
 * y_j -= So p_i for every off-band edge, summed per node over off_ptr (N+1) / off_adj (2K), the CSR of the off-band edge ends per node
 * (entry = 2 * t + end, t the position in io / jo / So): fixed order, no atomics.  Reads the full Hd blocks (both triangles) and
 * Ho[0 .. N-2]; y may not alias p.  Both calls only enqueue on `stream`.  ISLAM_EARG before any HIP call for N < 2, E < 1, K outside
 * [0, E] or a missing array. */
int islam_pvgo_band_assemble(double* Hd, double* Ho, double* rhs, const double* vo, const double* c_vo, const double* info_vo,
                             const int64_t* edges, const int64_t* node_ptr, const int64_t* node_adj, double w0, int N, int E,
                             const int64_t* off_idx, int K, int64_t* io, int64_t* jo, double* So, void* stream);
int islam_pvgo_band_matvec(const double* Hd, const double* Ho, const double* p, const int64_t* off_ptr, const int64_t* off_adj,
                           const int64_t* io, const int64_t* jo, const double* So, int N, int K, double* y, void* stream);
/* Dense fp64 Cholesky A = L L^T of the general-topology normal matrix and the solve with its factor (csrc/dense_chol.hip, DESIGN.md
 * section 3.17): the O(n^3) step of the loop-closure LM on the matrix cores (v_mfma_f64_16x16x4_f64), n = 9N, any n >= 1.
 * Storage contract.  A: n x n row-major device doubles.  islam_dense_chol_factor READS the strict upper triangle of A and diag (n) --
 * the diagonal of the matrix, A's own diagonal is not read -- and WRITES L into the lower triangle and the diagonal of A.  The strict
 * upper triangle and diag are never written: factoring the same linearisation again with another diag (the LM's growing damping)
 * needs no restoration, and no second n x n array exists at any time.  islam_dense_chol_solve reads the lower triangle and the
 * diagonal of that array only and solves L y = b, L^T x = y for one right-hand side; x may alias b (neither may overlap the workspace).
 * Pivot rule.  The pivot of column c is d = a_cc - sum_k l_ck^2 as computed; d <= 0 or d not finite fails.  info (one device int,
 * rewritten by every factor call) receives c + 1 for the first failing column (LAPACK's potrf numbering), 0 when none fails.  After a
 * failed pivot every remaining launch still runs and terminates (no loop depends on data); the lower triangle then holds unspecified
 * values (NaN among them), and a solve on it returns unspecified values without faulting.
 * Determinism.  No atomics, every sum in an order fixed by n: the same inputs give the same bits on every call.
 * Both calls only enqueue on `stream`: no read-back, no synchronisation.  With nb = ceil(n / 64): the factor is 3 nb - 1 launches (per
 * block column the MFMA update of all rows below, the diagonal block in one workgroup, the panel by substitution; the last column
 * has no panel), the solve 2 nb launches and one device-to-device copy of b.
 * workspace: islam_dense_chol_workspace_bytes(n) bytes (two vectors of n doubles; 0 for n < 1), shared by both calls.
 * ISLAM_EARG before any HIP call for n < 1, a NULL pointer or a workspace that is too small. */
size_t islam_dense_chol_workspace_bytes(int n);
int islam_dense_chol_factor(double* A, const double* diag, int n, void* workspace, size_t workspace_bytes,
                            int* info /* device */, void* stream);
int islam_dense_chol_solve(const double* L, int n, const double* b, double* x /* may alias b */,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Inverse of that factor in place and covariance blocks from it (csrc/dense_inverse.hip): Sigma = A^-1 = W^T W
 * with W = L^-1, for the marginal covariances of loop-closure graphs.
 * islam_dense_chol_invert_factor.  L: the n x n array islam_dense_chol_factor left (info = 0).  READS and WRITES the lower triangle and the
 * diagonal only: W = L^-1 replaces L.  The strict upper triangle (the matrix's own entries) is never written and never read as data:
 * every load whose column can exceed its row is predicated and gives 0 there, so NaN above the diagonal cannot reach the result.
 * Block columns of 64: one launch inverts every diagonal block (one wave each), then per block column, descending, T = -L_below W_jj
 * (stored transposed in the workspace) and W_below = tril(W_trailing) T, both on v_mfma_f64_16x16x4_f64.  With nb = ceil(n / 64):
 * 2 nb - 1 launches.  workspace: islam_dense_chol_inverse_workspace_bytes(n) bytes (one 64 x n panel of doubles; 0 for n < 1).
 * islam_pvgo_dense_cov_blocks.  W: that inverse, n = 9 N.  node_cov (N,9,9) device: Sigma_kk = sum_{i >= 9k} W[i, 9k:9k+9]^T W[i, 9k:9k+9].
 * pair_cov (P,9,9) device: Sigma_ab (rows node a, columns node b) for every pairs[p] = (a, b), any a, b in [0, N), a > b and a = b
 * included; both are sums over the rows i >= 9 max(a, b) of the lower triangle only.  pairs: (P,2) int64 in HOST memory -- it is
 * validated here and travels to the device as kernel arguments (384 pairs per launch), so nothing is copied and the array may be
 * freed when the call returns.  P = 0 with pairs = NULL is allowed; node_cov or pair_cov may be NULL to skip it.  anchor >= 0: the six
 * pose rows / columns of that node are written as zero in every block that touches them (the gauge was fixed there by unit rows in
 * the matrix); -1: none.  One workgroup per block, rows strided over its threads, reduced in a fixed order; the (b, a) block is the
 * transpose of the (a, b) block to the bit.  1 + ceil(P / 384) launches.
 * Both calls only enqueue on `stream`.  Dependencies are launch boundaries: no atomics, no spin-waits, no cooperative launches, no loop
 * whose trip count depends on data -- on a factor that holds NaN (a failed pivot) every launch still terminates.  Every sum runs in an
 * order fixed by n (and the pair): a second call gives the same bits.
 * ISLAM_EARG before any HIP call for n < 1, n not a multiple of 9 (cov_blocks), a NULL matrix, a NULL or too small workspace, an anchor
 * outside [-1, N), P < 0, P > 0 without pairs, or a pair index outside [0, N). */
size_t islam_dense_chol_inverse_workspace_bytes(int n);
int islam_dense_chol_invert_factor(double* L, int n, void* workspace, size_t workspace_bytes, void* stream);
int islam_pvgo_dense_cov_blocks(const double* W, int n, int anchor, const int64_t* pairs /* host */, int P,
                                double* node_cov, double* pair_cov, void* stream);
/* Marginal covariances of a loop-closure graph from its band form A = B + R (csrc/pvgo_band_cov.inl), without
 * any (9N)^2 array: Sigma = B_a^-1 - Y_c G Y_c^T.  B = (Hd, Ho) as islam_pvgo_band_assemble leaves it, B_a = B with the six pose rows and
 * columns of node `anchor` replaced by the identity (-1: none); cols (R) int64 in HOST memory: DoF indices 9 node + c in [0, 9N), none of
 * them a pose DoF of the anchor, the first Rc of them the pose DoF of the closure ends (islam_amd.pvgo_dense.band_columns);
 * Y_c = B_a^-1[:, cols[:Rc]]; G (Rc x Rc, symmetric) = (I + M Y_S)^-1 M with M = R and Y_S = Y_c on those DoF, formed by the caller.
 * islam_pvgo_band_inverse_columns.  Y (9N x ldy row-major, ldy >= R): Y[:, r] = B_a^-1 e_cols[r], the anchor's pose rows exactly zero.  One
 * launch writes the anchored copy of (Hd, Ho) into the workspace (Hd, Ho are not written); every column is one unit right-hand side
 * through the chain solver (what islam_pvgo_solve_chain_enqueue runs, damping 0), enqueued from a loop here; one launch transposes the
 * solutions into Y.  status (one device int, or NULL): ISLAM_ENOTPD if any solve met a non-positive pivot, ISLAM_OK otherwise.
 * islam_pvgo_band_cov_blocks.  Sd (N,9,9), So (N-1,9,9): islam_pvgo_marginals of the same (Hd, Ho) and anchor.  G: 16 ceil(Rc / 16) rows of
 * ldg >= 16 ceil(Rc / 16) doubles, zero outside its leading Rc x Rc (the matrix-core kernel reads whole 16-column chunks of it).
 * V = Y[:, :Rc] G on v_mfma_f64_16x16x4_f64 (kept in the workspace), then node_cov (N,9,9): Sd[k] - V_k Y_k^T over the first Rc columns,
 * entries (p, q) and (q, p) averaged, and pair_cov (P,9,9): base(a, b) - V_a Y_b^T for every pairs[p] = (a, b) ((P,2) int64 in HOST memory,
 * any a, b in [0, N)), base = Sd[a] for a = b (averaged likewise: equal to node_cov[a] to the bit), So[a] for b = a + 1, So[b]^T for
 * a = b + 1, otherwise the rows of node a of Y at the columns where cols holds the DoF of node b -- ISLAM_EARG if cols lacks one of them
 * other than the anchor's pose DoF.  A far pair (a, b) with a > b whose node a has its DoF in cols too is formed as block (b, a) and stored
 * transposed, so that the two orders of one pair give transposes of each other to the bit (the columns of B_a^-1 come from separate
 * solves and are symmetric only up to rounding times the condition number).  The pose rows / columns of the anchor are exactly zero in
 * every block.  node_cov or pair_cov may be
 * NULL to skip it; Rc = 0 (no closure): the blocks of the chain inverse are copied through, G and the workspace may be NULL.  status (one
 * device int, or NULL): ISLAM_ENOTPD if a diagonal entry of node_cov outside the anchor's pose DoF is not finite or not positive.
 * Launches: the projection, one for node_cov, and one per 160 pairs (or 48 distinct far second nodes).
 * workspace: islam_pvgo_band_inverse_workspace_bytes(N, R) bytes serve both calls (the chain solver's workspace, the anchored band, and
 * 9N x 16 ceil(R / 16) doubles; 0 for N < 2 or R < 0).  Both calls only enqueue on `stream`; no atomics, every sum in an order fixed by the
 * shapes: the same inputs give the same bits.  ISLAM_EARG before any HIP call for N < 2, R < 0, Rc outside [0, R], ldy < R, ldg too
 * small, an anchor outside [-1, N), a missing array, a workspace that is too small, or an index of cols / pairs out of range. */
size_t islam_pvgo_band_inverse_workspace_bytes(int N, int R);
int islam_pvgo_band_inverse_columns(const double* Hd, const double* Ho, int N, int anchor, const int64_t* cols /* host */, int R,
                                    const int seg_len[2], void* workspace, size_t workspace_bytes, double* Y, int ldy,
                                    int* status /* device */, void* stream);
int islam_pvgo_band_cov_blocks(const double* Sd, const double* So, const double* Y, int ldy, int N, int anchor,
                               const int64_t* cols /* host */, int R, int Rc, const double* G, int ldg, const int64_t* pairs /* host */,
                               int P, void* workspace, size_t workspace_bytes, double* node_cov, double* pair_cov,
                               int* status /* device */, void* stream);
/* vo_loss forward/backward (pvgo.py:67-78 with PyPose's left-tangent gradient convention).
 * fwd: e (E,6) = Log(P^-1 Xi^-1 Xj); trans_loss, rot_loss (E).  bwd: grad_poses (E,7), last column 0. */
int islam_pvgo_vo_loss_fwd(const double* nodes, const int64_t* edges, const double* poses, int E,
                           double* err6, double* trans_loss, double* rot_loss, void* stream);
int islam_pvgo_vo_loss_bwd(const double* poses, const double* err6, const double* g_trans, const double* g_rot,
                           int E, double* grad_poses, void* stream);
/* align_to (pvgo.py:114-119): nodes <- target * nodes[0]^-1 * nodes ; vels <- R(target) R(nodes[0])^-1 vels */
int islam_pvgo_align(const double* nodes, const double* vels, const double* target7, int N,
                     double* nodes_out, double* vels_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISLAM_HIP_H */
