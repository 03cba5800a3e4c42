/* ep24 - C ABI of the MI355X-native YOLOX-24p training path (libep24.so, gfx950 only).
 *
 * The reference (IN2-ViAUn/Exploration-of-Potential, /root/reference) has NO native/FFI boundary on this
 * path: it is plain Python over torch ops.  The drop-in surface is therefore the reference's Python API
 * (exploration-of-potential_amd/yolox_24p mirrors it) and this C ABI sits one level below it: every entry
 * point replaces the torch-op sequence of one row of SURVEY.md section 8(a), cited per function as
 * file:line under /root/reference.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller owns every buffer
 *   - `stream` is a hipStream_t (passed as void*); nothing here allocates, frees or synchronises
 *   - activations are NHWC bf16 with an explicit row stride `ld_*` (elements between consecutive pixels),
 *     so a tensor may be a channel slice of a wider (concat) buffer
 *   - conv weights are [Cout][KH*KW][Cin] ("KRSC"); fp32 masters, bf16 packed copies
 *   - return 0 on success, a negative EP24_E_* otherwise; text via ep24_last_error()
 */
#ifndef EP24_H
#define EP24_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EP24_OK 0
#define EP24_E_ARG (-1)          /* bad shape / alignment / null pointer (reference raises IndexError/assert) */
#define EP24_E_LAUNCH (-2)       /* HIP launch error */
#define EP24_E_UNSUPPORTED (-3)

#define EP24_MAX_GT 50           /* max_labels, yolox_24p/datasets/data_augment.py:131 */
#define EP24_RAYS 24
#define EP24_LABEL_COLS 51
#define EP24_NUM_SUMS 32         /* per-step loss accumulators, see ep24_loss_* */

const char* ep24_last_error(void);
/* Bumped whenever an exported signature or the meaning of an argument changes.  2 (round 4): ep24_bn_act_bwd_reduce / _apply /
 * _apply_acc and ep24_pack_weights_batched took new arguments in round 3, ep24_conv_set_patch went away, the BatchNorm-backward sums
 * became 2^-36 fixed point, ep24_circle_lens is new.  A caller built against another version must not call in. */
#define EP24_ABI_VERSION 3
int ep24_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * a1  conv + BN + SiLU blocks  (yolox_24p/models/network_blocks.py:29-54 BaseConv.forward and its autograd)
 * ------------------------------------------------------------------------------------------------ */

/* y[B,OH,OW,Cout] = conv(x[B,H,W,Cin], w[Cout][k*k][Cin]), pad (k-1)/2, bf16 MFMA implicit GEMM, fp32
 * accumulate.  y is bf16 (y_f32=0) or fp32 (y_f32=1, + bias) with row stride ld_y.  If `stats` is non-null
 * the per-channel sum and sum-of-squares of the fp32 results are atomically added, as 2^-20 fixed point
 * int64 (order independent => bitwise reproducible), into stats[replica][0][c] / stats[replica][1][c]
 * (replica = block % stats_replicas): the BN batch statistics (torch.nn.BatchNorm2d training mode,
 * network_blocks.py:47).  Requires Cin % 8 == 0.
 * Output pixel (n,oh,ow) lands on row n*y_batch_rows + y_row0 + oh*OW + ow of y (y_batch_rows = 0 means
 * dense OH*OW): lets the head write straight into its slice of the [B,8400,107] tensor. */
int ep24_conv_fwd_bf16(const void* x, int64_t ld_x, const void* w, void* y, int64_t ld_y, int y_f32,
                       int64_t y_batch_rows, int64_t y_row0, const float* bias, int64_t* stats, int stats_replicas,
                       int B, int H, int W, int Cin, int Cout, int ksize, int stride, void* stream);

/* The same two entry points with an explicit kernel choice PER CALL (A/B timing, tests that compare two kernels on one shape;
 * there is no process-wide switch).  kernel_opts bit 0: the 3x3 stride-1 layers run in the generic tiled kernel instead of the
 * halo-patch kernels; bit 1: the tiled kernels store their output 8 bytes per lane instead of staging it for 16-byte stores (a store-width
 * option: the same bits in y, dx - accumulated too - and the statistics; it is also what runs without the bit for Cout % 8 != 0, ld % 8 != 0
 * or a destination that is not 16-byte aligned, in the tiled, ring and 8-wave kernels alike);
 * bit 2: a stride-2 input gradient runs as one launch per parity class (four) instead of one merged launch; bit 3: the 3x3
 * stride-1 layers run in the 8-wave lockstep halo-patch kernel (csrc/conv_patch.hip) instead of the loader / consumer ring
 * (csrc/conv_ring.hip, the default since round 4);
 * bit 4: reserved, refused (EP24_E_UNSUPPORTED; it selected the ring without a patch);
 * bit 5: reserved, refused (the ring's 32 x 32 x 16 consumers);
 * bit 6: reserved, refused (the ring's 256 x 64 tile);
 * bit 7: the tiled kernel without its three-stage form (round 4: layers whose 128-wide tiles leave at most one workgroup per
 * CU - the 20 x 20 level at B = 20 - run in 128-wide tiles with three LDS stages and two tiles in flight; with bit 7 they run in 64-wide
 * two-stage tiles as before; bit-identical results); bit 8: 1x1 stride-1 layers with 128 < K <= 256 and fewer than 100 000 pixels run
 * in the tiled kernel, as they did before the streaming kernel's weight tile was requested in one batch (round 5: the streaming kernel
 * is the default for every 1x1 stride-1 layer with K <= 256 now; y and a first-writer dx are bit-identical either way, an ACCUMULATED dx
 * is not - the tiled kernel rounds twice, the streaming kernel once: see ep24_conv_dgrad_bf16); bit 9: 3x3 stride-1 layers with at most 64 channels on either side
 * run in the tiled kernel instead of conv_wreg_kernel (round 5, csrc/conv_wreg.hip: every weight fragment of the layer in registers,
 * persistent workgroups, one LDS window per tap row; bit-identical outputs, the batch statistics equal to fp32 summation order; the
 * default for such layers with at least 65 536 pixels, an image at least 32 wide and a plain first-writer destination).  kernel_opts = 0 is exactly ep24_conv_fwd_bf16 / ep24_conv_dgrad_bf16, and every default kernel of a 3x3 stride-1
 * layer (ring, 8-wave halo patch, tiled) gives bit-identical results. */
/* Bits 4, 5 and 6 (and bit 0 of the weight gradient's kernel_opts) selected variants that were built, measured and lost in rounds
 * 3 - 4; they were removed, their source is at commit 6cc7180. */
/* Always 0: kept so that version-3 callers keep binding. */
int ep24_ab_variants(void);
int ep24_conv_fwd_bf16_ex(const void* x, int64_t ld_x, const void* w, void* y, int64_t ld_y, int y_f32,
                          int64_t y_batch_rows, int64_t y_row0, const float* bias, int64_t* stats, int stats_replicas,
                          int B, int H, int W, int Cin, int Cout, int ksize, int stride, int kernel_opts, void* stream);
int ep24_conv_dgrad_bf16_ex(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx, int accumulate,
                            int B, int H, int W, int Cin, int Cout_k, int ksize, int stride, int kernel_opts, void* stream);

/* The 3x3 stride-1 layers run as a loader / consumer ring (csrc/conv_ring.hip: 4 MFMA waves fed by 4 LDS-DMA waves through counters
 * in LDS).  Every wait on a counter is a bounded spin; this returns how many of them have given up since the library was loaded
 * (reads a device word: synchronises with the device; the grid-wide wait of the fused BatchNorm backward counts in).  Always 0 unless
 * the hand-off protocol is broken - tests assert it. */
int ep24_conv_ring_timeouts(void);

/* Input gradient of a stride-1 conv that is the ONLY consumer of the conv-BN-act unit below it (a Bottleneck's 3x3 over its 1x1,
 * network_blocks.py:54-79): dx IS that unit's dy, so the epilogue also takes the unit's two BatchNorm-backward sums - what
 * ep24_bn_act_bwd_reduce would compute from dx and z - from the tile on its way out.  z [B*H*W][ld_z]: the unit's conv output;
 * mean / invstd / gamma / beta [Cin]; dgamma / dbeta: fixed-point sums, replica r at + r * rep_stride.  First writer only (dx is
 * overwritten); Cin, ld_dx, ld_z multiples of 8. */
int ep24_conv_dgrad_bnr_bf16(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx, int B, int H, int W, int Cin,
                             int Cout_k, int ksize, const void* z, int64_t ld_z, const float* mean, const float* invstd,
                             const float* gamma, const float* beta, int64_t* dgamma, int64_t* dbeta, int64_t rep_stride, int reps,
                             int act, void* stream);

/* Which device kernel ep24_conv_fwd_bf16 (dgrad = 0) / ep24_conv_dgrad_bf16 (dgrad = 1, stride 1) launches for a shape - the
 * library's own dispatch rule, for reports (bench.py attributes launch times to kernels with it).  Returns 0 =
 * igemm_dma_kernel (generic tiled), 1 = conv_patch_kernel (halo patch, 8 waves in lockstep), 2 = igemm_stream_kernel (1x1
 * streaming), 3 = conv_ring_kernel (halo patch as a loader / consumer ring), 6 = conv_wreg_kernel
 * (3x3 stride-1, at most 64 channels on either side: weights in registers), < 0 on error.
 * 4: reserved, never returned.
 * 5: reserved, never returned.
 * y_f32 / has_bias as in ep24_conv_fwd_bf16 (both 0 for dgrad). */
int ep24_conv_kernel_for(int dgrad, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int y_f32, int has_bias);
/* ... and for the _ex entry points with the given kernel_opts. */
int ep24_conv_kernel_for_ex(int dgrad, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int y_f32, int has_bias,
                            int kernel_opts);

/* dx[B,H,W,Cin] (+)= conv_transpose(dy[B,OH,OW,Cout_k], wt[Cin][k*k][Cout_k]); Cout_k % 8 == 0 (zero padded).
 * wt is the pure transpose of w (no tap flip).  Replaces autograd's conv input gradient.
 * accumulate = 0: dx = bf16(acc), acc the fp32 sum.  accumulate = 1, by the kernel that runs (ep24_conv_kernel_for(1, ...)):
 *   - the streaming 1x1 kernel (id 2: 1x1 stride-1 with Cout_k <= 256; also ep24_conv1x1_dgrad_bnr_bf16 and
 *     ep24_conv1x1_dgrad_bnbwd_bf16, which are forms of it): dx = bf16(acc + float(dx)) - ONE rounding;
 *   - every other kernel (tiled - all stride-2 input gradients, merged or per parity class, and 1x1 layers under kernel_opts bit 8
 *     -, ring, 8-wave halo patch; the weights-in-registers kernel does not accumulate, its layers run in the tiled kernel then):
 *     dx = bf16(float(bf16(acc)) + float(dx)) - TWO roundings, through the 16-byte and the 8-byte store path alike (kernel_opts
 *     bit 1, ld_dx % 8 != 0, Cin % 8 != 0 or a dx that is not 16-byte aligned select the path, never the value).
 * tests/test_gpu_conv_exact.py holds every path to its form bit for bit. */
int ep24_conv_dgrad_bf16(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx, int accumulate,
                         int B, int H, int W, int Cin, int Cout_k, int ksize, int stride, void* stream);

/* dw[co][t][ci] += sum_pixels dy[.,co] * x[.@t,ci]   fp32, row stride ld_dw between co rows (= taps*cin_valid
 * when dense), only co < cout_valid and ci < cin_valid are written.  Split over pixels with fp32 atomics.
 * Replaces autograd's conv weight gradient. */
int ep24_conv_wgrad_bf16(const void* x, int64_t ld_x, const void* dy, int64_t ld_dy, float* dw, int64_t ld_dw,
                         int cout_valid, int cin_valid,
                         int B, int H, int W, int Cin, int Cout, int ksize, int stride, void* stream);

/* The same weight gradient without atomics (bitwise reproducible): pixel split s of the launch stores its partial
 * dW (layout of dw above, cout_valid * ld_dw floats) at slab + s * cout_valid * ld_dw with plain stores; every
 * element of every split is written.  ep24_conv_wgrad_splits returns the number of splits that launch uses (>= 1, a
 * pure function of the shape), so the caller can size the slab; ep24_wgrad_reduce then does, for n_layers rows
 * desc[i] = (grad offset, numel, splits, slab offset) (all in floats), grad[off + j] += sum_s slab[soff + s*numel + j]
 * in a fixed order.  Together they replace autograd's conv weight gradient for the training engine. */
int ep24_conv_wgrad_splits(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
int ep24_conv_wgrad_slab_bf16(const void* x, int64_t ld_x, const void* dy, int64_t ld_dy, float* slab, int64_t slab_floats,
                              int64_t ld_dw, int cout_valid, int cin_valid,
                              int B, int H, int W, int Cin, int Cout, int ksize, int stride, void* stream);
/* The same two with a kernel_opts argument.  Bit 0: reserved, refused (EP24_E_UNSUPPORTED at the launch; it selected the weight gradient as a ring). */
int ep24_conv_wgrad_splits_ex(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int kernel_opts);
int ep24_conv_wgrad_slab_bf16_ex(const void* x, int64_t ld_x, const void* dy, int64_t ld_dy, float* slab, int64_t slab_floats,
                                 int64_t ld_dw, int cout_valid, int cin_valid, int B, int H, int W, int Cin, int Cout, int ksize,
                                 int stride, int kernel_opts, void* stream);
/* Round 5: up to 16 weight gradients of ONE tile class in one launch (a weight gradient is needed by nobody before the optimizer and
 * every layer keeps its dz and its input, so the layers of a backward segment wait for each other; grouped they fill the chip without
 * being cut into many short pixel splits).  desc is a HOST array [n][17] of int64 - x, ld_x, dy, ld_dy, slab, slab_floats, ld_dw,
 * cout_valid, cin_valid, B, H, W, Cin, Cout, ksize, stride, splits - read during the call; `splits` (>= 1) is the caller's: slab s
 * of problem i receives the partial sums of its s-th run of ceil(steps / splits) 64-pixel steps, ep24_wgrad_reduce folds them.
 * ep24_conv_wgrad_tile_class: bit 0 = 64-wide tiles over Cout (else 128), bit 1 = 64-wide tiles over Cin; one class per launch. */
int ep24_conv_wgrad_tile_class(int Cin, int Cout, int ksize);
int ep24_conv_wgrad_group_bf16(const int64_t* desc, int n, void* stream);
int ep24_wgrad_reduce(const int64_t* desc, int n_layers, int64_t max_numel, float* grad, const float* slab, void* stream);

/* fp32 master [Cout][T][Cin] (row stride ld_w) -> bf16 w_fwd [Cout][T][Cin_pad] and bf16 w_dgrad
 * [Cin][T][Cout_pad] (either may be null).  Only real elements are written; the caller zero-initialises the
 * padded buffers once. */
int ep24_pack_weights(const float* w, int64_t ld_w, void* w_fwd, void* w_dgrad, int Cout, int T, int Cin,
                      int Cin_pad, int Cout_pad, void* stream);

/* The same for every conv segment of a model in one launch.  desc [n_seg][8] int64 = {master offset, w_fwd offset,
 * w_dgrad offset or -1, Cout, T, Cin, Cin_pad, Cout_pad} (element offsets into flat / w_fwd / w_dgrad); prefix
 * [n_seg+1] int64 = running sum of Cout*T*Cin (total = prefix[n_seg]); tile_prefix [n_seg+1] = running sum of
 * T*ceil(Cout/64)*ceil(Cin/64), the 64x64 tiles of the LDS transpose that writes w_dgrad coalesced.
 * chunk_seg [ceil(total/4096)] int32 = segment of element 4096*c and tile_seg [total_tiles] int32 = segment of tile t are
 * optional lookup tables built once by the host (NULL: the kernels bisect the prefix tables, eight dependent loads per chunk).
 * which: 0 both copies, 1 w_fwd only, 2 w_dgrad only (backward is the first to read it).
 * w_fwd: only real elements are written, as in the single-layer form.  w_dgrad: where a segment's Cout_pad and w_dgrad offset are
 * multiples of 8 the rows leave as 16-byte stores, so its Cout padding columns (Cout <= co < Cout_pad) MAY be rewritten, and only
 * with +0 - the caller still zero-initialises them once, and they hold +0 after every call.  Nothing outside a segment's
 * [Cin][T][Cout_pad] block is written, and nothing of a copy that `which` excludes. */
int ep24_pack_weights_batched(const float* flat, const int64_t* desc, const int64_t* prefix, const int64_t* tile_prefix,
                              int n_seg, void* w_fwd, void* w_dgrad, int64_t total, int64_t total_tiles,
                              const int32_t* chunk_seg, const int32_t* tile_seg, int which, void* stream);

/* y = silu(bn(z)) (+ residual), training-mode BatchNorm with batch statistics taken from `stats`
 * ([replicas][2][C] fixed-point sums over the M rows, as written by ep24_conv_fwd_bf16).  Also writes save[0][c]=mean,
 * save[1][c]=invstd for the backward and updates running_mean / running_var (unbiased) / num_batches_tracked
 * (momentum, eps: yolox_24p/exp/yolox_base.py:58-62).  act: 1 = SiLU, 0 = identity. */
int ep24_bn_act_fwd(const void* z, int64_t ld_z, const int64_t* stats, int stats_replicas, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, int64_t* num_batches, int64_t* num_batches2,
                    float* save, void* y, int64_t ld_y, const void* residual, int64_t ld_res,
                    int64_t M, int C, float eps, float momentum, int act, void* stream);   /* num_batches2: the counter of the
                    second BatchNorm module when two units share the launch (merged CSP / head pairs), else NULL */

/* pass 1 of the backward: dgamma[c] += sum du*zhat, dbeta[c] += sum du, du = dy * silu'(bn(z)); the sums are
 * 2^-36 fixed-point int64 (NOT the forward statistics' 2^-20: gradient sums of the head are 1e-5 .. 1e-4 per workgroup; a workgroup's
 * partial sum must stay below 2^20 in magnitude - one that does not, or is NaN, makes the channel's folded sum NaN), kept in `reps` replicas (replica r of either sum 2*C*r elements behind
 * the pointer, i.e. [reps][2][C] when dbeta = dgamma + C; a workgroup adds to replica blockIdx % reps): the memory-side atomic
 * units serialise the adds to one address, and with a single copy every workgroup of the launch hit the same 2 C addresses. */
int ep24_bn_act_bwd_reduce(const void* dy, int64_t ld_dy, const void* z, int64_t ld_z, const float* save,
                           const float* gamma, const float* beta, int64_t* dgamma, int64_t* dbeta,
                           int64_t M, int C, int act, int reps, void* stream);
/* pass 2: dz = gamma*invstd*(du - dbeta/M - zhat*dgamma/M)  -> bf16 [M,C] (ld_dz).  dgamma/dbeta are this
 * call's sums (scratch, zeroed by the caller before pass 1); if gamma_grad/beta_grad are non-null they
 * receive += of those sums (the parameter .grad accumulators).  The `reps` replicas of the sums (layout as in pass 1) are
 * folded exactly (integers) by every workgroup.  save, gamma, beta, gamma_grad and beta_grad are read / updated 8 channels at
 * a time as 16-byte vectors: they must be 16-byte aligned (C % 8 == 0 already). */
int ep24_bn_act_bwd_apply(const void* dy, int64_t ld_dy, const void* z, int64_t ld_z, const float* save,
                          const float* gamma, const float* beta, const int64_t* dgamma, const int64_t* dbeta,
                          float* gamma_grad, float* beta_grad, void* dz, int64_t ld_dz, int64_t M, int C, int act,
                          int reps, void* stream);

/* The input gradient of a 1x1 stride-1 conv of the streaming kernel (Cout_k <= 256) that ALSO takes the BatchNorm-backward sums of the
 * unit below (round 5): what it stores - with `accumulate`, old + new: the complete gradient over a shortcut - is that unit's dy, so
 * sum(du) and sum(du * zhat) are added to dgamma / dbeta ([reps][..] 2^-36 fixed point, replica stride rep_stride, zeroed by the caller)
 * from the rounded rows on their way out, with ep24_bn_act_bwd_reduce's expressions (the fp32 order of the partial sums differs); that
 * unit's reduce launch is not needed.  dx is bit-identical to ep24_conv_dgrad_bf16's.  z / mean / invstd / gamma / beta: the unit below
 * (act = 1, SiLU).  EP24_E_UNSUPPORTED for a shape the streaming kernel does not take. */
int ep24_conv1x1_dgrad_bnr_bf16(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx, int accumulate, int B, int H, int W,
                                int Cin, int Cout_k, const void* z, int64_t ld_z, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, int64_t* dgamma, int64_t* dbeta, int64_t rep_stride, int reps,
                                int act, void* stream);

/* Depthwise 3x3 convolution (groups = channels) of the DWConv blocks (yolox_24p/models/network_blocks.py:57-76: a depthwise BaseConv
 * followed by a 1x1 BaseConv; `depthwise=True` of CSPDarknet / Bottleneck / YOLOPAFPN / YOLOXHead, darknet.py:107, network_blocks.py:92,
 * yolo_pafpn.py:30, yolo_head_24p.py:45 - in no BASELINE configuration).  HBM-bound elementwise kernels (csrc/dwconv.hip): NHWC bf16
 * activations, w = the fp32 master [C][3][3] read in place, fp32 accumulation, stride 1 or 2, pad 1; C % 8 == 0.
 *   fwd:   z = conv(x, w); `stats` as ep24_conv_fwd_bf16 ([replicas][2][C] fixed-point batch statistics, ADDED to what the buffer
 *          holds, workgroup b into replica b % replicas), or NULL.  As in ep24_conv_fwd_bf16 the statistics are those of the fp32
 *          accumulator BEFORE its rounding to bf16, not of the stored z (tests/test_gpu_backbone_exact.py pins this).
 *   dgrad: dx (+)= the input gradient from dz [B,OH,OW,C].
 *   wgrad: slab [splits][C][9] fp32 = per-workgroup partial sums of dw, splits = ep24_dwconv_wgrad_splits(...) (fixed by the shape);
 *          ep24_wgrad_reduce folds them in order into the flat gradient, as for every other weight gradient (no atomics).
 * BatchNorm + activation of the unit are the ep24_bn_act_* entry points. */
int ep24_dwconv_fwd_bf16(const void* x, int64_t ld_x, const float* w, void* z, int64_t ld_z, int64_t* stats, int stats_replicas,
                         int B, int H, int W, int C, int ksize, int stride, void* stream);
int ep24_dwconv_dgrad_bf16(const void* dz, int64_t ld_dz, const float* w, void* dx, int64_t ld_dx, int accumulate, int B, int H,
                           int W, int C, int ksize, int stride, void* stream);
int ep24_dwconv_wgrad_splits(int B, int H, int W, int C, int stride);
int ep24_dwconv_wgrad_slab_bf16(const void* x, int64_t ld_x, const void* dz, int64_t ld_dz, float* slab, int64_t slab_floats, int B,
                                int H, int W, int C, int ksize, int stride, void* stream);

/* A 1x1 stride-1 conv unit TOGETHER WITH the BatchNorm pass in front of it (round 5; csrc/conv_igemm.hip igemm_stream_kernel<XF>).
 * The streaming 1x1 kernel is the one conv kernel whose A operand passes through registers, so the pass that would have produced
 * that operand as a launch of its own runs on the rows in flight: one dependent launch and one read of the rows less, the same
 * values bit for bit (the rows the MFMAs read are the bf16 values that are stored).  Shapes: Cin, Cout <= 128 (one K pass, one N
 * tile); ep24_conv1x1_xf_ok says whether a shape is taken.  SiLU units only (act = 1).
 *   ep24_conv1x1_bnin_bf16: y_in = silu(bn(z_in)) (+ residual) exactly as ep24_bn_act_fwd (statistics fold, save, running
 *     statistics, counters), then z_out = conv1x1(y_in, w) with its batch statistics exactly as ep24_conv_fwd_bf16
 *     (network_blocks.py:50-51 of the producing unit and :38-48 of this one; Bottleneck.forward :95-99).
 *   ep24_conv1x1_dgrad_bnbwd_bf16: dz = ep24_bn_act_bwd_apply(dy, z, ...) - stored, the weight gradient reads it; the sums are
 *     published into gamma_grad / beta_grad - then dx (+)= dz . wt exactly as ep24_conv_dgrad_bf16 of the unit's 1x1 conv
 *     (Cin / Cout_k as there: the forward conv's input channels / its output channels padded to 8). */
int ep24_conv1x1_xf_ok(int B, int H, int W, int Cin, int Cout);
int ep24_conv1x1_bnin_bf16(const void* z_in, int64_t ld_zin, const int64_t* stats_in, int reps_in, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, int64_t* num_batches,
                           int64_t* num_batches2, float* save, void* y_in, int64_t ld_yin, const void* residual, int64_t ld_res,
                           float eps, float momentum, int act, const void* w, void* z_out, int64_t ld_zout, int64_t* stats_out,
                           int reps_out, int B, int H, int W, int Cin, int Cout, void* stream);
int ep24_conv1x1_dgrad_bnbwd_bf16(const void* dy, int64_t ld_dy, const void* z, int64_t ld_z, const float* save,
                                  const float* gamma, const float* beta, const int64_t* dgamma, const int64_t* dbeta,
                                  float* gamma_grad, float* beta_grad, void* dz, int64_t ld_dz, int act, int reps, const void* wt,
                                  void* dx, int64_t ld_dx, int accumulate, int B, int H, int W, int Cin, int Cout_k, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 PARITY MODE of the conv graph (csrc/f32path.hip).  The reference trains in fp32 (train_24p.py:86-104: no AMP,
 * network_blocks.py:50-51); ep24.engine.Engine(dtype=torch.float32) runs the same launch plan on fp32 activations through
 * these entry points so that images -> SimOTA indices / loss / gradients can be compared with the CPU oracle at fp32
 * accuracy (tests/test_gpu_fp32.py).  One thread per output element, reductions in double: not a fast path.
 * All tensors NHWC fp32 with a row stride in elements; weights are read in place from the flat fp32 master:
 * element (co, tap, ci) at w[co * w_co_stride + tap * w_tap_stride + ci].
 * ------------------------------------------------------------------------------------------------ */
int ep24_f32_stem_pack(const float* images, float* rows, int64_t ld, int B, int H, int W, void* stream);            /* Focus + 3x3 im2col */
/* transposed = 0: y = conv(x, w) (+ bias) with the row mapping of ep24_conv_fwd_bf16 (network_blocks.py:38-51);
 * transposed = 1: x is dy [B,OH,OW,Cout], y is dx [B,H,W,Cin] (+)= the input gradient.  B,H,W,Cin,Cout,ksize,stride always
 * describe the FORWARD convolution. */
int ep24_f32_conv(const float* x, int64_t ld_x, const float* w, int64_t w_co_stride, int64_t w_tap_stride, float* y, int64_t ld_y,
                  int64_t y_batch_rows, int64_t y_row0, const float* bias, int accumulate, int B, int H, int W, int Cin, int Cout,
                  int ksize, int stride, int transposed, void* stream);
int ep24_f32_conv_wgrad(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, float* dw, int64_t w_co_stride,
                        int64_t w_tap_stride, int B, int H, int W, int Cin, int Cout, int ksize, int stride, void* stream);   /* dw += */
/* training-mode BatchNorm + activation (+ residual): batch statistics (two-pass, double) -> save[0]=mean, save[1]=invstd,
 * running statistics, num_batches; then y = act(bn(z)) + residual. */
int ep24_f32_bn_act_fwd(const float* z, int64_t ld_z, const float* gamma, const float* beta, float* running_mean, float* running_var,
                        int64_t* num_batches, float* save, float* y, int64_t ld_y, const float* residual, int64_t ld_res, int64_t M,
                        int C, float eps, float momentum, int act, void* stream);
/* both passes of its backward: sums [2C] double scratch; gamma_grad / beta_grad += (both, or both null: EP24_E_ARG for one alone);
 * dz written. */
int ep24_f32_bn_act_bwd(const float* dy, int64_t ld_dy, const float* z, int64_t ld_z, const float* save, const float* gamma,
                        const float* beta, double* sums, float* gamma_grad, float* beta_grad, float* dz, int64_t ld_dz, int64_t M,
                        int C, int act, void* stream);
int ep24_f32_spp_fwd(const float* x, int64_t ld_x, float* y5, float* y9, float* y13, int64_t ld_y, int32_t* idx, int B, int H, int W,
                     int C, void* stream);      /* idx [3][B*H*W*C]: argmax pixel (y*W+x): the first maximum, the last NaN if there is one */
int ep24_f32_spp_bwd(const float* dy5, const float* dy9, const float* dy13, int64_t ld_dy, const int32_t* idx, float* dx,
                     int64_t ld_dx, int accumulate, int B, int H, int W, int C, void* stream);
int ep24_f32_upsample2_fwd(const float* x, int64_t ld_x, float* y, int64_t ld_y, int B, int H, int W, int C, void* stream);
int ep24_f32_upsample2_bwd(const float* dy, int64_t ld_dy, float* dx, int64_t ld_dx, int accumulate, int B, int H, int W, int C,
                           void* stream);
int ep24_f32_rows_copy(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int accumulate, int64_t M, int C, void* stream);
int ep24_f32_head_decode_bwd(const float* dout, const float* out, float* d_regobj, float* d_cls, int B, int A, int a0, int H, int W,
                             float stride, int ncols, const float* d_origin, void* stream);   /* d_regobj [cells,32], d_cls [cells,ceil8(C)] */
int ep24_f32_colsum(const float* g, int64_t ld, float* db, int64_t M, int N, void* stream);    /* db[c] += sum over rows */

/* ------------------------------------------------------------------------------------------------
 * a1/a2  glue ops of the graph
 * ------------------------------------------------------------------------------------------------ */
/* Focus + im2col for the 3x3 stem: images [B,3,S,S] fp32 NCHW -> rows [B*(S/2)^2][ld] bf16, columns
 * (kh,kw,c4) with c4 = TL,BL,TR,BR x 3 channels, 108 real + zero padding to ld (network_blocks.py:188-210).  images must be
 * 8-byte aligned (pixel pairs are one load), as for ep24_focus_pack. */
int ep24_stem_pack(const float* images, void* rows, int64_t ld, int B, int H, int W, void* stream);

/* The Focus stem without an im2col buffer (round 3; network_blocks.py:188-210, Focus.forward + its BaseConv 3x3 over 12 channels).
 * ep24_focus_pack: images [B,3,S,S] fp32 NCHW -> f16 [B][S/2][S/2][16] bf16, channel (x parity * 2 + y parity) * 3 + c (the
 * reference's cat(top-left, bottom-left, top-right, bottom-right)), channels 12..15 zero.
 * ep24_stem_conv_fwd_bf16: y[B*FH*FW][ld_y] = conv3x3(f16, w), w = [Cout][ld_w] bf16 with column tap * 12 + channel (the packed
 * forward copy of the [Cout][3][3][12] master); stats as ep24_conv_fwd_bf16.  _infer: y = act(acc + bias) (BatchNorm folded).
 * ep24_stem_conv_wgrad_slab_bf16: slab[s][Cout][108] = partial dW of pixel split s (column tap * 12 + channel), folded by
 * ep24_wgrad_reduce; ep24_stem_conv_wgrad_splits = the number of splits.  Cout <= 64 for the weight gradient. */
int ep24_focus_pack(const float* images, void* f16, int B, int H, int W, void* stream);
int ep24_stem_conv_fwd_bf16(const void* f16, const void* w, int64_t ld_w, void* y, int64_t ld_y, int64_t* stats, int stats_replicas,
                            int B, int FH, int FW, int Cout, void* stream);
int ep24_stem_conv_fwd_infer_bf16(const void* f16, const void* w, int64_t ld_w, const float* bias, int act, void* y, int64_t ld_y,
                                  int B, int FH, int FW, int Cout, void* stream);
int ep24_stem_conv_wgrad_slab_bf16(const void* f16, const void* dy, int64_t ld_dy, float* slab, int64_t slab_floats, int B, int FH,
                                   int FW, int Cout, void* stream);
int ep24_stem_conv_wgrad_splits(int B, int FH, int FW, int Cout);

/* SPP max pools k = 5, 9, 13, stride 1, pad k/2 over x[B,H,W,C] (network_blocks.py:131-143).  Writes the
 * three pooled maps into y5/y9/y13 (row stride ld_y) and the winning window offset (dy*16+dx biased by 8)
 * into idx [3][B*H*W][C] uint8 for the backward (first maximum in row-major window order, as ATen).
 * scratch: 9*B*H*W*C bytes, 8-byte aligned, for the separable two-pass form (row maxima + their column offsets); null = one pass. */
int ep24_spp_fwd(const void* x, int64_t ld_x, void* y5, void* y9, void* y13, int64_t ld_y, uint8_t* idx,
                 int B, int H, int W, int C, void* scratch, void* stream);
/* dx (+)= routed gradients of the three pools.  idx must be 8-byte aligned (the codes of 8 channels are one load). */
int ep24_spp_bwd(const void* dy5, const void* dy9, const void* dy13, int64_t ld_dy, const uint8_t* idx,
                 void* dx, int64_t ld_dx, int accumulate, int B, int H, int W, int C, void* stream);

/* nearest x2 upsample into a slice (yolo_pafpn.py:32) and its backward (sum of the 2x2 block). */
int ep24_upsample2_fwd(const void* x, int64_t ld_x, void* y, int64_t ld_y, int B, int H, int W, int C, void* stream);
int ep24_upsample2_bwd(const void* dy, int64_t ld_dy, void* dx, int64_t ld_dx, int accumulate,
                       int B, int H, int W, int C, void* stream);

/* hipMemsetAsync(p, 0, bytes) on the stream (step-start clearing of gradient / statistics buffers). */
int ep24_memset_zero(void* p, int64_t bytes, void* stream);
/* fp32 <-> bf16 casts of n (multiple of 4) contiguous elements: the bf16 wire format of the data-parallel gradient buckets
 * (ep24.dp.GradReducer(comm_dtype=torch.bfloat16): half the xGMI bytes of the reference's fp32 DDP buckets, core/trainer.py:163).
 * Four elements move per lane: the fp32 side must be 16-byte aligned and the bf16 side 8-byte aligned, else EP24_E_ARG. */
int ep24_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
int ep24_cast_bf16_f32(const void* src, float* dst, int64_t n, void* stream);

/* strided row copy / add:  dst[m, 0:C] (=|+=) src[m, 0:C]  (bf16).  The copy moves every bit pattern unchanged (NaN payloads, -0). */
int ep24_rows_copy(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int accumulate, int64_t M, int C,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * a3  head decode (yolox_24p/models/yolo_head_24p.py:212-237)
 * ------------------------------------------------------------------------------------------------ */
/* in place on out[B,A,107] fp32 rows of one level (anchor offset a0, HxW cells, stride s):
 * xy=(t+grid)*s, r=exp(t)*s, obj/cls logits untouched.  origin [B,A,26] (nullable) receives the raw regression
 * outputs first - the head's origin_preds under use_l1 (yolo_head_24p.py:179-188). */
int ep24_head_decode_fwd(float* out, int B, int A, int a0, int H, int W, float stride, int ncols, float* origin,
                         void* stream);
/* backward through the decode for one level + split into the padded bf16 gradients the prediction convs
 * consume: d_regobj [B*H*W][32] (26 reg + 1 obj + zeros), d_cls [B*H*W][round8(C)] (C classes + zeros).
 * d_origin [B,A,26] (nullable) is added to the raw regression gradient (the L1 branch's path around the decode). */
int ep24_head_decode_bwd(const float* dout, const float* out, void* d_regobj, void* d_cls, int B, int A, int a0,
                         int H, int W, float stride, int ncols, const float* d_origin, void* stream);
/* bias gradient: db[n] += sum_m g[m][n] for n < N (bf16 rows of stride ld). */
int ep24_colsum(const void* g, int64_t ld, float* db, int64_t M, int N, void* stream);
/* the same without atomics: ep24_colsum_splits(M) partial rows slab[s*N + n], folded in order by ep24_wgrad_reduce
 * with a row (offset, N, splits, slab offset). */
int ep24_colsum_splits(int64_t M);
int ep24_colsum_slab(const void* g, int64_t ld, float* slab, int64_t M, int N, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a4-a8  SimOTA assignment, batched over images, no host synchronisation
 *        (yolox_24p/models/losses.py:360-592, yolox_24p/utils/boxes.py:102-243)
 * ------------------------------------------------------------------------------------------------ */
/* a4+a5 (pts_in_poly + get_in_boxes_info, losses.py:497-592).  labels [B,50,51] fp32; xs/ys/strides [A].
 * Out: num_gt[B] int32 (rows with sum>0, losses.py:190), in_box[B*A], in_ctr[B*A] uint64 bitmasks over GTs.
 * Safe on any stream next to any other kernel.  (Round 2 measured different angle sums in lanes 48..63 of a wave when MFMA
 * kernels of another stream shared the SIMDs; the cause was a packed fp32 multiply with swapped operand halves that the
 * vectoriser had emitted - tools/hazard_probe.hip - and the library is built without such instructions since round 3:
 * DESIGN.md section 4, tests/test_abi.py::test_no_half_swapped_packed_fp32, tests/test_gpu_hazard.py.) */
int ep24_assign_candidates(const float* labels, const float* xs, const float* ys, const float* strides,
                           int32_t* num_gt, uint64_t* in_box, uint64_t* in_ctr, int B, int A, void* stream);
/* a6+a7 (bboxes_iou + class cost + total cost, boxes.py:166-243, losses.py:396-424) for every candidate
 * anchor: pw[B,50,A] and cost[B,50,A] fp32 (entries of non-candidate anchors / g >= num_gt are untouched).
 * At most 96 classes (the class terms of a workgroup's 64 anchors share its 24 x 256 floats of ray scratch): num_classes > 96
 * returns EP24_E_UNSUPPORTED before any launch and writes nothing; so does ep24_assign_cost_range. */
int ep24_assign_cost(const float* outputs, int ncols, const float* labels, const int32_t* num_gt,
                     const uint64_t* in_box, const uint64_t* in_ctr, float* pw, float* cost, int B, int A,
                     int num_classes, void* stream);
/* The same for anchors [a_lo, a_hi) of every image (round 5).  A pair's values do not depend on the launch's extent: launches over
 * disjoint ranges that cover [0, A) write exactly what ep24_assign_cost writes, so a head level's rows can be computed as soon as
 * that level's outputs exist (ep24.train: on the forward lane that produced them, off the loss path). */
int ep24_assign_cost_range(const float* outputs, int ncols, const float* labels, const int32_t* num_gt,
                           const uint64_t* in_box, const uint64_t* in_ctr, float* pw, float* cost, int B, int A,
                           int num_classes, int a_lo, int a_hi, void* stream);
/* a8 part 1 (dynamic_k_matching, losses.py:449-464): per (image, gt) top-10 pw sum -> k, the k cheapest
 * candidates are OR-ed into match[B*A] (uint64 bit g).  match must be zeroed by the caller; ks[B,50] out.
 * The candidate set is the IMAGE's: every anchor with any bit in in_box | in_ctr, whichever label set it (the reference's fg_mask),
 * P of them.  The min(10, P) largest pw are taken by (value descending, anchor ascending) and summed in that order in fp32,
 * k = max(1, trunc(sum)), and the min(k, P) smallest cost are taken by (value ascending, anchor ascending): on equal values the
 * lower anchor index wins, in both selections.  pw / cost of non-candidate anchors are read and dropped (they may hold anything);
 * nothing of g >= num_gt[b] is written - neither ks[b][g] nor bit g of match. */
int ep24_dynamic_k(const float* pw, const float* cost, const int32_t* num_gt, const uint64_t* in_box,
                   const uint64_t* in_ctr, uint64_t* match, int32_t* ks, int B, int A, void* stream);
/* a8 part 2 (losses.py:471-493): conflicts -> argmin cost, final fg mask, matched gt index (-1 = bg),
 * matched pairwise value. */
int ep24_assign_resolve(const uint64_t* match, const float* pw, const float* cost, const int32_t* num_gt,
                        int32_t* matched_gt, float* matched_iou, int B, int A, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a9+a10  losses and their gradient (yolox_24p/models/losses.py:80-157, :283-357)
 * ------------------------------------------------------------------------------------------------ */
/* per-block partial sums of the 24 circle-GIoU terms (matched rows), obj BCE (all anchors), cls BCE
 * (matched rows), num_fg; partials [nblocks][EP24_NUM_SUMS]; nblocks = ep24_loss_blocks(B, A). */
int ep24_loss_blocks(int B, int A);
/* L1 branch (use_l1, losses.py:197-198,255-262,304-309,594-604): origin [B,A,26] = the raw regression
 * outputs before the decode (null = branch off), xs/ys/strides [A] the anchor grid; adds sum |origin - l1_target| of
 * the matched rows as accumulator 27. */
int ep24_loss_terms(const float* outputs, int ncols, const float* labels, const int32_t* matched_gt,
                    const float* matched_iou, float* partials, int B, int A, int num_classes, const float* origin,
                    const float* xs, const float* ys, const float* strides, void* stream);
/* fixed-order reduction of the partials, dynamic task weights and state update (losses.py:286-345).
 * state[26] = last_{iou[24],obj,cls} (initialise to 1.0).  result[64]:
 *   [0] loss  [1..24] reg_w*loss_iou  [25] loss_obj  [26] loss_cls  [27] num_fg (clamped >= 1)
 *   [28] num_gts  [29..52] reg_w  [53] obj_w  [54] cls_w  [55] num_fg raw  [56] loss_l1 (added to [0] unweighted) */
int ep24_loss_finalize(const float* partials, int nblocks, const int32_t* num_gt, int B, float* state, float* result,
                       void* stream);
/* d loss / d outputs [B,A,ncols] fp32, scaled by *grad_scale (device scalar, may be null = 1).  With the L1 branch
 * (d_origin non-null) also d loss / d origin [B,A,26] = sign(origin - l1_target) / num_fg on matched rows, 0 elsewhere. */
int ep24_loss_grad(const float* outputs, int ncols, const float* labels, const int32_t* matched_gt,
                   const float* matched_iou, const float* result, const float* grad_scale, float* dout, int B, int A,
                   int num_classes, const float* origin, const float* xs, const float* ys, const float* strides,
                   float* d_origin, void* stream);

/* Round 5: ep24_loss_grad and ep24_head_decode_bwd of every level in ONE pass (the captured step, not the L1 branch): instead of the dense
 * fp32 [B,A,27+C] gradient it writes, per head level, the bf16 rows the prediction convs' backward consumes - reg+obj [B*cells][32] and
 * classes [B*cells][ld_cls = C rounded up to 8] - with the decode's chain rule applied (xy * stride, radii * decoded radius;
 * yolo_head_24p.py:212-237).  levels: HOST array [n_levels][4] of int64 = (cells per image, the stride's float32 bits, d_regobj, d_cls)
 * in anchor order; bit-identical to the two-launch form. */
int ep24_loss_grad_decode(const float* outputs, int ncols, const float* labels, const int32_t* matched_gt, const float* matched_iou,
                          const float* result, int B, int A, int num_classes, int n_levels, const int64_t* levels, void* stream);

/* stand-alone forms behind utils.bboxes_iou (boxes.py:166-243) and IOUloss.forward (losses.py:80-157) */
int ep24_circle_pairwise(const float* gt50, const float* pred26, float* out, int G, int P, void* stream);
int ep24_circle_matched_fwd(const float* pred26, const float* target50, float* loss24, int N, void* stream);
int ep24_circle_matched_bwd(const float* pred26, const float* target50, const float* dloss24, float* dpred26, int N,
                            void* stream);
/* circle_inter itself (IOUloss.circle_inter, losses.py:23-78; module-level utils.boxes.circle_inter, boxes.py:102-163):
 * intersection area of the k-th gt circle (radius gt_r[g][k]) with the k-th predicted circle and the centre distance,
 * res_inter / dist [pairs][24].  pairwise = 0: G == P rows matched one to one (the method); pairwise = 1: every gt row against
 * every pred row, pair index g * P + p (the module function's repeat_interleave / repeat order).  Case order as the reference:
 * |r1 - r2| >= d -> pi * rmin^2; d >= r1 + r2 -> 0 (overrides); else the lens with cosines clipped to +-0.99. */
int ep24_circle_lens(const float* gt_cx, const float* gt_cy, const float* gt_r, const float* pd_cx, const float* pd_cy,
                     const float* pd_r, float* res_inter, float* dist, int G, int P, int pairwise, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a11  optimizer (yolox_24p/exp/yolox_base.py:120-124: SGD momentum 0.9 nesterov, no decay - the default; the
 *      *_decay entry points below add stock YOLOX's weight decay by parameter group, yolox/exp/yolox_base.py:198-224)
 * ------------------------------------------------------------------------------------------------ */
/* flat fp32 p/g/buf of n elements: buf = first ? g : m*buf+g ; p -= lr*(g + m*buf); g is scaled by
 * grad_scale first (1/world for data parallel means).  `first` is read from *first_flag (device int32),
 * which is cleared afterwards. */
int ep24_sgd_nesterov(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float grad_scale,
                      int32_t* first_flag, void* stream);
/* The same update with its hyper-parameters read from DEVICE memory, hp[8] = {lr, momentum, grad_scale, ema decay d,
 * 1 - d, ...}: a captured step follows an LRScheduler (utils/lr_scheduler.py:33-34) without being
 * re-captured.  ema (nullable, same layout as p) receives ModelEMA.update of the freshly written parameters in the
 * same pass: ema = ema*d + (1-d)*p, each product and the sum rounded to fp32 (utils/ema.py:47-60). */
int ep24_sgd_nesterov_hp(float* p, const float* g, float* buf, int64_t n, const float* hp, int32_t* first_flag, float* ema,
                         void* stream);
/* The same update restricted to elements [first, first + n) (first % 4 == 0): parameters whose gradients are complete are
 * updated while the tail of backward still produces the rest.  last != 0 on the call that finishes the step (it clears
 * first_flag); ema, if given, is the EMA copy's flat buffer (same layout). */
int ep24_sgd_nesterov_hp_range(float* p, const float* g, float* buf, int64_t first, int64_t n, const float* hp,
                               int32_t* first_flag, float* ema, int last, void* stream);
/* ... and the packed bf16 FORWARD copy of the conv weights kept current by the same pass (round 5; ABI 3): the flat buffer holds a
 * conv weight as [Cout][kh][kw][Cin], which for Cin % 8 == 0 is the layout of its packed copy, and segments start at multiples of 64
 * elements; wf_delta[e >> 6] = (offset of element e's segment in wf) - (its offset in the flat buffer), INT32_MIN for groups without
 * such a copy (those still go through ep24_pack_weights_batched).  The step no longer re-reads the masters to pack them. */
int ep24_sgd_nesterov_hp_range_pack(float* p, const float* g, float* buf, int64_t first, int64_t n, const float* hp,
                                    int32_t* first_flag, float* ema, int last, const int32_t* wf_delta, void* wf, void* stream);
/* ModelEMA.update over one flat buffer (parameters, or the BatchNorm running statistics); hp non-null overrides
 * decay / one_minus_decay with hp[3] / hp[4]. */
int ep24_ema_update(float* ema, const float* src, int64_t n, float decay, float one_minus_decay, const float* hp,
                    void* stream);
/* writes hp[0..4] on the stream (by-value arguments: no host buffer has to outlive the call). */
int ep24_set_hparams(float* hp, float lr, float momentum, float grad_scale, float ema_decay, float one_minus_decay,
                     void* stream);
/* Weight decay by parameter group (torch.optim.SGD(momentum, nesterov=True, weight_decay), dampening 0), in the same one pass.
 * decay_grp has one byte per 64 elements of the WHOLE flat buffer, indexed (first + i) >> 6 exactly as wf_delta is: non-zero = the
 * group decays (segments start at multiples of 64 elements, so a group lies in one segment).  Per element, every product and sum
 * rounded to fp32 on its own, the gradient scaled first:
 *     gs = g * grad_scale;   d = decays ? gs + weight_decay * p : gs;   b' = first ? d : m*b + d;   p' = p - lr*(d + m*b')
 * (the decay product is not formed for a group that does not decay: those elements get the bits of the entry points above).  The
 * EMA and the packed forward copy are made from p' as before.  A null decay_grp is EP24_E_ARG.
 * ep24_set_hparams_decay writes hp[0..5], hp[5] = weight_decay; ep24_sgd_nesterov_decay is the by-value form (whole buffer, clears
 * first_flag); ep24_sgd_nesterov_decay_hp_range_pack reads hp[0..5] and takes nullable ema and nullable wf_delta / wf (both or
 * neither), so it stands for the _hp, _hp_range and _hp_range_pack forms. */
int ep24_set_hparams_decay(float* hp, float lr, float momentum, float grad_scale, float ema_decay, float one_minus_decay,
                           float weight_decay, void* stream);
int ep24_sgd_nesterov_decay(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float grad_scale,
                            float weight_decay, const uint8_t* decay_grp, int32_t* first_flag, void* stream);
int ep24_sgd_nesterov_decay_hp_range_pack(float* p, const float* g, float* buf, int64_t first, int64_t n, const float* hp,
                                          int32_t* first_flag, float* ema, int last, const int32_t* wf_delta, void* wf,
                                          const uint8_t* decay_grp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a13  fisheye sector warp (yolox/demo_featuremap.py:244-328)
 * ------------------------------------------------------------------------------------------------ */
/* The host mirror computes the 1-D tables exactly as the reference does (np.linspace / np.cos / np.sin,
 * demo_featuremap.py:258-283) and the crop box; the O(13200*T) part runs here.
 * winner[y*canvas_w+x] = max over (angle a, radius r) pairs landing on canvas pixel (y,x) of a*T+r, i.e. the
 * LAST writer of the reference's fancy-index scatter (:295-298).  Caller initialises winner to -1.
 * cos_tab/sin_tab [n_ang] and rho [T] are device float64. */
int ep24_sector_map(const double* cos_tab, const double* sin_tab, int n_ang, const double* rho, int T, int canvas_w,
                    int canvas_h, int32_t* winner, void* stream);
/* Crop [y0:y0+out_h, x0:x0+out_w] of the canvas (:301-306): dst [out_h][out_w][3] uint8 gathered from
 * src [T][n_ang][3] through the winner map, `fill` where nothing landed (114 image / 0 mask).  If src_index
 * is non-null the flat source index (row*n_ang+col, -1 = fill) is written too. */
int ep24_sector_gather(const uint8_t* src, const int32_t* winner, int canvas_w, int y0, int x0, int out_h, int out_w,
                       int T, int n_ang, uint8_t* dst, int fill, int32_t* src_index, void* stream);
/* bounding box of the non-zero pixels of channel 0 (:309-326): box = {xmin,ymin,xmax,ymax}; caller initialises
 * it to {INT_MAX,INT_MAX,-1,-1}. */
int ep24_mask_bbox(const uint8_t* mask3, int out_h, int out_w, int32_t* box, void* stream);

/* uint8 HWC bilinear resize with OpenCV's INTER_LINEAR fixed-point arithmetic (cv2.resize(image, (13200, T)),
 * demo_featuremap.py:285).  src [sh][sw][3] -> dst [dh][dw][3]. */
int ep24_resize_linear_u8(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, void* stream);
/* gather + resize in one pass (no [T, n_ang] intermediate): dst[oy][ox] = bilinear sample of src at the texel the
 * winner map selects, with the arithmetic of ep24_resize_linear_u8 / ep24_sector_gather (bit-identical results). */
int ep24_sector_warp_u8(const uint8_t* src, int sh, int sw, const int32_t* winner, int canvas_w, int y0, int x0,
                        int out_h, int out_w, int T, int n_ang, uint8_t* dst, int fill, void* stream);

/* The continuous sector map: the scatter above with its truncations removed.  For an image h x w, angle Theta,
 * row count T, canvas width cw, crop origin (x0, y0) and N = 13200, a source point (u, v) in pixel-index coordinates (pixel i is
 * centred at i; u = x_norm * w, v = y_norm * h) goes to, all in double,
 *     dx = (u + 0.5) * (N / w) - 0.5               dy = (v + 0.5) * (T / h) - 0.5
 *     a  = (N - 1) - dx                            r  = (T - 1) - dy
 *     th = ((180 - Theta) / 2 + Theta * a / (N - 1)) * pi / 180
 *     rho = (1000 - T) + T * r / (T - 1)           c = rho * cos th,  s = rho * sin th
 *     X = c + cw / 2 - 1 - x0 - 0.5 * sign(c)      Y = 1000 - s - 1 - y0 + 0.5
 * The +-0.5 terms put the point at the centre of the pixel that the truncation toward zero selects.
 * points [m][2] and out [m][2] are device float64 (x, y); one thread per point; m == 0 is EP24_OK. */
int ep24_sector_points(const double* points, int m, double theta, int T, int h, int w, int canvas_w, int x0, int y0, double* out,
                       void* stream);
/* 24-point labels under the warp, two launches, no allocation, no synchronisation, no floating-point atomics.
 * rows [R][51] float64: the normalised label rows (class, cx, cy, 24 x (x, y)) of all images, concatenated.
 * geo [n][12] float64 per image: Theta, T, h, w, cw, x0, y0, h', w' (size of the warped image), r (letterbox scale), index of the
 *   image's first row in `rows`, number of its rows (the first max_labels are read).  rot [24][2] float64: cos / sin of k * 15 degrees.
 * Per row: (a) each of the 24 edges vertex k -> k + 1 is cut into 8 equal pieces in source pixel space and the 192 outline points
 * are mapped as above; (b) the centre is the midpoint of their bounding box if that lies inside the mapped outline (even-odd rule:
 * edge p -> q is crossed when (p.y > cy) != (q.y > cy) and the crossing's x is > cx), else the map of the old centre, and bit 0 of
 * the row's flag word is set; (c) each of the 24 rays from the centre takes its nearest intersection with the closed 192-edge
 * outline by the side-of-line rule of ep24_augment_labels (a ray that meets no edge stays at the centre) and the point is clamped
 * to [0, w'] x [0, h']; (d) centre and vertices are multiplied by r; (e) the row is dropped unless min(width, height) of the new
 * vertices is > 1.  out [n][max_labels][51] fp32: the survivors in input order, zero padded; out_count [n]; out_flags
 * [n][max_labels] int32 beside the output rows.  cand [n][max_labels][51] fp32 and keep [n][max_labels] int32 are scratch (they
 * need no initialisation).  n == 0 is EP24_OK; n <= 65535. */
int ep24_sector_labels(const double* rows, const double* geo, const double* rot, int n, int max_labels, float* cand, int32_t* keep,
                       float* out, int32_t* out_count, int32_t* out_flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a13b  fisheye lens model (Kannala-Brandt, the model of OpenCV's cv2.fisheye): images, points, labels by calibration
 * ------------------------------------------------------------------------------------------------ */
/* A lens is model[14] float64: pin = (fx, fy, cx, cy) of the pinhole frame, fish = (fx, fy, cx, cy) of the fisheye frame, k1..k4,
 * theta_max (half field of view in radians, 0 < theta_max < pi / 2) and thetad(theta_max).  Coordinates are pixel-index coordinates
 * (pixel i is centred at i, as for ep24_sector_points).  All map arithmetic is double, every operation rounded on its own, with
 *     P(t) = 1 + t (k1 + t (k2 + t (k3 + t k4)))      thetad(th) = th * P(th^2)
 * to_fisheye(u, v):   a = (u - cx_p) / fx_p, b = (v - cy_p) / fy_p, r = hypot(a, b);  th = min(atan r, theta_max);
 *                     s = r > 0 ? thetad(th) / r : 1;   (X, Y) = (fx_f * a * s + cx_f, fy_f * b * s + cy_f)
 * to_pinhole(X, Y):   x = (X - cx_f) / fx_f, y = (Y - cy_f) / fy_f, rd = hypot(x, y);  td = min(rd, thetad(theta_max));
 *                     th solves thetad(th) = td: Newton from th = td, a fixed 12 steps th -= (thetad(th) - td) / thetad'(th) with
 *                     thetad'(th) = 1 + t (3 k1 + t (5 k2 + t (7 k3 + t 9 k4))), t = th^2, clamped to [0, theta_max] after each;
 *                     s = rd > 0 ? tan th / rd : 1;   (u, v) = (fx_p * x * s + cx_p, fy_p * y * s + cy_p)
 *                     (the divisor is rd, as it is r above: inside the field rd = td, beyond it the point keeps its azimuth only)
 * A point beyond the field lands on the field's rim at the same azimuth; nothing is ever non-finite.  k = 0 is the equidistant
 * projection.  The host (ep24.lens.LensModel) refuses a model whose thetad is not increasing on [0, theta_max] or whose Newton
 * iteration does not reproduce th to 1e-14; the entry points below take the table as it is.
 * `direction`: 0 = distort (pinhole -> fisheye), 1 = undistort (fisheye -> pinhole).
 *
 * ep24_lens_points: points [m][2] and out [m][2] device float64 (x, y) through to_fisheye (0) or to_pinhole (1); `model` is a HOST
 * pointer, read during the call; one thread per point; m == 0 is EP24_OK. */
int ep24_lens_points(const double* points, int m, const double* model, int direction, double* out, void* stream);
/* Images, one launch per batch.  images: one packed uint8 buffer; desc [n][3] int64 = {byte offset, h, w} of every contiguous HWC
 * source (h, w < 2^26); table [n][18] float64 = {model[14], direction, dst_h, dst_w, byte offset of the image in `out`}.  Every
 * destination pixel (ox, oy) is mapped into the source frame with the OTHER direction's map (distort: (sx, sy) = to_pinhole(ox, oy),
 * undistort: to_fisheye).  It is SAMPLED when it lies inside the field (distort: hypot(x, y) <= thetad(theta_max); undistort:
 * atan r <= theta_max) and 0 <= sx <= w - 1 and 0 <= sy <= h - 1, else it takes `fill` (0..255) in every channel.  The sample is
 * bilinear in integers:  qx = floor(sx * 32 + 0.5), xa = qx >> 5, wx = qx & 31, xb = min(xa + 1, w - 1), the same for y, and
 *     v = ((32 - wx)(32 - wy) p[ya][xa] + wx (32 - wy) p[ya][xb] + (32 - wx) wy p[yb][xa] + wx wy p[yb][xb] + 512) >> 10.
 * ep24_lens_warp_u8 writes uint8 HWC images of any sizes into `out` at their offsets; max_pixels, the largest dst_h * dst_w of the
 * batch, sizes the grid only: (min(ceil(max_pixels / 256), 4096), n) workgroups that stride over the pixels of their image.
 * ep24_lens_preproc_u8 writes the network input, out [n][3][S_h][S_w] fp32 with the channel order kept and the values of the uint8
 * form; the destination of every image is S_h x S_w (the table's size and offset fields are not read); the same grid rule with
 * S_h * S_w pixels, which must stay below 2^31 - 2^20.  n == 0 is EP24_OK; n <= 65535. */
int ep24_lens_warp_u8(const uint8_t* images, const int64_t* desc, const double* table, int n, int64_t max_pixels, uint8_t* out,
                      int fill, void* stream);
int ep24_lens_preproc_u8(const uint8_t* images, const int64_t* desc, const double* table, int n, float* out, int S_h, int S_w,
                         int fill, void* stream);
/* 24-point labels under the lens map: the contract of ep24_sector_labels, steps (a) - (e), with the forward map of the image's
 * direction (distort: to_fisheye, undistort: to_pinhole) in place of the sector map.  geo [n][22] float64 per image: model[14],
 * direction, h, w (the source image: rows are normalised by them), h', w' (the destination: vertices are clamped to
 * [0, w'] x [0, h']), the scale that centre and vertices are multiplied by, index of the image's first row in `rows`, number of its
 * rows.  Everything else as for ep24_sector_labels. */
int ep24_lens_labels(const double* rows, const double* geo, const double* rot, int n, int max_labels, float* cand, int32_t* keep,
                     float* out, int32_t* out_count, int32_t* out_flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N3  inference path: eval-mode network + postprocess
 * ------------------------------------------------------------------------------------------------ */
/* BaseConv in eval mode (network_blocks.py:50-51 with BatchNorm2d.eval()): y = act(z*scale + shift) (+ residual),
 * scale = gamma / sqrt(running_var + eps), shift = beta - running_mean*scale.  C, ld_z, ld_y (and ld_res with a residual) are
 * multiples of 8, M > 0 and 8 <= C <= 8192: the kernel keeps scale and shift in 2*C*4 bytes of LDS, 64 KiB at the most.
 * Anything else is EP24_E_ARG before a launch. */
int ep24_bn_act_infer(const void* z, int64_t ld_z, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, void* y, int64_t ld_y, const void* residual, int64_t ld_res,
                      int64_t M, int C, float eps, int act, void* stream);
/* eval head (yolo_head_24p.py:190-191, 239-256): decode xy / radii in place and apply sigmoid to obj and class logits. */
int ep24_head_decode_eval(float* out, int B, int A, int a0, int H, int W, float stride, int ncols, void* stream);
/* BatchNorm folding for inference, all conv units in two launches: w' = w * gamma / sqrt(running_var + eps) (packed bf16
 * [Cout][T][Cin_pad]) and bias = beta - running_mean * scale.  flat = the fp32 parameter buffer, bstat = the running
 * statistics buffer; desc[n_seg][12] int64 = {master offset, packed offset, Cout, T, Cin, Cin_pad, gamma offset, beta offset
 * (flat), running-mean offset, running-var offset (bstat), bias offset, 0}; prefix / cprefix [n_seg+1] = element / channel
 * prefix sums; eps[n_seg].  Only the Cin real columns of a packed row are written.  n_seg, total = prefix[n_seg] and
 * total_channels = cprefix[n_seg] are all > 0 (EP24_E_ARG otherwise, before a launch). */
int ep24_fold_bn(const float* flat, const float* bstat, const int64_t* desc, const int64_t* prefix, const int64_t* cprefix,
                 const float* eps, int n_seg, int64_t total, int64_t total_channels, void* w_folded, float* bias, void* stream);
/* conv -> BN(running statistics) -> act (+ residual) of the eval-mode network as ONE launch: the conv over the folded weights
 * with y = act(acc + bias) + residual in its epilogue (act: 0 none, 1 SiLU, 2 ReLU; res nullable). */
int ep24_conv_fwd_infer_bf16(const void* x, int64_t ld_x, const void* w, const float* bias, int act, const void* res,
                             int64_t ld_res, void* y, int64_t ld_y, int B, int H, int W, int Cin, int Cout, int ksize,
                             int stride, void* stream);
/* postprocess (utils/boxes.py:29-99) in three launches.  prepare: per row best class (first maximum), class_conf,
 * score = obj*class_conf or -1 when below conf_thre, bounding rectangle of the 24 points (with the reference's
 * theta*cos(theta) factors, passed in as the host computes them).  nms: per image (one workgroup) candidates sorted by score (ties: lower row first), greedy
 * suppression of IoU > nms_thre within a class (torchvision batched_nms) or across classes (class_agnostic); keep
 * [B][A] receives the kept rows in order, keep_count[B] their number; sort_key / sort_idx / dead are [B][P] scratch,
 * P a power of two >= A.  gather: det[n][29] = (pred[:, :27], class_conf, class_pred) of one image's kept rows.
 * A NaN score is no candidate (NaN >= conf_thre is false: the row gets -1).  A NaN class score is never greater than the running
 * maximum, so it is passed over - except in class column 0, where the scan starts: a leading NaN stays, class 0 is reported
 * with class_conf = NaN and the row is no candidate.  The rectangle is fminf / fmaxf over the 24 points: a NaN point is left out.
 * sort_key / sort_idx / dead need no initialisation; keep beyond keep_count is not written. */
int ep24_post_prepare(const float* pred, int ncols, int num_classes, int64_t n_rows, float conf_thre,
                      const float* ray_factors /* [48]: theta_k*cos(theta_k), then theta_k*sin(theta_k) */, float* score,
                      float* conf, int32_t* cls, float* rect, void* stream);
int ep24_post_nms(const float* score, const int32_t* cls, const float* rect, int B, int A, float nms_thre,
                  int class_agnostic, float* sort_key, int32_t* sort_idx, uint8_t* dead, int32_t* keep,
                  int32_t* keep_count, int P, void* stream);
int ep24_post_gather(const float* pred, int ncols, const float* conf, const int32_t* cls, const int32_t* keep, int n,
                     float* det, void* stream);
/* Polygon NMS (csrc/polynms.hip): ep24_post_nms with the rectangle IoU replaced by the exact area IoU of
 * the detections' own 24 points.  pred[B][A][ncols], score[B][A] and cls[B][A] are ep24_post_prepare's input and outputs.
 *   Candidates and order are ep24_post_nms's: the rows with score >= 0 (obj * class_conf >= conf_thre), score descending, ties to
 *   the lower row index; only the K best of an image enter (1 <= K <= A; K = A is exact greedy NMS over every candidate, a smaller
 *   K drops the others: the usual nms_pre).  Candidate j is removed by a kept, better-placed candidate i iff the classes agree
 *   (or class_agnostic) and poly24_iou(a = P_i, b = P_j) > (double)nms_thre, with P's vertices x_k = cx + r_k * ray_cs[k],
 *   y_k = cy + r_k * ray_cs[24 + k] (product and sum separate fp32 operations, as ep24_eval_iou forms a detection's) and
 *   poly24_iou the function of csrc/poly24.h that ep24_eval_iou calls (iou_type 2), one lane per pair: the same bits.  A NaN IoU
 *   never suppresses: a row with a NaN coordinate is kept and removes nobody.  Pairs whose vertex boxes do not overlap have IoU
 *   exactly 0.0, so they are never evaluated; that is exact for nms_thre >= 0, and a negative (or NaN) nms_thre is EP24_E_ARG.
 *   Four launches, no host synchronisation: sort (sort_key / sort_idx [B][P], P a power of two >= A; n_cand[B] = min(candidates,
 *   K)), geometry of the sorted candidates (verts [B][K][48], vbox [B][K][4] = min / max of the vertices, vcls [B][K]), the
 *   suppression matrix mask [B][K][ceil(K / 64)] uint64 (bit j & 63 of word j >> 6 of row i set iff j > i, j < n_cand, class rule,
 *   IoU test; every word the scan reads - rows < n_cand, words from the row's diagonal word to ceil(n_cand / 64) - 1 - is written
 *   by the call, whatever the buffers held) and the scan (one workgroup per image).  keep [B][A] / keep_count [B] as ep24_post_nms
 *   writes them.  EP24_E_ARG for a null pointer, K < 1, K > A or a bad P; EP24_E_UNSUPPORTED for K > 65536. */
int ep24_post_nms_poly24(const float* pred, int ncols, const float* score, const int32_t* cls, int B, int A, int K,
                         float nms_thre, int class_agnostic, const float* ray_cs, float* sort_key, int32_t* sort_idx, int P,
                         int32_t* n_cand, float* verts, float* vbox, int32_t* vcls, uint64_t* mask, int32_t* keep,
                         int32_t* keep_count, void* stream);
/* Polygon voting (csrc/tta.hip; DESIGN.md section 7, "Test-time augmentation"): runs after ep24_post_nms_poly24 on the buffers
 * that call leaves behind (sort_idx, n_cand, verts, vbox, vcls, keep, keep_count; same B, A, K, P, pred, score) and
 * replaces every kept detection by the score-weighted consensus of its voters.  voted [B][A][26] fp32: row m of image b belongs
 * to keep[b][m]; rows at and beyond keep_count[b] are not written.  n_voters [B][A] int32 likewise.
 *   Voters of the kept sorted row i: every sorted candidate j < n_cand[b], ranked before or after i, with the same class (unless
 *   class_agnostic) and poly24_iou(a = P_i, b = P_j) > (double)vote_thre - ep24_eval_iou's orientation with the kept row as the
 *   GT side - and i itself, always.  Pairs whose fp32 vertex boxes do not overlap have IoU exactly 0.0 and are not evaluated: exact
 *   for vote_thre >= 0; a negative (or NaN) vote_thre is EP24_E_ARG.  A NaN IoU never votes.
 *   One voter, or voters whose scores sum to 0: the 26 values of the kept row, bit for bit.  Otherwise, all in double with
 *   w_j = score[b][row_j]: C = sum w_j c_j / sum w_j over the voters' centres (pred columns 0, 1); for ray k, t_jk = the nearest
 *   crossing t >= 0 of C + t * (cos, sin)(15 deg * k) - the direction in double - with the closed polygon verts_j by the side-of-line rule of
 *   ep24_augment_labels (an edge counts iff its ends' side values have opposite signs or are zero; one side value per vertex;
 *   an edge on the line gives its ends), a voter without a crossing abstains on that ray, r_k = sum w_j t_jk / sum w_j over the
 *   others, and the kept row's own r_k when that weight is not positive.  C and r_k are rounded once to fp32.  Every sum has a
 *   fixed order; no floating-point atomics.  The grid follows from B and K alone; no host synchronisation.
 *   EP24_E_ARG / EP24_E_UNSUPPORTED as ep24_post_nms_poly24. */
int ep24_post_vote_poly24(const float* pred, int ncols, const float* score, int B, int A, int K, float vote_thre,
                          int class_agnostic, const int32_t* sort_idx, int P, const int32_t* n_cand,
                          const float* verts, const float* vbox, const int32_t* vcls, const int32_t* keep,
                          const int32_t* keep_count, float* voted, int32_t* n_voters, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T1  tracking: identity of 24-point detections across frames (csrc/track.hip; ep24.track; DESIGN.md section 7, "Tracking").
 *     S streams, T track slots per stream, N detection rows per stream.  A frame is ep24_track_cost, then ep24_track_step: two
 *     launches whose grids follow from S, T and N alone, no host synchronisation, no floating-point atomics.
 *   State, owned by the caller; a tracker starts from all-zero tables with hdr[s][0] = 1:
 *     trk_f [S][T][32] fp32: 0..25 shape (cx, cy, r_0..r_23), 26, 27 velocity (vx, vy), 28 score, 29..31 zero.
 *     trk_i [S][T][8] int32: 0 id (0 = free slot: all of its words in both tables are zero), 1 class, 2 status (1 tentative,
 *       2 confirmed, 3 lost), 3 hits, 4 age (frames since the last match), 5 frame of birth (the frame counter after that step:
 *       the first frame is 1), 6 detection row of the last match or -1, 7 zero.
 *     hdr [S][4] int32: next id (ids are never reused), frame counter, spawns dropped so far because the table was full, live slots.
 *   Input: det [S][N][ncols] fp32, ncols >= 29, postprocess's rows (cx, cy, 24 radii, obj_conf, class_conf, class); count [S]:
 *     rows at and beyond count[s] are ignored and not read.  score = the single fp32 product det[26] * det[27]; class = (int)det[28].
 *     A row is eligible iff d < count[s] and score >= low_thre (a NaN score is not).
 * ep24_track_cost writes every word of iou [S][T][N] double and dscore [S][N] fp32 (the score of an eligible row, NaN otherwise).
 *     The predicted polygon of a live slot: centre p = (cx + vx, cy + vy), one fp32 add each, radii unchanged, vertices
 *     p + r_k * ray_cs (cos in ray_cs[k], sin in ray_cs[24 + k]; product and sum separate fp32 operations, as ep24_post_nms_poly24
 *     forms them); a row's polygon likewise from its own 26 values.  iou[s][t][d] = poly24_iou(a = predicted polygon of slot t,
 *     b = polygon of row d) of csrc/poly24.h when the slot is live, the row eligible and the classes agree (or class_agnostic);
 *     0.0 otherwise.  Pairs whose fp32 vertex boxes do not overlap with positive width and height have IoU exactly 0.0 and are not
 *     evaluated; a pair with a NaN vertex on either side is evaluated, and its NaN is stored as it is (it never matches).
 *     EP24_E_ARG: a null pointer, S, T or N < 1, ncols < 29, low_thre not finite.  EP24_E_UNSUPPORTED: T not a multiple of 64 or
 *     above 1024, N above 4096, S above 65535.
 * ep24_track_step, one workgroup per stream, on the iou and dscore the cost call left (same det, S, T, N):
 *   Stage 1: the live slots against the eligible rows with score >= high_thre; a pair is admissible iff iou > (double)match_thre.
 *   Stage 2: the slots stage 1 left unmatched that were confirmed with age 0 before the step, against the eligible rows with
 *     score < high_thre; admissible iff iou > (double)match_low_thre.
 *   Either stage matches greedily by the strict total order (iou descending, slot ascending, row ascending): take the first
 *     admissible pair, remove its slot and its row, repeat.  (Computed as rounds of mutual best - every unmatched slot takes its
 *     best admissible unmatched row, ties to the lower row; every row its best slot, ties to the lower slot; mutual choices are
 *     matched - which gives the same set; the number of rounds depends on the data, nothing else of the launch does.)  A NaN iou
 *     is never admissible.
 *   Matched slot, row z, with p the predicted centre and e = z_c - p: c = p + alpha * e; v = v + beta * e;
 *     r_k = r_k + gamma * (z_k - r_k); every operation a separate fp32 one.  score = the row's; the class stays; hits += 1;
 *     age = 0; word 6 = the row; a tentative slot becomes confirmed when hits >= min_hits, a lost slot becomes confirmed.
 *   Unmatched live slot: a tentative one is freed; any other gets age += 1 and is freed when age > max_age, else its status
 *     becomes lost, c = p (it coasts), v stays, word 6 = -1.
 *   Spawns: the rows of stage 1 left unmatched with score >= new_thre, in ascending row order; the k-th of them takes the k-th
 *     free slot in ascending slot order, the slots freed in this step included: the row's 26 shape values bit for bit, v = 0,
 *     score, class, hits = 1, age = 0, id = next id + k, status tentative when min_hits > 1, else confirmed, birth = this frame,
 *     word 6 = the row.  A row without a free slot adds 1 to the dropped counter and takes no id.
 *   hdr: next id += spawns placed; frame counter += 1; dropped; live slots after the step.
 *   Outputs, every word written: det_track [S][N] int32 = the id matched to or spawned from row d, else 0.  out_f [S][T][29],
 *     out_i [S][T][4]: one row per slot that is confirmed with age 0 after the step, in ascending slot order - out_f = the 26
 *     filtered values, then columns 26..28 of the matched (or spawning) row; out_i = id, row, hits, slot; the rows after them are
 *     zero.  out_count [S] = their number.
 *   EP24_E_ARG: a null pointer, S, T or N < 1, ncols < 29, a threshold that is not finite, match_thre or match_low_thre < 0 (the
 *     box pre-test is exact from 0), a gain outside [0, 1], min_hits < 1, max_age < 0.  EP24_E_UNSUPPORTED: T not a multiple of 64
 *     or above 1024, N above 4096.
 * ------------------------------------------------------------------------------------------------ */
int ep24_track_cost(const float* det, int ncols, const int32_t* count, const float* trk_f, const int32_t* trk_i, int S, int T,
                    int N, float low_thre, int class_agnostic, const float* ray_cs, double* iou, float* dscore, void* stream);
int ep24_track_step(const float* det, int ncols, const double* iou, const float* dscore, float* trk_f, int32_t* trk_i,
                    int32_t* hdr, int S, int T, int N, float high_thre, float new_thre, float match_thre, float match_low_thre,
                    float alpha, float beta, float gamma, int max_age, int min_hits, int32_t* det_track, float* out_f,
                    int32_t* out_i, int32_t* out_count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E1  evaluation: COCO-style AP of 24-point detections (pycocotools evaluateImg + accumulate, area "all", no crowd /
 *     ignore, one maxDets; csrc/evaluate.hip, the match kernel in csrc/evalgeom.h).  iou_type 0 = circle24 (mean over the 24 rays of the ray circles' IoU,
 *     fp32), 1 = rect (axis-aligned boxes, float64), 2 = poly24 (exact area IoU of the two 24-gons, float64: GT vertices
 *     against c + r_k * (cos, sin)(15 deg * k) formed in fp32; csrc/poly24.h).  ray_cs[48] = cos(15 deg * k), then
 *     sin(15 deg * k), fp32.
 * ------------------------------------------------------------------------------------------------ */
/* out[G][D] double = IoU of gt50[G][50] (centre + 24 vertices, label columns 1..50) against det26[D][26] (centre + 24 radii). */
int ep24_eval_iou(const float* gt50, const float* det26, int G, int D, int iou_type, const float* ray_cs, double* out,
                  void* stream);
/* One workgroup per image b of labels[B][L][51] (L <= 256; the first n rows, n = rows whose sum is > 0).  Detection r < count[b]
 * of image b is row row_off[b] + a of rows[.][ncols], a = keep[b * keep_stride + r] (keep nullable: a = r); class_conf / class
 * from conf / cls at that row index (post_prepare's arrays) or, both null, from the row's columns 27 / 28 (postprocess rows).
 * score = row[26] * class_conf.  Per (image, class) the first max_dets (<= 128) detections in (score desc, r asc) order are
 * matched greedily at the 10 thresholds iou_thr[10] (double, compared against min(t, 1 - 1e-10); equal IoUs go to the later GT
 * row); each appends one record at an offset taken from *rec_count: rec_key = (~ordered score bits) << 32 | (seq_base + b) << 7
 * | rank, rec_cls, rec_p = r, rec_tp = 10-bit TP mask.  npig[num_classes] += the GTs per class.  sort_scratch [B][P] int64
 * (P a power of two >= every count, <= 65536); *err |= 1 if a count exceeds P.  num_classes < 65535, seq_base + B <= 2^25. */
int ep24_eval_match(const float* labels, int L, int B, const float* rows, int ncols, const int64_t* row_off,
                    const int32_t* keep, int64_t keep_stride, const int32_t* count, const float* conf, const int32_t* cls,
                    int num_classes, int iou_type, const float* ray_cs, const double* iou_thr, int max_dets,
                    int64_t seq_base, int64_t* sort_scratch, int P, int64_t* rec_key, int32_t* rec_cls, int32_t* rec_p,
                    int32_t* rec_tp, int32_t* rec_count, int32_t* npig, int32_t* err, void* stream);
/* Stable LSD radix sort of n records by (class, key): order[n] = record indices in that order.  Passes of 8 bits over the
 * key's low key_low_bits bits, its high 32 bits and the class's low cls_bits bits.  Scratch: key_tmp [2][n], cls_tmp [2][n],
 * idx_tmp [2][n], hist [256 * ceil(n / 4096)]. */
int ep24_eval_sort(const int64_t* key, const int32_t* cls, int64_t n, int key_low_bits, int cls_bits, int64_t* key_tmp,
                   int32_t* cls_tmp, int32_t* idx_tmp, int32_t* hist, int32_t* order, void* stream);
/* One workgroup per class over the sorted records: precision[10][101][num_classes] and recall[10][num_classes] (double) as
 * pycocotools accumulate computes them, -1 for a class without GTs.  The kernel is ep24_segm_accumulate's (E6) with one area
 * range, one maxDets, no ignore bits and no position filter; each workgroup finds its class's records in the sorted order by
 * binary search.  rec_thr[101] double; ctp_scratch [n] int32, env_scratch [n] double.  cls_range: unused since the two accumulate
 * kernels became one; may be null; neither read nor written. */
int ep24_eval_accumulate(const int32_t* order, const int32_t* rec_cls, const int32_t* rec_tp, int64_t n, const int32_t* npig,
                         int num_classes, const double* rec_thr, int64_t* cls_range, int32_t* ctp_scratch,
                         double* env_scratch, double* precision, double* recall, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E2  instance masks of 24-point polygons (csrc/mask.hip).  As everywhere in this header: raw device
 *     pointers, sizes and a stream; the caller owns every buffer, nothing allocates, frees or synchronises.
 *     Packed masks are uint32 [N][H][WW], WW = ceil(W / 32): pixel x is bit x & 31 of word x >> 5, bits at x >= W are zero.
 *     bbox [N][4] int32 = (x0, y0, x1, y1), the smallest and largest set pixel, or (W, H, -1, -1) for an empty mask;
 *     area [N] int32 = the number of set pixels.  H * W < 2^31.
 * ------------------------------------------------------------------------------------------------ */
/* verts[n][24][2] fp32 from rows det[n][ncols] = (cx, cy, 24 radii, ...): x_k = cx / ratio + (r_k / ratio) * ray_cs[k],
 * y_k = cy / ratio + (r_k / ratio) * ray_cs[24 + k], every operation a separate fp32 one (ratio = 1 leaves the rows as they are;
 * the letterbox ratio maps them back to the original image). */
int ep24_poly24_vertices(const float* det, int ncols, int n, const float* ray_cs, float ratio, float* verts, void* stream);
/* Rasterise verts[N][24][2] (already in the pixel coordinates of the H x W canvas).  The centre of pixel (x, y) is the point
 * (x, y).  In double, for row yc = y the edge (x0, y0) -> (x1, y1) counts iff (y0 <= yc) != (y1 <= yc), crosses at
 * xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0), and pixel x is set iff an odd number of counting edges have x < xc.  Every word
 * of bits, bbox and area is written by the call itself (no memset needed); the statistics use integer atomics only. */
int ep24_poly24_raster(const float* verts, int N, int H, int W, uint32_t* bits, int32_t* bbox, int32_t* area, void* stream);
/* masks uint8 [N][H][W] (non-zero = set) -> packed bits with bbox and area, and back (0 / 1). */
int ep24_mask_pack_u8(const uint8_t* masks, int N, int H, int W, uint32_t* bits, int32_t* bbox, int32_t* area, void* stream);
int ep24_mask_unpack_u8(const uint32_t* bits, int N, int H, int W, uint8_t* masks, void* stream);
/* inter[G][D] int64 = popcount(A_g & B_d) over the rows and words of the two boxes' overlap (a pair with disjoint boxes reads
 * no mask word); iou[G][D] double = inter / (a_area + b_area - inter), 0 when that union is 0.  Integer sums only. */
int ep24_mask_iou(const uint32_t* a_bits, const int32_t* a_bbox, const int32_t* a_area, int G, const uint32_t* b_bits,
                  const int32_t* b_bbox, const int32_t* b_area, int D, int H, int W, int64_t* inter, double* iou, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E3  drawing 24-point detections onto an image (csrc/draw.hip; ep24.draw.draw_detections).  The reference's
 *     Evaluator.vis (show_24p.py:325-367) draws, in the class colour, a filled centre dot of radius 4, a dot of radius 2 on each of
 *     the 24 points, the closed 24-gon with lines of thickness 2 and the class name next to the centre, after bboxes /= ratio,
 *     truncation of centre and radii to int and clipping of each vertex to [0, W] x [0, H].  That integer geometry is kept; the pixel
 *     rules are this library's own and exact (cv2's Bresenham lines and Hershey text cannot be reproduced without cv2: the deviation).
 *     Image uint8 [H][W][3], contiguous, channel order left alone, 1 <= H, W <= EP24_DRAW_MAX_SIDE; the centre of pixel (x, y) is the
 *     point (x, y).  det [n][29] = the rows of postprocess (cx, cy, 24 radii, obj, class_conf, class), n >= 0.
 *   Row geometry (fp32, every operation separate, then truncation toward zero): xc = (int)(cx / ratio), yc = (int)(cy / ratio),
 *     r_k = (int)(rad_k / ratio), vx_k = (int)min(max((float)xc + (float)r_k * cs[k], 0), (float)W), vy_k the same with cs[24 + k]
 *     and H; cs = ray_cs[48] (cos, then sin of 15 deg * k, fp32); score = obj * class_conf (fp32); cls = (int)col28.
 *   A row is skipped (draws nothing) if !(score >= conf), or any of cx / ratio, cy / ratio, rad_k / ratio is non-finite or has
 *     magnitude >= 2^20, or cls is not in [0, num_classes).
 *   Solid coverage of pixel X = (x, y) by a row, all in int64 - any of:
 *     centre disc   (x - xc)^2 + (y - yc)^2 <= 16;
 *     vertex discs  (x - vx_k)^2 + (y - vy_k)^2 <= 4 for some k;
 *     edges         for each k, P = v_k, Q = v_((k + 1) mod 24), d = Q - P, w = X - P, L2 = d.d, t = w.d:  t <= 0: w.w <= 1;
 *                   t >= L2: |X - Q|^2 <= 1;  else (d.x * w.y - d.y * w.x)^2 <= L2  (squared distance to the segment <= 1; P = Q too);
 *     text          label bytes b_0 .. b_(m-1): the class's entry of labels [num_classes][24] (label_len [num_classes], 0..24),
 *                   followed when show_scores is set by a space and the two decimal digits of min(99, (int)(score * 100.0f)) (never
 *                   below 0; bytes past 24 are dropped).  Origin tx = xc + 3, ty = yc - 3 - 7 s, s = font_scale; with u = x - tx,
 *                   v = y - ty the pixel is covered iff 0 <= v < 7 s, 0 <= u < 6 s m, cu = (u mod 6 s) div s < 5 and bit 4 - cu of
 *                   font[b_j - 32][v div s] is set, j = u div 6 s.  font uint8 [95][7]: bytes 32..126, 7 rows of 5 bits, MSB
 *                   leftmost; a byte outside 32..126 draws as '?'.
 *   Fill coverage (only with fill_alpha > 0): the pixel is inside the integer polygon by ep24_poly24_raster's rule - in double, an
 *     edge counts iff (y0 <= y) != (y1 <= y), crosses at x0 + ((y - y0) * (x1 - x0)) / (y1 - y0), inside iff an odd number of counting
 *     edges have x < that crossing.
 *   Painter's order: rows in row order (postprocess's NMS order); for each row not skipped: solid-covered -> pix = colors[cls];
 *     else fill-covered -> per channel pix = (pix * (256 - a) + color * a + 128) >> 8, a = fill_alpha in 0..255.  A pixel that no row
 *     covers keeps its byte (and is not written).  The result is a bit-exact function of the inputs.
 * ------------------------------------------------------------------------------------------------ */
#define EP24_DRAW_REC_WORDS 64        /* int32 words of one primitive record */
#define EP24_DRAW_MAX_SIDE 16384
#define EP24_DRAW_MAX_FONT_SCALE 1024
/* One thread per row -> rec [n][EP24_DRAW_REC_WORDS] int32: [0] skip flag, [1] xc, [2] yc, [3..50] the 24 vertices (x, y), [51] colour
 * (c0 | c1 << 8 | c2 << 16), [52] m, [53..58] the 24 label bytes (zero past m), [59..62] the row's pixel box (x0, y0, x1, y1, inclusive;
 * over discs, edges and text, which also holds the fill; (0, 0, -1, -1) for a skipped row), [63] 0.  Every word of every record is
 * written by the launch, whatever the buffer held.  colors uint8 [num_classes][3].  EP24_E_ARG: n < 0, num_classes < 1, ratio not a
 * positive finite number, NaN conf, a null pointer with n > 0; EP24_E_UNSUPPORTED: H, W or font_scale outside their ranges. */
int ep24_draw24_prepare(const float* det, int n, float ratio, float conf, const float* ray_cs, int H, int W, const uint8_t* colors,
                        int num_classes, const uint8_t* labels, const int32_t* label_len, int font_scale, int show_scores,
                        int32_t* rec, void* stream);
/* Paints the records onto image IN PLACE: one workgroup per 64 x 16 pixel tile, every pixel read and written by exactly one thread,
 * no atomics; the records are tested against the tile 256 at a time in row order (no cap on n), and a tile that no record's box
 * touches writes nothing.  fill_alpha outside 0..255 is EP24_E_ARG. */
int ep24_draw24_paint(uint8_t* image, int H, int W, const int32_t* rec, int n, const uint8_t* font, int fill_alpha, int font_scale,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * E4  feature-map response (csrc/featmap.hip; ep24.featmap).  The reference's title experiment
 *     (yolox/demo_featuremap.py:330-392): the channel mean of each neck output as a heat map, and the mean of that map inside the
 *     ground-truth region.  No allocation, no stream synchronisation, no floating-point atomics: every result is a bit-exact
 *     function of the inputs.  All fp32 steps are separate operations (no contraction), all index arithmetic is 64-bit.
 * ------------------------------------------------------------------------------------------------ */
#define EP24_FEATMAP_MAX_SCALE 64
/* out[r] = (sum of x[r * ld + c], c in [0, C)) / (float)C for M bf16 rows: a channel slice of an NHWC activation buffer with
 * M = B * H * W (fpn_np.sum(axis=0) / fpn_channel, :345).  The sum is fp32, the division a true division.  A row's result depends on
 * that row's C values only - not on M, the grid or its neighbours - and the summation order is a fixed function of C: G = the power
 * of two >= C / 8 (at most 64) lanes share a row, lane g adds the values of the 16-byte chunks g, g + G, ... one by one in index order
 * starting from 0.0f, and the G partial sums meet in a butterfly (partner distance G / 2, ..., 1).  Requirements: C % 8 == 0,
 * C >= 8, ld % 8 == 0, ld >= C, x 16-byte aligned - anything else is EP24_E_UNSUPPORTED; M < 0, or a null pointer with M > 0, is
 * EP24_E_ARG; M = 0 launches nothing. */
int ep24_featmap_mean_bf16(const void* x, int64_t ld, int64_t M, int C, float* out, void* stream);
/* range[n] = (min, max) over the `cells` values of map n (maps fp32 [N][cells]): fminf / fmaxf from (+inf, -inf), so NaNs are
 * ignored and an empty or all-NaN map gives (+inf, -inf).  One workgroup per map.  EP24_E_ARG: N < 0, cells < 0, a null pointer. */
int ep24_featmap_range(const float* maps, int N, int64_t cells, float* range, void* stream);
/* Heat map: out uint8 [N][H * scale][W * scale][3], pixel (Y, X) takes cell (Y / scale, X / scale) of maps fp32 [N][H][W].  Colour
 * index in fp32 with (lo, hi) = range[n]: t = (v - lo) / (hi - lo), q = t * 256.0f; idx = 0 if !(hi > lo) or !(q >= 0), 255 if
 * q >= 255, else (int)q; the colour is lut[idx] of a uint8 [256][3] table.  base == NULL: the pixel is the colour.  Otherwise base is
 * fp32 [N][3][H * scale][W * scale] (the network input: planar, 0 - 255), its byte is 0 if !(b >= 0), 255 if b >= 255, else (int)b,
 * and per channel out = (byte * (256 - alpha) + colour * alpha + 128) >> 8 - the fill expression of ep24_draw24_paint.  Plane ch of
 * base, column ch of lut and channel ch of out belong together.  Every byte of out is written.  EP24_E_ARG: N < 0, alpha outside
 * 0..255, a null maps / range / lut / out with N > 0; EP24_E_UNSUPPORTED: scale outside 1..EP24_FEATMAP_MAX_SCALE, H or W < 1, or
 * an output side above EP24_DRAW_MAX_SIDE. */
int ep24_featmap_render(const float* maps, int N, int H, int W, int scale, const float* range, const uint8_t* lut, const float* base,
                        int alpha, uint8_t* out, void* stream);
/* Response of maps fp32 [B][H][W] inside the regions of labels fp32 [B][L][51] (class, centre, 24 x (x, y) in pixels of the network
 * input): sum[b][l] = the double-precision sum of the region's cells (a fixed order), count[b][l] their number, mean = sum / count,
 * or 0 with count 0.  A row whose 51 values, added in fp32 in index order, do not come to more than 0 is padding; a row with a
 * non-finite vertex, or one of magnitude >= 2^20, has an empty region: count, sum and mean are 0 for both.
 *   mode 0 "rect" (:378-385): the bounding rectangle of the 24 vertices; s = (float)stride, x0 = (int)(xmin / s), x1 = (int)(xmax / s),
 *     the same in y (fp32, truncation toward zero); the edges are clamped to [0, W] / [0, H] (the reference's slice would wrap a
 *     negative index) and the region is the half-open [y0, y1) x [x0, x1).
 *   mode 1 "poly24": cell (i, j) belongs iff the point ((j + 0.5) * stride, (i + 0.5) * stride) - the anchor centre of
 *     get_in_boxes_info - is inside the 24-gon by ep24_poly24_raster's crossing rule in double (csrc/raster_rule.h).
 * One workgroup per (image, row).  EP24_E_ARG: B or L < 0, stride < 1, another mode, a null pointer with B * L > 0;
 * EP24_E_UNSUPPORTED: H or W outside 1..EP24_DRAW_MAX_SIDE. */
int ep24_featmap_response(const float* maps, int B, int H, int W, int stride, const float* labels, int L, int mode, double* sum,
                          int32_t* count, double* mean, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N4  24-point label generation (yolox_24p/datasets/2+24_labels_create.py:61-116, :175-180)
 * ------------------------------------------------------------------------------------------------ */
/* rotation_for_24p for n objects (n <= 65535 per call).  masks: uint8 instance masks (non-zero = object) somewhere in
 * one device buffer; desc[n][6] int64 = {byte offset of the mask, H, W, L = int(sqrt(H^2 + W^2)), number of ray samples
 * = len(arange(0, L, 0.2)), row stride in bytes}; centre[n][2] double = box centre (x, y) as the reference forms it
 * (:167-168); rot[24][2] double = cos / sin of k*15 degrees as numpy computes them.  H + W + L must stay below 32768
 * (the reference holds the coordinates in int16).  Out: out_pts[n][24][2] int32 (x, y), out_r[n][24] double; a ray
 * without any candidate pixel (np.argmin of an empty array in the reference) gives (-1,-1) and +inf. */
int ep24_ray24(const uint8_t* masks, const int64_t* desc, const double* centre, const double* rot, int n,
               int32_t* out_pts, double* out_r, void* stream);
/* cv2.contourArea(cv2.convexHull(points)) of each object's 24 integer points (:175-176): area[n] double. */
int ep24_hull_area24(const int32_t* pts, int n, double* area, void* stream);

/* COCO segmentations -> the instance masks ep24_ray24 reads (pycocotools annToMask: rleFrPoly, rleMerge as a union, rleDecode),
 * csrc/cocomask.hip.  masks: one device buffer of `total` bytes, 4-byte aligned, total a multiple of 4, zeroed by the caller before
 * the first call; desc[n][6] as for ep24_ray24; every mask is uint8 0 / 1, row-major [H, W], at its byte offset.  No kernel writes
 * outside [0, total) or outside the mask its descriptor names.
 * ep24_cocomask_poly_xor: one round (at most 7 polygons of every annotation).  edges[ne][8] int32 = {xs, ys, xe, ye, annotation,
 *   bit 0..6 = the polygon's index within the annotation modulo 7, 1 on the first edge of its polygon, 0}, the vertices being
 *   (int)(5 * x + .5) / (int)(5 * y + .5) with the polygon closed; the edges of a polygon are adjacent and in its order, and edges[0]
 *   starts one.  start[ne + 1] int64 = running sum of max(|xe - xs|, |ye - ys|) + 1 (its first entry may be any base), npts =
 *   start[ne] - start[0].  Every dense point that is a boundary point of rleFrPoly flips its bit of mask byte [y][x].
 * ep24_cocomask_poly_scan: finishes a round.  items[n] int32 (n <= 65535) = annotation * 2 + (1 if this is the annotation's last
 *   round); every column's running XOR of bits 0..6, OR bit 7, goes back as 0 / 1 (last round) or into bit 7.  max_w = largest W.
 * ep24_cocomask_rle: runs[n][3] int64 (n <= 65535) = {annotation, first entry in ends, number of runs}; ends = inclusive prefix
 *   sums of each annotation's column-major run lengths (the first run is of zeros, runs may be empty); max_w = largest W. */
int ep24_cocomask_poly_xor(uint8_t* masks, int64_t total, const int64_t* desc, const int32_t* edges, const int64_t* start, int ne,
                           int64_t npts, void* stream);
int ep24_cocomask_poly_scan(uint8_t* masks, int64_t total, const int64_t* desc, const int32_t* items, int n, int max_w, void* stream);
int ep24_cocomask_rle(uint8_t* masks, int64_t total, const int64_t* desc, const int64_t* runs, const int64_t* ends, int n,
                      int max_w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E5  instance masks -> COCO run lengths (csrc/rle.hip; ep24.cocomask.encode).  pycocotools' rleEncode: the mask
 *     is walked column-major (p = x * H + y) from a previous value of 0, every change of value closes a run, the end closes the last;
 *     the first run is of zeros (0 when pixel (0, 0) is set), an all-zero mask is [H * W], an all-one mask [0, H * W].  Input: packed
 *     masks as in E2.  Integer work only, no atomics, every result a bit-exact function of the inputs; nothing allocates or synchronises.
 *   The batch is N masks of one size H x W behind each other (tab == NULL; column tables at n * W), or masks of their own sizes
 *     named by tab[N][4] int64 = {first uint32 word of the mask in bits, H, W, first entry of the mask in the column table}; then
 *     the H and W arguments are the largest of the table.  A table row with H or W <= 0 or H * W >= 2^31 is skipped (one run of 0).
 *   N < 0, H or W <= 0, H * W >= 2^31: EP24_E_UNSUPPORTED.  A null pointer with N > 0: EP24_E_ARG.  A grid axis over N is cut into
 *     launches of 65 535 inside the call.
 * ep24_rle_pack_bytes: the byte masks of ep24_ray24's buffer and desc[N][6] (non-zero = set) -> the packed rows tab names; H and W
 *   are tab's and must be desc's, max_h the largest H.  A mask that does not lie inside [0, total) is left unwritten.
 * ep24_rle_count: colcnt[mask's first entry + x] int32 = the transitions in column x (the pixel before (x, 0) is (x - 1, H - 1)).
 * ep24_rle_scan: colcnt -> per mask the exclusive prefix over its columns, in place; offsets[N + 1] int64 = the exclusive prefix
 *   of runs[n] = transitions + 1 over the masks, in index order.  N = 0 writes offsets[0] = 0.
 * ep24_rle_emit: ends[offsets[n] + j] int32 = the position of mask n's transition j, j < runs[n] - 1 (entry runs[n] - 1 is not
 *   written); cap = the entries ends can hold: nothing is written at or beyond it, or outside the mask's own range.
 * ep24_rle_counts: counts[i] int32, i < min(total, offsets[N]) = ends[i] - ends[i - 1], with 0 before a mask's first end and H * W
 *   as its last; counts and ends are different buffers.
 * ------------------------------------------------------------------------------------------------ */
int ep24_rle_pack_bytes(const uint8_t* masks, int64_t total, const int64_t* desc, const int64_t* tab, int N, int max_h,
                        uint32_t* bits, void* stream);
int ep24_rle_count(const uint32_t* bits, const int64_t* tab, int N, int H, int W, int32_t* colcnt, void* stream);
int ep24_rle_scan(int32_t* colcnt, const int64_t* tab, int N, int H, int W, int64_t* offsets, void* stream);
int ep24_rle_emit(const uint32_t* bits, const int64_t* tab, int N, int H, int W, const int32_t* colprefix, const int64_t* offsets,
                  int32_t* ends, int64_t cap, void* stream);
int ep24_rle_counts(const int32_t* ends, const int64_t* offsets, const int64_t* tab, int N, int H, int W, int64_t total,
                    int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E6  COCO "segm" evaluation on instance masks (csrc/segmeval.hip; ep24.segmeval.SegmEvaluator): pycocotools'
 *     rleIou, evaluateImg and accumulate with crowd GTs, ignore flags, area ranges and several maxDets.  Packed masks as in E2, named
 *     by tab[N][4] int64 = {first uint32 word of the mask in bits, H, W, unused} as for ep24_rle_count.  Nothing allocates, frees or
 *     synchronises; the only atomics are the integer sums into npig; every result is a bit-exact function of the inputs.
 * ep24_segm_mask_stats: bbox[N][4] and area[N] int32 with E2's meaning ((x0, y0, x1, y1) of the set pixels, (W, H, -1, -1) for an empty
 *   mask, the popcount).  Every output word is written; a table row with a negative first word, H or W <= 0 or H * W >= 2^31 reads no
 *   mask word and gives (0, 0, -1, -1) and 0.
 * ep24_segm_iou: grp[J][8] int64, one row per (image, category) = {H, W, first GT mask, G, first DT mask, D, first entry in iou, 0};
 *   mask indices point into tab, bbox, area (N rows) and gt_crowd (uint8 per mask, read for GT masks only).  The first entries must be
 *   the running sum of G * D over the rows (from any base) and pairs that sum: one wave per pair finds its row by a binary search.
 *   iou[first entry + d * G + g] double, detection-major as pycocotools holds it: with inter = popcount(GT_g & DT_d) over the rows and
 *   words where the two boxes overlap (disjoint boxes read no mask word), 0.0 if inter == 0, else inter / area(DT_d) for a crowd GT and
 *   inter / (area_g + area_d - inter) otherwise - one correctly rounded double division of exact integers (rleIou).  inter (nullable)
 *   int64 receives the counts at the same indices.  G == 0 or D == 0 writes nothing.  The masks of a group have the group's H and W:
 *   a pair whose table rows say otherwise is written as 0 without reading a mask word; a row that names masks outside [0, N) writes
 *   nothing.  More than 2^24 pairs are cut into several launches inside the call.
 * ep24_segm_match: one wave per row of mgrp[J][8] int64 = {first GT, G, first detection, D (<= 128), first entry in iou, class, image
 *   sequence number (< 2^25), 0}.  GT indices address gt_crowd, gt_ignore0 (uint8: the annotation's ignore OR iscrowd, the host's OR)
 *   gt_area (double: the annotation's area field) and scratch; detection indices address dt_area (double), dt_rank (int32: the dense
 *   rank of the score among the run's distinct scores, 0 = highest) and the records.  Detections stand in the order the host fixed
 *   (score descending, input order ascending).  For every area range a < NA <= 4 of area_rng[NA][2] double and every threshold t of
 *   iou_thr[10] double, evaluateImg: GT g is ignored iff ignore0 || gt_area < lo || gt_area > hi; the GTs are taken in a stable order
 *   with the non-ignored first; per detection, best = min(thr, 1 - 1e-10), a GT already matched at (a, t) is skipped unless it is
 *   crowd, the walk stops at the first ignored GT once a non-ignored match is held, a GT with iou >= best becomes the match (equal
 *   IoUs go to the later GT); a matched detection inherits the GT's ignore flag, an unmatched one is ignored iff dt_area lies outside
 *   the range.  Record n = the detection's index: rec_m[n][NA] int32 = 10 TP bits | 10 ignore bits << 16, rec_key[n] =
 *   dt_rank << 32 | sequence << 7 | position in the group, rec_cls[n] = class: ep24_eval_sort's ascending order of (class, key) is
 *   pycocotools' (class, score descending, image, position).  npig[num_classes][NA] int32 += the non-ignored GTs (the caller zeroes
 *   it once per evaluation).  Scratch: one int64 per GT of the call, indexed as gt_area is (only groups with G > 64 touch it; there
 *   is no other cap on G).  A row with D > 128, a negative count or index or a class outside [0, num_classes) is skipped.
 * ep24_segm_accumulate: over the n records in the order ep24_eval_sort gave, for every class k, area range a and max_dets[m] (int32
 *   [NM], NM <= 4): only records whose position is < max_dets[m] count, a record ignored at t is neither TP nor FP at t;
 *   precision[10][101][K][NA][NM] and recall[10][K][NA][NM] double with the expressions of ep24_eval_accumulate - tp / (fp + tp + eps),
 *   the envelope from the right, the left search over recall = tp / npig - and -1 where npig[k][a] == 0.  One kernel serves both entry points
 *   (csrc/accumulate.h); the records being ordered by class, each workgroup finds its class's range by binary search.  rec_thr[101]
 *   double; ctp_scratch [NA * NM][n] int32, env_scratch [NA * NM][n] double.  K <= 65535.  cls_range: unused since the two accumulate
 *   kernels became one; may be null; neither read nor written.
 * ------------------------------------------------------------------------------------------------ */
int ep24_segm_mask_stats(const uint32_t* bits, const int64_t* tab, int N, int32_t* bbox, int32_t* area, void* stream);
int ep24_segm_iou(const uint32_t* bits, const int64_t* tab, int N, const int32_t* bbox, const int32_t* area,
                  const uint8_t* gt_crowd, const int64_t* grp, int J, int64_t pairs, double* iou, int64_t* inter, void* stream);
int ep24_segm_match(const int64_t* mgrp, int J, const double* iou, const uint8_t* gt_crowd, const uint8_t* gt_ignore0,
                    const double* gt_area, const double* dt_area, const int32_t* dt_rank, const double* area_rng, int NA,
                    const double* iou_thr, int num_classes, int64_t* scratch, int32_t* rec_m, int64_t* rec_key, int32_t* rec_cls,
                    int32_t* npig, void* stream);
int ep24_segm_accumulate(const int32_t* order, const int64_t* rec_key, const int32_t* rec_cls, const int32_t* rec_m, int64_t n,
                         const int32_t* npig, int num_classes, int NA, const int32_t* max_dets, int NM, const double* rec_thr,
                         int64_t* cls_range, int32_t* ctp_scratch, double* env_scratch, double* precision, double* recall,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * E7  boundary bands for Boundary IoU (csrc/boundary.hip; ep24.masks.boundary, SegmEvaluator(iou_type="boundary")).
 *     For a mask M of an H x W image and a radius d >= 1: erode(M, d) sets pixel (x, y) iff every pixel (x', y') with |x' - x| <= d and
 *     |y' - y| <= d is set in M, pixels outside the image counting as not set (d iterations of a 3 x 3 erosion on the zero-framed mask);
 *     boundary(M, d) = M & ~erode(M, d).  Boundary IoU of a pair is min(rleIou of the masks, rleIou of their bands), the radius being
 *     max(1, round(0.02 * the image's diagonal)): the host's formula, never the object's size.  Packed masks as in E2.  Integer work
 *     only, no atomics, nothing allocates or synchronises; every result is a bit-exact function of the inputs.
 * ep24_mask_boundary: out = boundary(bits, d) at the same word offsets as bits.  tab == NULL: N masks of one size H x W behind each
 *   other, one radius d for all.  Otherwise tab[N][4] int64 = {first uint32 word of the mask in bits and out, H, W, d}; the H and W
 *   arguments are then the largest of the table and the d argument is ignored.  Every word of out that belongs to a valid mask is
 *   written by the call (no memset needed), the bits at x >= W as zero; nothing else is written.  d >= max(H, W) gives out == bits (the
 *   radius is clamped, not walked).  A table row with a negative first word, H or W <= 0, H * W >= 2^31 or d < 1 is skipped and writes
 *   nothing.  N < 0, H or W <= 0 (N > 0), H * W >= 2^31, d < 1 without a table: EP24_E_UNSUPPORTED.  A null bits or out with N > 0, or
 *   out == bits: EP24_E_ARG.  N == 0 writes nothing.  A grid axis over N is cut into launches of 65 535 inside the call.
 * ep24_segm_iou_min: iou[i] = other[i] < iou[i] ? other[i] : iou[i], i < n (finite, non-negative values; n == 0 is EP24_OK): the min of
 *   the two IoU tables of ep24_segm_iou, kept behind the ABI like every other piece of compute.
 * ------------------------------------------------------------------------------------------------ */
int ep24_mask_boundary(const uint32_t* bits, const int64_t* tab, int N, int H, int W, int d, uint32_t* out, void* stream);
int ep24_segm_iou_min(double* iou, const double* other, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E8  24-point evaluation by strata of object size and distortion zone (csrc/evalstrata.hip, csrc/evalgeom.h; DESIGN.md section 7;
 *     ep24.evaluate.Evaluator24(strata=...)).  E1's matcher with pycocotools' area-range semantics, the range widened to a stratum
 *     {area_lo, area_hi, z_lo, z_hi} (double): an object with area A and zone value z lies outside it iff A < area_lo || A > area_hi ||
 *     z < z_lo || z >= z_hi (area closed at both ends as pycocotools' ranges, zone half open so that zones partition).  At most 8 strata.
 *     Measures, both double, every operation rounded on its own:
 *       area = (0.5 * |sum over k = 0..23 of (x_k * y_{k+1} - x_{k+1} * y_k)|) / (s * s), the sum from 0.0 in that order over the
 *         object's 24 points converted from fp32 (a GT's: label columns 3..50; a detection's: c + r_k * (cos, sin)(15 deg * k), product
 *         and sum in fp32 as E1 forms them), s = scales[image] = input pixels per original pixel: areas in original-image pixels.
 *       zone from the centre (X, Y) (a GT's: label columns 1, 2; a detection's: row columns 0, 1) and the image's row of zt[B][16] =
 *         {kind, fx, fy, cx, cy, k1, k2, k3, k4, theta_max, thetad(theta_max), 0...}: x = (X - cx) / fx, y = (Y - cy) / fy,
 *         rd = sqrt(x * x + y * y) (a plain sqrt, not hypot).  kind 0: z = 0.  kind 1: z = rd.  kind 2: z = theta * (180 / pi) with theta
 *         the result of ep24_lens_points' 12 clamped Newton steps on td = fmin(rd, thetad(theta_max)), and z = +infinity where
 *         rd > thetad(theta_max).  Any other kind reads as 0.
 *     Nothing allocates, frees or synchronises; the only atomics are integer ones (npig, the append offset); every result is a bit-exact
 *     function of the inputs.
 * ep24_eval_measure: out[n][2] double = (area, zone) of rows[n][ncols] fp32, row_kind 0 = label rows (ncols >= 51), 1 = detection rows
 *   (ncols >= 26); image[n] int32 names every row's entry of scales[B] and zt[B][16]; an index outside [0, B) reads nothing and gives
 *   (NaN, NaN).  n == 0 is EP24_OK.  EP24_E_ARG: a row_kind other than 0 / 1, ncols too small, a null pointer with n > 0.
 * ep24_eval_match_strata: ep24_eval_match's arguments, meaning and limits, plus scales[B], zt[B][16] (device) and strata[NA][4] - a HOST
 *   array, read during the call.  Per image, class, stratum a and threshold t, evaluateImg without crowd: a GT is ignored iff it lies
 *   outside stratum a; the class's first max_dets detections go in (score desc, r asc) order; among the GTs not yet matched at (a, t)
 *   with iou >= min(thr, 1 - 1e-10) the match is the lexicographic maximum of (not ignored, iou, row) - the best non-ignored GT if one
 *   qualifies, else the best ignored one, equal IoUs to the later row.  A matched detection gets its TP bit and inherits the GT's ignore
 *   flag; an unmatched one is ignored iff it lies outside the stratum itself.  rec_m[n][NA] int32 = 10 TP bits | 10 ignore bits << 16
 *   (the layout ep24_segm_accumulate reads); rec_key, rec_cls, rec_p as ep24_eval_match; rec_val[n][2] double (nullable) = the
 *   detection's (area, zone).  npig[num_classes][NA] += the non-ignored GTs.  EP24_E_UNSUPPORTED: NA outside 1..8 and ep24_eval_match's
 *   limits; EP24_E_ARG: strata null or a stratum with lo > hi (or a NaN), and ep24_eval_match's.  B == 0 launches nothing.
 * ep24_eval_accumulate_strata: ep24_segm_accumulate's kernel and tables - precision[10][101][K][NA][NM], recall[10][K][NA][NM] - with
 *   NA <= 8 and NM <= 4 (EP24_E_UNSUPPORTED beyond); a record's position is the low 7 bits of its key.
 * ------------------------------------------------------------------------------------------------ */
int ep24_eval_measure(const float* rows, int ncols, int row_kind, const int32_t* image, int n, const double* scales,
                      const double* zt, int B, const float* ray_cs, double* out, void* stream);
int ep24_eval_match_strata(const float* labels, int L, int B, const float* rows, int ncols, const int64_t* row_off,
                           const int32_t* keep, int64_t keep_stride, const int32_t* count, const float* conf,
                           const int32_t* cls, int num_classes, int iou_type, const float* ray_cs, const double* iou_thr,
                           int max_dets, int64_t seq_base, int64_t* sort_scratch, int P, const double* scales,
                           const double* zt, const double* strata, int NA, int64_t* rec_key, int32_t* rec_cls,
                           int32_t* rec_p, int32_t* rec_m, double* rec_val, int32_t* rec_count, int32_t* npig,
                           int32_t* err, void* stream);
int ep24_eval_accumulate_strata(const int32_t* order, const int64_t* rec_key, const int32_t* rec_cls, const int32_t* rec_m,
                                int64_t n, const int32_t* npig, int num_classes, int NA, const int32_t* max_dets, int NM,
                                const double* rec_thr, int32_t* ctp_scratch, double* env_scratch, double* precision,
                                double* recall, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N1 input pipeline (yolox_24p/datasets/data_augment.py:109-174)
 * ------------------------------------------------------------------------------------------------ */
/* preproc for n images (n <= 65535): images = raw uint8 HWC sources in one device buffer; desc[n][6] int64 =
 * {byte offset, h, w, row stride in bytes, rh = int(h*r), rw = int(w*r)} with r = min(S_h/h, S_w/w) (:118-123);
 * scales[n][2] double = {1/(rw/w), 1/(rh/h)} (OpenCV's scale_x, scale_y).  out [n,3,S_h,S_w] fp32: the image resized
 * with cv2.resize's INTER_LINEAR fixed-point arithmetic in the top-left corner, 114 elsewhere, channels in source order. */
int ep24_preproc_u8(const uint8_t* images, const int64_t* desc, const double* scales, int n, float* out, int S_h, int S_w,
                    void* stream);
/* TrainTransform's label half (:145-173): rows [total][51] double = (class, 50 normalised coordinates) of all images,
 * row_off[n+1] int64, whr[n][3] double = (width, height, r).  out [n][max_labels][51] fp32: x columns (v*width)*r,
 * y columns (v*height)*r, first max_labels rows, zero padded. */
int ep24_preproc_labels(const double* rows, const int64_t* row_off, const double* whr, int n, float* out, int max_labels,
                        void* stream);
/* Multiscale training (Exp.preprocess, exp/yolox_base.py:109-118).  Bilinear resize of n contiguous fp32 planes sh x sw -> dh x dw
 * (n = B*3 for a batch; any positive sizes) with the result of F.interpolate(mode="bilinear", align_corners=False), the source
 * coordinates in DOUBLE: per axis s = (double)n_in / n_out, src = max(s*(d + 0.5) - 0.5, 0), i0 = min((int)src, n_in-1),
 * i1 = min(i0 + 1, n_in-1), w1 = (float)(src - i0), w0 = 1.0f - w1; then in fp32, every operation rounded on its own,
 * top = a*wx0 + b*wx1, bot = c*wx0 + d*wx1, out = top*wy0 + bot*wy1 (a, b from row y0; c, d from row y1).  Equal sizes: a copy.
 * A plane (source and destination) holds at most 2^31 - 1 elements. */
int ep24_resize_bilinear_f32(const float* src, int n, int sh, int sw, float* dst, int dh, int dw, void* stream);
/* The label half: rows x 51 floats; column 0 (the class) copied, odd columns * scale_x, even columns >= 2 * scale_y (one rounded fp32
 * multiply each: targets[..., 1::2] * scale_x, targets[..., 2::2] * scale_y).  out == in is allowed.  rows <= 2^40. */
int ep24_scale_labels(const float* in, float* out, int64_t rows, float scale_x, float scale_y, void* stream);
/* Test-time augmentation (csrc/tta.hip, ep24/tta.py).  ep24_mirror_f32: N planes [H][W] of fp32 mirrored left to right,
 * out[n][y][x] = in[n][y][W - 1 - x] as 32-bit words (NaN payloads stay); any W >= 1, 16-byte accesses when W % 4 == 0 and both
 * pointers are 16-byte aligned.  in == out is EP24_E_ARG. */
int ep24_mirror_f32(const float* in, int N, int H, int W, float* out, void* stream);
/* The B x A_v decoded prediction rows view[B][A_v][ncols] of one view of width w_v, brought back into the canonical frame and
 * written to rows [off, off + A_v) of every image of merged[B][A_tot][ncols]; other rows are not touched.  s = the fp32 value of
 * W0 / w_v, computed by the host in double and rounded once.  Each operation is one fp32 operation: cx' = cx * s, or
 * (w_v - cx) * s when mirror (the label mirror's W - x); cy' = cy * s; r'_k = r_k * s, or r_((12 - k) mod 24) * s when mirror.
 * Columns >= 26 are copied as words; with s == 1.0f and mirror == 0 the whole row is.  EP24_E_ARG: ncols < 27, off < 0,
 * off + A_v > A_tot, s not finite or not positive. */
int ep24_tta_unmap(const float* view, int B, int A_v, int ncols, int w_v, float s, int mirror, float* merged, int A_tot, int off,
                   void* stream);

/* Baseline JPEG decode, the arithmetic half ("JPEG decode"): what libjpeg's default path computes behind its Huffman stage
 * - dequantisation, the islow integer IDCT, "fancy" chroma upsampling, 16-bit fixed-point YCbCr -> RGB, clamp - bit for bit, for a
 * batch of images of any sizes and samplings in two launches.  The Huffman stage is libep24jpeg.so (include/ep24_jpeg.h), on the host.
 * ep24_jpeg_idct: coef = the int16 coefficient blocks of all planes (a plane = one component of one image), 64 per block in natural
 *   order, plane after plane, block row-major within a plane over its MCU-padded grid; qt = nqt tables of 64 uint16, natural order
 *   (both 16-byte aligned); plane_desc[n_planes + 1][4] int64 = {first block of the plane (cumulative, plane 0: 0), blocks per row,
 *   index of its table, 0}, row n_planes = {total_blocks}.  planes (8-byte aligned, 64 * total_blocks bytes): plane p is the uint8
 *   raster of 8 * blocks-per-row samples per row at byte 64 * first block.  One launch for every block of every image.
 * ep24_jpeg_color: image_desc[n + 1][12] int64 = {0 first 4-pixel group of the image (cumulative, image 0: 0; an image has
 *   ceil(H * W / 4)), 1 byte offset of the image in out (a multiple of 4), 2 H, 3 W, 4 mode (0 one component, 1 4:4:4, 2 4:2:2 = h2v1,
 *   3 4:2:0 = h2v2), 5 byte offset of the Y plane in planes, 6 its row stride, 7 / 8 byte offsets of the Cb / Cr planes, 9 their row
 *   stride, 10 dw = ceil(W / 2) (W for mode 1), 11 dh = ceil(H / 2) for mode 3, else H}, row n = {total_groups}.  out: every image a
 *   contiguous uint8 [H, W, 3] (the form ep24_preproc_u8 reads), channels B, G, R with bgr != 0, else R, G, B; a one-component image
 *   gives three equal channels.  One launch.
 * No image index sits in a grid dimension.  A store that a descriptor would send outside planes / out is dropped.  EP24_E_ARG: a
 * negative count, a null pointer with work to do, a misaligned buffer; a count of 0 launches nothing. */
int ep24_jpeg_idct(const void* coef, const void* qt, int nqt, const int64_t* plane_desc, int n_planes, int64_t total_blocks,
                   uint8_t* planes, void* stream);
int ep24_jpeg_color(const uint8_t* planes, const int64_t* image_desc, int n, int64_t total_groups, uint8_t* out, int64_t out_bytes,
                    int bgr, void* stream);

/* Baseline JPEG decode, the Huffman stage on the device ("JPEG decode: Huffman stage on the GPU"): the scan bytes of a batch
 * of files -> int16 coefficients in ep24_jpeg_idct's layout, by self-synchronising subsequence decoders; the marker walk that makes the
 * inputs is ep24jpeg_scan_layout of libep24jpeg.so (include/ep24_jpeg.h), the state machine is csrc/jpeg_huff_core.h.
 * ep24_jpeg_huffman: bytes[nbytes] = the entropy-coded data of all images; image_desc[n][16] int64 = {0 byte offset of the image's scan
 *   in bytes, 1 its length (below 2^28), 2 first row of the image in segments, 3 its restart segments (>= 1), 4 its subsequences (the sum
 *   of max(1, ceil(length / subseq_bytes)) over its segments), 5 first coefficient of the image in coef, 6 its coefficient count, 7
 *   components (1 or 3), 8 / 9 luma sampling h / v (1 or 2; chroma is 1 x 1), 10 / 11 MCUs per row / MCU rows, 12 restart interval in
 *   MCUs (0: none), 13 .. 15 0}; segments[nseg][6] int32 = {byte offset relative to the image's scan, length, first MCU, MCUs the
 *   segment must hold, first subsequence of the segment within the image (cumulative, segment 0: 0), 0}; table_specs[n][6] records of 276
 *   bytes (ep24jpeg_huff_spec: 16 code counts, 256 symbols, int32 symbol count): DC of component 0 .. 2, then AC of component 0 .. 2.
 *   subseq_bytes: 16, 32, 64, 128 or 256; tile: threads per workgroup = subsequences per tile, a multiple of 64 up to 1024.  One
 *   workgroup per image.  coef must be ZERO where the images lie (the caller's memset on the same stream): only nonzero coefficients
 *   are stored, the DC as the DIFFERENCE the file codes.  status[n] int32 is written for every image: 0, EP24JPEG_E_DATA (-4: an invalid
 *   code, a run past coefficient 63, bits consumed behind the end of a restart segment, or fewer complete blocks than a segment must
 *   hold; surplus bits and blocks at the end of a segment are ignored) or EP24_E_ARG (a descriptor row that does not fit the buffers:
 *   nothing of that image is read or written).
 * ep24_jpeg_dc: the same image_desc; turns the DC differences into values - a prefix sum per component in scan order, in int32, from zero
 *   at every restart segment - and sets status[i] = EP24JPEG_E_DATA where a value leaves int16.  Runs behind ep24_jpeg_huffman on the
 *   same stream; ep24_jpeg_idct then reads coef.
 * No image index sits in a grid dimension's limit (n <= 2^31 / 3).  A store that a descriptor would send outside the image's
 * coefficients is dropped.  EP24_E_ARG: a negative count, a null pointer with work to do, a misaligned buffer (descriptors 8 bytes,
 * segment rows and status 4), another subseq_bytes or tile; n = 0 launches nothing. */
int ep24_jpeg_huffman(const uint8_t* bytes, int64_t nbytes, const int64_t* image_desc, int n, const int32_t* segments, int64_t nseg,
                      const uint8_t* table_specs, int subseq_bytes, int tile, void* coef, int64_t ncoef, int32_t* status, void* stream);
int ep24_jpeg_dc(const int64_t* image_desc, int n, void* coef, int64_t ncoef, int32_t* status, void* stream);

/* Baseline JPEG encode, the arithmetic half ("JPEG encode"): what libjpeg's default compress path computes in front of its
 * Huffman stage - 16-bit fixed-point RGB -> YCbCr, h2v1 / h2v2 chroma downsampling with its edge rules, the islow integer forward
 * DCT, quantisation, the dummy blocks of the MCU padding - in every coefficient, for a batch of images of any sizes and samplings in two
 * launches.  The Huffman stage is ep24jpeg_entropy_encode of libep24jpeg.so (include/ep24_jpeg.h), on the host.
 * ep24_jpeg_sample: image_desc[n + 1][8] int64 = {0 first 8-sample group of the image (cumulative, image 0: 0), 1 device address of
 *   pixel (0, 0), 2 row stride in bytes, 3 H, 4 W, 5 mode (0 one component, 1 4:4:4, 2 4:2:2, 3 4:2:0) + 256 if the pixels are BGR,
 *   6 byte offset of the image's Y plane in planes (a multiple of 8), 7 0}, row n = {total_groups}.  The pixels are read where they
 *   lie: uint8, 3 bytes per pixel (1 for mode 0), rows `stride` apart.  With wb = ceil(cw / 8), hb = ceil(ch / 8) of a component
 *   (cw = W, ch = H for Y; halved and rounded up as the mode says for Cb / Cr) its plane is the uint8 raster of hb * 8 rows of wb * 8
 *   samples over its REAL block grid; Cb follows Y, Cr follows Cb.  An image has 8 hb wb groups for Y and, but for mode 0, as many of
 *   its chroma grid for Cb and Cr together.  One launch.
 * ep24_jpeg_fdct: plane_desc[n_planes + 1][8] int64 = {0 first block of the plane (cumulative over the MCU-padded grids, plane 0: 0),
 *   1 blocks per row of the padded grid, 2 index of its table, 3 byte offset of the plane in planes, 4 wb, 5 hb (the real grid),
 *   6 blocks of this component per MCU row (h), 7 0}, row n_planes = {total_blocks}; qt = nqt tables of 64 uint16, natural order.
 *   coef (int16, 64 * total_blocks) is filled in ep24_jpeg_idct's layout, dummy blocks included: zero but for the DC of the block to
 *   the left (in a dummy block row: of the last block of the row above in the same MCU).  One launch for every block of every image.
 * No image index sits in a grid dimension.  A store (and a read of planes) that a descriptor would send outside planes is dropped.
 * EP24_E_ARG: a negative count, a null pointer with work to do, a misaligned buffer (coef and qt 16 bytes, planes and descriptors 8);
 * a count of 0 launches nothing. */
int ep24_jpeg_sample(const int64_t* image_desc, int n, int64_t total_groups, uint8_t* planes, int64_t plane_bytes, void* stream);
int ep24_jpeg_fdct(const uint8_t* planes, int64_t plane_bytes, const void* qt, int nqt, const int64_t* plane_desc, int n_planes,
                   int64_t total_blocks, void* coef, void* stream);

/* Baseline JPEG encode, the Huffman stage on the device ("JPEG encode: Huffman stage on the GPU"): the coefficients
 * ep24_jpeg_fdct leaves on the device -> the entropy-coded bytes of every image (FF 00 stuffing, 1-padding, RSTn markers; no header, no
 * EOI), back to back in one buffer, byte for byte what ep24jpeg_entropy_encode of libep24jpeg.so writes between the SOS header and FF D9
 * with the Annex K tables.  The block walk, the bit emitter and the stuffing are csrc/jpeg_huffenc_core.h, which ep24jpeg_encode_emulate
 * runs on the host.  Shared inputs: coef (int16, ncoef values, ep24_jpeg_idct's layout); image_desc[n + 1][16] int64 = {0 first block of
 * the image in SCAN order (MCU by MCU: the luma component's h x v blocks row by row, then Cb, then Cr; cumulative, image 0: 0), 1 first
 * restart segment of the image (cumulative; an image has ceil(MCUs / interval) of them, 1 without restarts), 2 components (1 or 3), 3 / 4
 * luma sampling h / v (1 x 1, 2 x 1 or 2 x 2; chroma is 1 x 1), 5 / 6 MCUs per row / MCU rows (1 .. 1024), 7 restart interval in MCUs
 * (0: none), 8 .. 10 first block of each component's plane in coef (ep24_jpeg_fdct's cumulative block index), 11 .. 15 0}, row n =
 * {total_blocks, total_segments}.
 * ep24_jpeg_huffenc_count: positions[total_blocks] int64 receives, per block in scan order, the bits of the image's blocks up to and
 *   including it; segments[total_segments][2] int64 = {first 32-bit word of the segment relative to the image's first - every segment
 *   starts on a fresh word -, its bits without the 1-padding}; image_words[n] the words of every image, word_base[n + 1] their exclusive
 *   sum: what the caller reads back (ONE synchronisation) to allocate words[word_base[n]], zeroed.  Three launches.
 * ep24_jpeg_huffenc_emit: the same inputs and the count's outputs; every block's codes are shifted into words (big-endian; a word a block
 *   fills entirely is a plain store, its first and last word are ORed in with atomicOr - words MUST be zero), then image_bytes[n] (the
 *   stuffed bytes of every image, markers included), offsets[n + 1] (their exclusive sum) and out[offsets[i], offsets[i + 1]) are
 *   written: the caller reads offsets and copies only [0, offsets[n]).  out_bytes >= 8 * nwords + 2 * total_segments always suffices.
 *   Four launches.
 * status[n] int32, zeroed by the caller in front of the count: bits are ORed in - 1 a DC difference outside +-2047, 2 an AC coefficient
 *   outside +-1023 (nothing further of that block is coded; the image's bytes are then not a valid scan), 4 a store at or beyond nwords /
 *   out_bytes was dropped - or EP24_E_ARG is written: a descriptor row that does not fit the buffers, nothing of that image is read or
 *   written.  All positions are 64-bit.  No image index sits in a grid dimension's limit.
 * EP24_E_ARG: a negative count, a null pointer with work to do, a misaligned buffer (coef 16 bytes, descriptors and sums 8, words and
 * status 4); n = 0 launches nothing. */
int ep24_jpeg_huffenc_count(const void* coef, int64_t ncoef, const int64_t* image_desc, int n, int64_t total_blocks, int64_t total_segments,
                            int64_t* positions, int64_t* segments, int64_t* image_words, int64_t* word_base, int32_t* status, void* stream);
int ep24_jpeg_huffenc_emit(const void* coef, int64_t ncoef, const int64_t* image_desc, int n, int64_t total_blocks, int64_t total_segments,
                           const int64_t* positions, const int64_t* segments, const int64_t* word_base, uint32_t* words, int64_t nwords,
                           int64_t* image_bytes, int64_t* offsets, uint8_t* out, int64_t out_bytes, int32_t* status, void* stream);

/* Training augmentation (mosaic, random affine, mixup, mirror, HSV), two launches per batch.  Every output image
 * is assembled from up to four TILES: a tile is one source image, resized by s = min(S_h/h, S_w/w) as preproc resizes it and
 * placed on a canvas (2 S_h x 2 S_w with four tiles for a mosaic; S_h x S_w with one tile at the top left without).  Shared inputs:
 *   tiles[n][4][16] int64 = {0 byte offset of the source in `images`, 1 h, 2 w, 3 row stride in bytes, 4 rw = int(w*s),
 *       5 rh = int(h*s), 6 lx1, 7 ly1, 8 lx2, 9 ly2 (canvas region [lx1,lx2) x [ly1,ly2)), 10 padw, 11 padh (canvas position of
 *       the resized image's pixel (0,0): lx1 - sx1, ly1 - sy1), 12 row_lo, 13 row_hi (the source's label rows in `rows`),
 *       14, 15 reserved (0)}; an unused tile has an empty region (lx2 == lx1) and row_hi == row_lo;
 *   tile_scales[n][4][3] double = {1/(rw/w), 1/(rh/h) (OpenCV's scale_x, scale_y, as for ep24_preproc_u8), s};
 *   params[n][16] double = {0 a00, 1 a01, 2 t0, 3 a10, 4 a11, 5 t1: canvas -> output, o = A*c + t;  6 i00, 7 i01, 8 i02, 9 i10,
 *       10 i11, 11 i12: its inverse, computed by the host in double;  12 dh, 13 ds, 14 dv: HSV gains;  15 reserved (0)};
 *   flags[n][2] int32 = {mirror, hsv on}.
 * ep24_augment_u8: out [n,3,S_h,S_w] fp32.  Output pixel (x, y): xm = mirror ? S_w-1-x : x; canvas u = (i00*xm + i01*y) + i02,
 * v = (i10*xm + i11*y) + i12 in double; the owner is the first tile with lx1-0.5 <= u < lx2-0.5 and ly1-0.5 <= v < ly2-0.5 (none:
 * 114 in the three channels); fx = ((u - padw) + 0.5)*scale_x - 0.5 (fy likewise) in double, rounded to float, then the fixed-point
 * bilinear sample of ep24_preproc_u8.  With hsv on, sampled pixels (not the padding) go BGR -> HSV (H in [0,180), S, V in [0,255]),
 * H = (H + dh) mod 180, S = clip(S + ds, 0, 255), V = clip(V + dv, 0, 255) and back in fp32, nothing rounded to uint8 (cv2 rounds
 * twice).  With hsv off the output is a bit-exact function of the inputs. */
int ep24_augment_u8(const uint8_t* images, const int64_t* tiles, const double* tile_scales, const double* params,
                    const int32_t* flags, int n, float* out, int S_h, int S_w, void* stream);
/* The label half: rows [total][51] double = (class, 50 normalised coordinates); rot[24][2] double = cos / sin of k*15 degrees
 * (ep24.labels24._rot_table).  Candidates of image i are the rows of tile 0, then tile 1, ... (the first max_labels of each).
 * All arithmetic in double: canvas X = (v*w)*s + padw, Y = (v*h)*s + padh; output c' = A*c + t, P'_j = A*P_j + t, mirrored
 * x -> S_w - x.  A candidate survives if its centre is at least min_margin inside both the output rectangle [0,S_w] x [0,S_h] and
 * (in canvas space) its tile's region, and if the 24 re-cast vertices have min(width, height) > 1.  Re-cast vertex k =
 * c' + r_k * (cos, sin)(15k deg), r_k = the smallest t >= 0 at which the ray meets one of the 24 edges P'_j -> P'_j+1 (ends
 * included), cut at the ray's exit from the output rectangle and at its exit from the tile's region (taken in canvas space along
 * A^-1 * d, x negated first when mirrored).  out [n][max_labels][51] fp32: the survivors in candidate order, the first max_labels
 * of them, zero padded; out_count[n] int32: the number of survivors (it may exceed max_labels). */
int ep24_augment_labels(const double* rows, const int64_t* tiles, const double* tile_scales, const double* params,
                        const int32_t* flags, const double* rot, int n, int S_h, int S_w, double min_margin, float* out,
                        int32_t* out_count, int max_labels, void* stream);
/* Mixup (MosaicDetection.mixup) fused into the same two launches: every argument of the sibling above, plus one descriptor per
 * output image.  An image whose descriptor has on == 0 comes out bit-identical to ep24_augment_u8 / ep24_augment_labels.
 *   mix[n][16] int64 = {0 on, 1 byte offset of the partner source in `images`, 2 h, 3 w, 4 row stride in bytes, 5 rw = int(w*s),
 *       6 rh = int(h*s), 7 Wj = int(S_w*jit), 8 Hj = int(S_h*jit) (the jittered canvas, both >= 1), 9 x_off, 10 y_off (>= 0: the
 *       crop window's corner on the jittered canvas), 11 flip, 12 row_lo, 13 row_hi (the partner's label rows in `rows`),
 *       14, 15 reserved (0)};
 *   mix_scales[n][12] double = {0 S_w/Wj, 1 S_h/Hj, 2 1/(rw/w), 3 1/(rh/h), 4 s, 5 a00 = flip ? -Wj/S_w : Wj/S_w, 6 a11 = Hj/S_h,
 *       7 t0 = flip ? Wj - x_off : -x_off, 8 t1 = -y_off, 9 1/a00, 10 1/a11, 11 reserved (0)}.
 * ep24_augment_mix_u8: with a = the pixel of ep24_augment_u8 BEFORE HSV as an integer (114 where no tile owns it) and
 * px = xm + x_off, py = y + y_off: the partner value b is 0 if px >= Wj or py >= Hj; otherwise pxf = flip ? Wj-1-px : px,
 * u = (pxf+0.5)*(S_w/Wj) - 0.5, v = (py+0.5)*(S_h/Hj) - 0.5 in double, and b is ONE fixed-point bilinear sample of the partner at
 * fx = (u+0.5)*scale_x - 0.5 (fy likewise; a tile with padw = padh = 0) if -0.5 <= u < rw-0.5 and -0.5 <= v < rh-0.5, else 114.
 * The output is (a + b) >> 1 per channel (0.5*a + 0.5*b truncated to uint8), then HSV on the pixels that a tile or the partner
 * image owns, then the store.  cv2 would resize twice (letterbox, jitter); here the pixel is one sample of the raw source. */
int ep24_augment_mix_u8(const uint8_t* images, const int64_t* tiles, const double* tile_scales, const double* params,
                        const int32_t* flags, const int64_t* mix, const double* mix_scales, int n, float* out, int S_h, int S_w,
                        void* stream);
/* The label half with the partner as a fifth candidate source behind the four tiles (the first max_labels of its rows): canvas
 * X = (v*w)*s, Y = (v*h)*s; output (a00*X + t0, a11*Y + t1), mirrored like every other row; region [0,rw] x [0,rh] for the
 * centre margin and for the ray's exit (along (d_x/a00, d_y/a11), x negated first when mirrored).  Keep rules, re-cast, order,
 * cap and count as ep24_augment_labels. */
int ep24_augment_mix_labels(const double* rows, const int64_t* tiles, const double* tile_scales, const double* params,
                            const int32_t* flags, const int64_t* mix, const double* mix_scales, const double* rot, int n, int S_h,
                            int S_w, double min_margin, float* out, int32_t* out_count, int max_labels, void* stream);
/* Copy-paste (YOLOv5 / v8 copy_paste; csrc/paste.hip): a post-pass of two launches over the batch the launches
 * above produced.  The 24-gon of a label row is the object's mask.  Conventions as above: pixel x covers [x, x+1), its centre is
 * x + 0.5; labels [n][max_labels][51] fp32 rows (class, cx, cy, 24 x (x, y)) in output pixels; images [n,3,S_h,S_w] fp32.
 *   paste[n][8] int64 = {0 on, 1 partner j (0 <= j < n, j == i allowed), 2 flip, 3 dx, 4 dy, 5 select (bit k = candidate k may be
 *       pasted), 6, 7 reserved (0)}.  Image i takes objects of image j through the rigid integer transform
 *       point (X, Y) -> ((flip ? S_w - X : X) + dx, Y + dy);  output pixel (x, y) reads source pixel (xs, ys) with xu = x - dx,
 *       xs = flip ? S_w - 1 - xu : xu, ys = y - dy.  No resampling.
 * ep24_paste_labels: pre_labels / pre_count are the label launch's outputs for the whole batch, a snapshot (out_labels is another
 * buffer).  With E = min(pre_count[i], max_labels): out_labels[i][0:E] = pre_labels[i][0:E] bit for bit, the rest zero,
 * out_count[i] = pre_count[i], paste_range[n][2] int32 = {E, E}.  With on != 0 and pre_count[i] <= max_labels the candidates are
 * rows k = 0 .. min(pre_count[j], max_labels) - 1 of pre_labels[j], in that order, until the image holds max_labels rows.  The
 * transformed coordinates are evaluated in double on the fp32 inputs as written above and rounded once to fp32; those fp32 values
 * are what is tested and stored.  Candidate k is skipped if bit k of select is clear (k >= 64: always), if its centre is not at
 * least min_margin inside [0,S_w] x [0,S_h], if one of its 24 vertices is outside that closed rectangle, or if some row q among the
 * image's E rows and the candidates accepted before it has area(q) > 0 and inter(cand, q) / area(q) >= ioa_thr (inter: poly24.h's
 * trapezoid-decomposition intersection, area: the absolute shoelace area, both in double from the fp32 vertices; one division).
 * Otherwise it is appended as (class, transformed centre, vertices); with flip, source vertex k becomes vertex (12 - k) mod 24 (the
 * mirrored ray of 15k degrees is the ray of 180 - 15k degrees), so the row stays ordered by ray.  out_count[i] and
 * paste_range[i][1] grow by one per accepted candidate.  Acceptance is sequential per image: the result is a deterministic
 * function of the inputs.  The descriptor lives in device memory, so the library cannot refuse a partner outside [0, n): the
 * host side that builds it does (ep24.augment.paste_descriptors raises with EP24_E_ARG), and the kernels treat such a descriptor
 * as on == 0.  EP24_E_ARG: n < 0, a null pointer with n > 0, max_labels outside 1 .. 256, ioa_thr <= 0, min_margin < 0,
 * out_labels == pre_labels.  n == 0 is EP24_OK; n is cut into launches of 65 535 inside the call. */
int ep24_paste_labels(const float* pre_labels, const int32_t* pre_count, const int64_t* paste, int n, int S_h, int S_w,
                      double min_margin, double ioa_thr, float* out_labels, int32_t* out_count, int32_t* paste_range, int max_labels,
                      void* stream);
/* The image half, bit exact (fp32 in, fp32 out, no arithmetic on pixel values); every output word is written; out_images !=
 * pre_images.  Pixel (x, y) of image i is pre_images[j][c][ys][xs] if on, (xs, ys) is inside the image and the point
 * (x + 0.5, y + 0.5) is inside at least one row of out_labels[i][paste_range[i][0] : paste_range[i][1]] by the crossing rule of
 * ep24_poly24_raster (csrc/raster_rule.h, vertices promoted to double); otherwise it is pre_images[i][c][y][x].  A row with a NaN
 * or infinite coordinate pastes nothing (ep24_paste_labels never writes one).  Tiles of 64 x 16 pixels that no pasted row's vertex
 * box meets are a plain copy.  S_w % 4 == 0 with 16-byte aligned buffers moves four pixels per access; any other shape runs pixel
 * by pixel. */
int ep24_paste_u8(const float* pre_images, const float* out_labels, const int32_t* paste_range, const int64_t* paste, int n,
                  float* out_images, int S_h, int S_w, int max_labels, void* stream);

/* ------------------------------------------------------------------------------------------------
 * C4  swapped backbones (yolox_24p/models/darknet.py:179-429, yolox/models/yolo_pafpn.py:31-38; BASELINE config 4)
 *     The conv / BN+act entry points above carry them (act = 2 is ReLU); these are the remaining pieces.
 * ------------------------------------------------------------------------------------------------ */
/* im2col of fp32 NCHW images for a k x k / stride / pad conv (the ResNet stem: 7, 2, 3): rows [B*OH*OW][ld] bf16, column
 * (kh*k + kw)*C + c, zero in the padding and in columns >= k*k*C; the conv itself is then a 1x1 GEMM over the rows. */
int ep24_im2col_bf16(const float* images, void* rows, int64_t ld, int B, int C, int H, int W, int k, int stride, int pad,
                     void* stream);
/* Bottleneck tail "out += identity; out = relu(out)" (darknet.py:266-268): the sum comes out of ep24_bn_act_fwd (act 0 +
 * residual); relu_fwd clamps it in place (x < 0 -> +0; NaN stays NaN and -0 stays -0, as ATen's relu: a diverged value stays
 * visible), relu_bwd masks the incoming gradient in place with the stored output (y <= 0 -> +0, as ATen's threshold_backward: a NaN y
 * passes the gradient). */
int ep24_relu_fwd(void* y, int64_t ld, int64_t M, int C, void* stream);
int ep24_relu_bwd(void* dy, int64_t ld_dy, const void* y, int64_t ld_y, int64_t M, int C, void* stream);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (darknet.py:303) on NHWC bf16; idx [B*OH*OW*C] uint8 = winning tap
 * (first maximum in scan order, as ATen); the backward gathers (no atomics), accumulate = 1 adds to dx. */
int ep24_maxpool3s2_fwd(const void* x, int64_t ld_x, void* y, int64_t ld_y, uint8_t* idx, int B, int H, int W, int C,
                        void* stream);
int ep24_maxpool3s2_bwd(const void* dy, int64_t ld_dy, const uint8_t* idx, void* dx, int64_t ld_dx, int accumulate, int B,
                        int H, int W, int C, void* stream);

/* DenseNet pieces (darknet.py:515-674).  Its pre-activation blocks (BatchNorm -> ReLU -> conv over a growing concatenation)
 * run as ep24_bn_act_fwd on the shared input with per-layer statistics gathered from the block's, the input gradient of
 * every consumer accumulating through ep24_bn_act_bwd_apply_acc. */
/* per-channel sum / sum of squares of x [M][C] (row stride ld) added to stats[0][0..1][c] with channel stride ld_stats
 * (the conv epilogue's fixed-point layout [rep][2][ld_stats]). */
int ep24_colstats(const void* x, int64_t ld, int64_t* stats, int64_t ld_stats, int64_t M, int C, void* stream);
/* dst[rep][2][C] = the first C channels of src[rep][2][ld_src]. */
int ep24_stats_gather(const int64_t* src, int64_t ld_src, int64_t* dst, int C, int reps, void* stream);
/* ep24_bn_act_bwd_apply with dz += instead of dz = (same arguments, every act of 0 .. 3): dz = bf16(float(bf16(new)) + old).
 * Every ep24_bn_act_* entry point refuses an act outside 0 .. 3 with EP24_E_ARG. */
/* Round 5: pass 1 and pass 2 as ONE launch (at most one 256-thread workgroup per CU; a grid-wide arrive / wait on *barrier between the
 * passes - an int32 the caller zeroes before the launch; a bounded spin whose give-ups ep24_conv_ring_timeouts counts).  Same sums,
 * same dz, same gradient publication as the two launches. */
int ep24_bn_act_bwd_fused(const void* dy, int64_t ld_dy, const void* z, int64_t ld_z, const float* save, const float* gamma,
                          const float* beta, int64_t* dgamma, int64_t* dbeta, float* gamma_grad, float* beta_grad, void* dz,
                          int64_t ld_dz, int64_t M, int C, int act, int reps, int32_t* barrier, void* stream);
int ep24_bn_act_bwd_apply_acc(const void* dy, int64_t ld_dy, const void* z, int64_t ld_z, const float* save,
                              const float* gamma, const float* beta, const int64_t* dgamma, const int64_t* dbeta,
                              float* gamma_grad, float* beta_grad, void* dz, int64_t ld_dz, int64_t M, int C, int act, int reps,
                              void* stream);
/* nn.AvgPool2d(2, 2) of the Transition blocks, NHWC bf16. */
int ep24_avgpool2_fwd(const void* x, int64_t ld_x, void* y, int64_t ld_y, int B, int H, int W, int C, void* stream);
int ep24_avgpool2_bwd(const void* dy, int64_t ld_dy, void* dx, int64_t ld_dx, int accumulate, int B, int H, int W, int C,
                      void* stream);
/* nn.MaxPool2d(kernel_size=2, stride=2) of the VGG backbone (darknet.py:481), NHWC bf16; idx = winning tap per output element. */
int ep24_maxpool2_fwd(const void* x, int64_t ld_x, void* y, int64_t ld_y, uint8_t* idx, int B, int H, int W, int C,
                      void* stream);
int ep24_maxpool2_bwd(const void* dy, int64_t ld_dy, const uint8_t* idx, void* dx, int64_t ld_dx, int accumulate, int B,
                      int H, int W, int C, void* stream);
/* *p += 1 on the stream: num_batches_tracked of a BatchNorm module whose launch is shared with a neighbour (the merged
 * conv1 / conv2 unit of a CSP layer). */
int ep24_incr_i64(int64_t* p, void* stream);
/* nn.Dropout2d as data: x[n, :, :, c] *= keep[n*C + c] in place (keep = 0 or 1/(1-p), drawn by the host once per step);
 * the same call is its backward. */
int ep24_chanscale(void* x, int64_t ld, const float* keep, int B, int64_t HW, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EP24_H */
