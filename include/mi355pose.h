/*
 * mi355pose.h — C ABI of libmi355pose.so: the MI355X (gfx950) kernels underneath the
 * domain-adaptive hand-pose training / evaluation hot path.
 *
 * The reference (CVlab315/Domain-Adaptative-Hand-Pose-Estimation) has NO native / FFI
 * boundary: it is 100 % Python on torch.nn.  Its drop-in surface is the
 * Python API (train1.py / test.py CLIs, uda.model class names, state_dict layout), which the
 * host package mirrors.  This header is the NEW internal boundary beneath that Python API:
 * one entry point per fused op and direction, each replacing the ATen op sequence the
 * reference issues at the cited file:line (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers + sizes; every buffer is DEVICE memory allocated by the caller;
 *     the library never allocates, never synchronises, never owns memory;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default);
 *     every entry point is hipGraph-capturable;
 *   - returns 0 on success, a negative MI355_E* code otherwise; text via mi355_last_error()
 *     (thread-local); no exceptions cross the ABI; re-entrant (autograd worker threads);
 *   - activations are NHWC ("rows x channels"), dtype MI355_F32 or MI355_BF16;
 *     heat-maps (21 channels) are NCHW fp32 rows of H*W, as the reference's losses see them;
 *   - scalars that change every iteration (GL lambda, learning rate, upstream loss grad)
 *     are read from DEVICE floats so that a captured graph replays with fresh values.
 *   - "conv-form": every conv-like layer is described as the convolution
 *         y[N,Ho,Wo,Co] = conv(x[N,Hi,Wi,Ci], w[Co][kh][kw][Ci], stride, pad)
 *     nn.Conv2d uses it directly; nn.ConvTranspose2d(Cin,Cout) is the ADJOINT of the
 *     conv-form with Co=Cin_t, Ci=Cout_t (its forward is conv_dgrad, its input-gradient is
 *     conv_fwd, its weight-gradient is conv_wgrad with the roles of x/dy swapped).
 */
#ifndef MI355POSE_H
#define MI355POSE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_F32 0
#define MI355_BF16 1
#define MI355_FP8 2   /* conv descriptors of the *_fp8 entry points only: fp8 operands, fp32 accumulate, bf16 results */

#define MI355_OK 0
#define MI355_EINVAL (-1)   /* bad argument / unsupported shape */
#define MI355_ELAUNCH (-2)  /* HIP launch error */
#define MI355_EWORKSPACE (-3)

typedef struct {
  int N, Hi, Wi, Ci; /* conv-form input  (NHWC)                       */
  int Ho, Wo, Co;    /* conv-form output (NHWC); = (Hi + 2 pad - kh) / stride + 1, or -- unit stride, mi355_conv_fwd* and
                        mi355_conv_wgrad only -- any smaller size: the top-left Ho x Wo crop of that output */
  int kh, kw, stride, pad;
  int dtype;         /* MI355_F32 | MI355_BF16 (activations+packed weights) | MI355_FP8 (mi355_conv_*_fp8 only) */
} mi355_conv_desc;

int mi355_version(void);
const char* mi355_last_error(void);

/* ---------------------------------------------------------------- convolutions (MFMA implicit GEMM)
 * Replace torch.nn.Conv2d / ConvTranspose2d forward+backward issued by
 *   uda/model/resnet.py:23-38 (torchvision ResNet stem/blocks), uda/model/pose_resnet2.py:33-41
 *   (3x ConvTranspose2d 4x4 s2 p1), uda/model/regda_7.py:4906-4929 (_make_head),
 *   :4513-4514,4551,4561 (make_head), :4588-4589,4627,4637 (make_head2).
 * w  : packed weights [Co][kh][kw][Ci]  in `dtype`     (forward operand)
 * wT : packed weights [Ci][kh][kw][Co]  in `dtype`     (dgrad operand)
 * bias: fp32 [Co] or NULL.  residual: tensor shaped like y (added before the store) or NULL.
 * scale_dev: NULL or device float multiplied into the result (folds utils/gl.py:18, grad*coeff).
 * accumulate!=0 : dx += result (several consumers of one tensor), else dx = result.
 * dw: fp32 [Co][kh][kw][Ci]; accumulate!=0 adds into dw.  ws: scratch of at least
 * mi355_conv_wgrad_workspace() bytes.
 */
int mi355_conv_fwd(const mi355_conv_desc* d, const void* x, const void* w, const float* bias,
                   const void* residual, void* y, void* stream);
int mi355_conv_dgrad(const mi355_conv_desc* d, const void* dy, const void* wT, const float* bias,
                     const float* scale_dev, int accumulate, void* dx, void* stream);
/* 1x1 / unit-stride bf16 convs (forward and input gradient) can run on a second kernel, the persistent pipelined GEMM of
 * csrc/pgemm.hip (same results bit for bit): mode 0 never (default: end to end it measured no gain), 1 where
 * it was faster per layer in isolation, 2 wherever the launch fits it (tests / A-B runs), -1 back to the environment's choice
 * (MI355_PGEMM).  Returns the previous setting. */
int mi355_set_pgemm(int mode);
/* Inference forms: y = act(conv(x) + bias + residual), dx = act(dgrad(dy) + bias) (the ConvTranspose2d forward), act = ReLU when
 * relu != 0.  The caller folds an eval-mode BatchNorm that follows into the operands (w * gamma / sqrt(var + eps) per output
 * channel, bias = beta - mean * that scale): conv -> BN -> (+identity) -> ReLU of resnet.py / pose_resnet2.py:33-41 /
 * regda_7.py:4906-4929 becomes one launch in test.py's forward-only path. */
int mi355_conv_fwd_act(const mi355_conv_desc* d, const void* x, const void* w, const float* bias, const void* residual, int relu,
                       void* y, void* stream);
int mi355_conv_dgrad_act(const mi355_conv_desc* d, const void* dy, const void* wT, const float* bias, int relu, void* dx,
                         void* stream);
/* dx <- result + (bit of acc_mask set ? dx : 0).  acc_mask: the ReLU bit mask of mi355_bn_train_fwd over a tensor shaped like
 * dx.  The fork of a residual block (torchvision Bottleneck / BasicBlock: out = relu(bn(...) + identity)): dx holds the
 * gradient of the block's OUTPUT ReLU input, still unmasked, and the conv is the block's first one (same input as the
 * identity branch); replaces the masked copy mi355_bn_bwd would write as `dresidual` and the add autograd would run. */
int mi355_conv_dgrad_masked_acc(const mi355_conv_desc* d, const void* dy, const void* wT, const float* scale_dev, void* dx,
                                const void* acc_mask, void* stream);
/* Convolution / transposed-convolution forward with the BatchNorm batch statistics of its OUTPUT computed in the
 * epilogue (the nn.BatchNorm2d that follows every conv of resnet.py / pose_resnet2.py:33-41 / regda_7.py:4906-4929 in
 * training mode): partial[slice][Co|Ci][n, mean, M2] per output-row tile, *nslices = slices written (0: this launch
 * could not fuse them -- the caller then runs mi355_bn_train_fwd).  partial_bytes >= mi355_conv_stats_bytes(rows, C). */
size_t mi355_conv_stats_bytes(long rows, int C);
int mi355_conv_fwd_stats(const mi355_conv_desc* d, const void* x, const void* w, const float* bias, void* y,
                         float* partial, size_t partial_bytes, int* nslices, void* stream);
int mi355_conv_dgrad_stats(const mi355_conv_desc* d, const void* dy, const void* wT, void* dx, float* partial,
                           size_t partial_bytes, int* nslices, void* stream);
/* Concatenated-K forward: y = conv(x, w) + x2 * w2^T + bias + bias2 as ONE implicit GEMM (K = kh*kw*Ci + c2).  Replaces the
 * `heatmap_conv(heatmap) + feature_conv(feature)` pair at the entry of the multiscale-fusion heads (reference
 * uda/model/regda_7.py:4573-4581 make_head.forward, :4649-4662 make_head2.forward) by one launch: x2 [N*Ho*Wo][c2] is the
 * heat-map operand re-laid as NHWC at the OUTPUT resolution (mi355_nchw_to_nhwc, channels zero-padded to c2), w2 [Co][c2]
 * the 1x1 heat-map weights, both in the descriptor's dtype (bf16 / fp32); c2 a multiple of the 16-byte chunk, <= 64 (bf16) /
 * 32 (fp32).  bias / bias2 nullable.  partial / nslices: nullable pair, BatchNorm statistics of y as in mi355_conv_fwd_stats. */
int mi355_conv_fwd_cat(const mi355_conv_desc* d, const void* x, const void* w, const float* bias, const void* x2,
                       const void* w2, const float* bias2, int c2, void* y, float* partial, size_t partial_bytes,
                       int* nslices, void* stream);
/* The same idea for the BACKWARD pass: a GEMM whose output is the dy of a BatchNorm (the input gradient of the conv
 * that consumed the BatchNorm's output) leaves that BatchNorm's backward reduction (sum dy_eff, sum dy_eff * xhat) per
 * output-row tile in partial[slice][C][2]; mi355_bn_bwd_partials then skips its reduction pass.  bn: the BatchNorm's
 * saved forward state; relu != 0 masks dy with y > 0 (y given) or with the mask recomputed from x (y NULL). */
typedef struct mi355_bn_bwd_src {
  const void* x; const void* y; const float* gamma; const float* beta; const float* save_mean; const float* save_invstd;
  int relu;
} mi355_bn_bwd_src;
int mi355_conv_dgrad_bnbwd(const mi355_conv_desc* d, const void* dy, const void* wT, const float* scale_dev, int accumulate,
                           void* dx, const mi355_bn_bwd_src* bn, float* partial, size_t partial_bytes, int* nslices,
                           void* stream);
int mi355_conv_fwd_bnbwd(const mi355_conv_desc* d, const void* x, const void* w, void* y, const mi355_bn_bwd_src* bn,
                         float* partial, size_t partial_bytes, int* nslices, void* stream);
/* ---- fp8 operand path (BASELINE config 5: "fp8 conv MFMA path"; reference layers: the K-heavy 3x3 / 4x4 convolutions
 * of uda/model/regda_7.py:4906-4929, pose_resnet2.py:33-41 and the torchvision Bottleneck 3x3).  OCP formats:
 * fmt 0 = e4m3 (activations, weights), fmt 1 = e5m2 (gradients).  Per-tensor scaling state = 4 floats on the device:
 * {scale, descale = 1/scale, amax bits (max |x| seen since the last update), descale of the latest weight pack made with it}.
 * A copy must be descaled with the scale it was MADE with: the state is refreshed at every optimizer step and a copy may be
 * consumed after that, so activation copies carry their own record (write = 2 below) and weight packs leave theirs in state[3].
 *
 * mi355_fp8_quantize: q[i] = saturate_fmt(x[i] * state[0]) for i < n (n a multiple of 16; x bf16 or fp32), and
 *   state[2] = max(state[2], max |x|) -- with write = 0 only the amax is taken (just-in-time scaling: amax, update, quantise);
 *   write = 2: q has 16 more bytes behind its n, which receive this copy's own record {scale, descale, 0, 0} (usable wherever
 *   a state's descale is read).
 * mi355_fp8_update_scale: for each of n states (stride_floats apart): scale = 2^k, k = the largest integer with
 *   amax * 2^margin * 2^k <= fmt_max, clamped to [-126, 126] (kept when no amax, or one >= 3.0e38, was recorded; 1 if never
 *   set), descale = 2^-k, amax = 0.  max |x| skips NaN elements and counts Inf.
 * mi355_pack_weights_fp8: fp32 master [O][T][I] -> e4m3 wf [O][T][I] and wt [I][T][O] (O, I multiples of 32).  margin >= 0:
 *   just-in-time per-tensor scale from amax(|w|), left in `state`; margin < 0: the scale already in `state` (delayed
 *   scaling).  Either way amax(|w|) is recorded in state[2] for the next mi355_fp8_update_scale, and state[3] = the descale
 *   this pack was made with (what its consumers must read). */
int mi355_fp8_quantize(const void* x, void* q, float* state, long n, int src_dtype, int fmt, int write, void* stream);
int mi355_fp8_update_scale(float* states, int n, int stride_floats, int fmt, int margin, void* stream);
int mi355_pack_weights_fp8(const float* w, void* wf, void* wt, float* state, int O, int T, int I, int margin, void* stream);
/* The same for many weights in one launch with the scales already in their states (delayed scaling): items in DEVICE memory,
 * blk0 = first block of the item = sum over earlier items of (O/32)*(I/32)*T. */
typedef struct mi355_pack8_item { const float* w; void* wf; void* wt; float* state; int O, T, I, blk0; } mi355_pack8_item;
int mi355_pack_weights_fp8_batched(const mi355_pack8_item* items_dev, int nitems, int total_blocks, void* stream);
/* mi355_conv_fwd / mi355_conv_dgrad with fp8 operands (d->dtype = MI355_FP8; channels contracted over: a multiple of 128):
 *   y  (bf16) = (conv(x8, w8)  * *descale_x  * *descale_w + bias) [+ residual]
 *   dx (bf16) = (dgrad(dy8, wT8) * *descale_dy * *descale_w) * (*scale_dev, optional) [+ dx when accumulate]
 * partial / nslices (nullable): BatchNorm statistics of the result from the epilogue, as mi355_conv_fwd_stats. */
int mi355_conv_fwd_fp8(const mi355_conv_desc* d, const void* x8, int x_fmt, const void* w8, const float* descale_x,
                       const float* descale_w, const float* bias, const void* residual, void* y, float* partial,
                       size_t partial_bytes, int* nslices, void* stream);
int mi355_conv_dgrad_fp8(const mi355_conv_desc* d, const void* dy8, int dy_fmt, const void* wT8, const float* descale_dy,
                         const float* descale_w, const float* scale_dev, int accumulate, void* dx, float* partial,
                         size_t partial_bytes, int* nslices, void* stream);
/* ---- MX (block-scaled) fp8 operand path ('mxfp8' compute mode; the same reference layers as the fp8 path: the K-heavy
 * 3x3 convs of uda/model/regda_7.py:4906-4929, the torchvision Bottleneck conv2 (resnet.py:92-107, stride 1 and 2) and the
 * 4x4 transposed convs of pose_resnet2.py:33-41).  Elements e4m3 (format 0) for every operand, gradients included; one E8M0
 * scale byte per block of 32 consecutive elements along the contracted axis; no scaling state.
 * Scale rule (NOT OCP MX v1.0's floor(log2 amax) - 8, which saturates the top of a block): amax = m * 2^E (m in [1, 2)),
 * e = E - 8 + (m > 1.75), clamped to [-127, 127]; byte = e + 127; element = RNE_e4m3(x * 2^-e).  All-zero block: 0x00;
 * a block holding NaN or Inf: 0xFF (E8M0 NaN), its elements quantised with the e of its finite values.
 *
 * mi355_mx_quantize: x [rows][C] (bf16 or fp32, C a multiple of 32) -> q e4m3 [rows][C] and scales [rows][C/32].  x and q
 *   16-byte aligned.
 * mi355_pack_weights_mx: fp32 master [O][T][I] (O, I multiples of 32) -> wf e4m3 [O][T][I] + sf [O][T][I/32] (forward operand)
 *   and wt e4m3 [I][T][O] + st [I][T][O/32] (input-gradient operand, blocks along O), both quantised from the master.
 * mi355_pack_weights_mx_batched: the same for many weights in one launch: items in DEVICE memory, blk0 = first block of the
 *   item = sum over earlier items of (O/32)*(I/32)*T. */
int mi355_mx_quantize(const void* x, void* q, void* scales, long rows, int C, int src_dtype, void* stream);
int mi355_pack_weights_mx(const float* w, void* wf, void* sf, void* wt, void* st, int O, int T, int I, void* stream);
typedef struct mi355_packmx_item { const float* w; void* wf; void* sf; void* wt; void* st; int O, T, I, blk0; } mi355_packmx_item;
int mi355_pack_weights_mx_batched(const mi355_packmx_item* items_dev, int nitems, int total_blocks, void* stream);
/* mi355_conv_fwd / mi355_conv_dgrad on MX operands (d->dtype = MI355_FP8; the contracted channel count -- Ci forward, Co input
 * gradient -- a power-of-two multiple of 128; the other a multiple of 8):
 *   y  (bf16) = conv(x8 * 2^sx, w8 * 2^sw) + bias [+ residual]           x8 [N][Hi][Wi][Ci], sx [N][Hi][Wi][Ci/32],
 *                                                                         w8 [Co][T][Ci],     sw [Co][T][Ci/32]
 *   dx (bf16) = dgrad(dy8 * 2^sdy, wT8 * 2^swT) * (*scale_dev, optional) [+ dx when accumulate]
 *                                                                         dy8 [N][Ho][Wo][Co], sdy [N][Ho][Wo][Co/32],
 *                                                                         wT8 [Ci][T][Co],     swT [Ci][T][Co/32]
 * (2^s: the E8M0 block scale).  fp32 accumulate; partial / nslices (nullable, together): BatchNorm statistics of the result
 * from the epilogue, as mi355_conv_fwd_stats.  Null pointers and misaligned channel counts fail before any launch. */
int mi355_conv_fwd_mx(const mi355_conv_desc* d, const void* x8, const void* sx, const void* w8, const void* sw, const float* bias,
                      const void* residual, void* y, float* partial, size_t partial_bytes, int* nslices, void* stream);
int mi355_conv_dgrad_mx(const mi355_conv_desc* d, const void* dy8, const void* sdy, const void* wT8, const void* swT,
                        const float* scale_dev, int accumulate, void* dx, float* partial, size_t partial_bytes, int* nslices,
                        void* stream);
/* Inference on MX operands (opt-in, mi355.set_mx_eval / MI355_MX_EVAL): the eval-mode forms of the same reference layers --
 * Bottleneck conv2 + bn2 + relu (resnet.py:92-107), the transposed convs + BatchNorm + ReLU of the upsampling neck
 * (pose_resnet2.py:33-41) and the 3x3 conv + BatchNorm + ReLU runs of the heads (regda_7.py:4906-4929) -- with the BatchNorm
 * folded into the packed weights and the bias by the caller, as for mi355_conv_fwd_act / mi355_conv_dgrad_act:
 *   y  (bf16) = act(conv(x8 * 2^sx, w8 * 2^sw) + bias [+ residual])      act = max(., 0) when relu, else the identity
 *   dx (bf16) = act(dgrad(dy8 * 2^sdy, wT8 * 2^swT) + bias)              (the transposed conv's forward, every stride-2 phase)
 * Operand constraints as mi355_conv_fwd_mx / mi355_conv_dgrad_mx; bias and residual nullable; y / dx required.  No statistics, no
 * accumulate, no scale_dev.  y8 + sy (dx8 + sdx): nullable, together only, output channel count a multiple of 32, y8 8-byte
 * aligned -- the MX copy of the bf16 values just stored, by the rule of mi355_mx_quantize: e4m3 laid out like y and one E8M0 byte
 * per 32 channels of a pixel ([pixels][C/32] in y's pixel order), i.e. what mi355_mx_quantize(y) would write, without the launch.
 * The dgrad form refuses geometries that leave output pixels without a tap (kernel smaller than the stride).  Every violation
 * fails with MI355_EINVAL before any launch. */
int mi355_conv_fwd_mx_act(const mi355_conv_desc* d, const void* x8, const void* sx, const void* w8, const void* sw, const float* bias,
                          const void* residual, int relu, void* y, void* y8, void* sy, void* stream);
int mi355_conv_dgrad_mx_act(const mi355_conv_desc* d, const void* dy8, const void* sdy, const void* wT8, const void* swT,
                            const float* bias, int relu, void* dx, void* dx8, void* sdx, void* stream);
/* The 3x3 / unit-stride fp8 launches (forward and input gradient) use the variant that stages one operand tile per kernel ROW
 * and reads it shifted for the three taps (a third fewer bytes per MFMA) from `min_tiles` 128x128 output tiles on: 0 never,
 * 1 wherever the shape allows (tests), -1 back to the environment's choice (MI355_FP8_KW3, default 1024).  Returns the previous
 * setting.  Same arithmetic in another summation order (fp32 accumulate). */
long mi355_set_fp8_kw3(long min_tiles);
/* Weight gradient of the K-heavy convs from the fp8 copies of their operands ('fp8' mode; replaces the bf16 mi355_conv_wgrad
 * for the layers of resnet.py:92-107 (Bottleneck conv2, stride 1 and 2), pose_resnet2.py:33-41 (4x4 transposed convs, in
 * conv-form: x = the output gradient, dy = the input) and regda_7.py:4906-4929 whose forward and input gradient already run on
 * fp8 operands): dw[Co][kh][kw][Ci] (fp32) (+)= descale_x * descale_dy * sum_m dy8[m][o] * x8[pixel(m, tap)][c].
 * x8: [N][Hi][Wi][Ci], dy8: [N][Ho][Wo][Co], each e4m3 (format 0) or e5m2 (1); `d` an fp8 descriptor that is either 3x3 /
 * stride 1 / pad 1 with a power-of-two width >= 8, or 3x3 / 4x4 / stride 2 / pad 1 with even extents and a power-of-two output
 * width in [8, 64]; channel counts multiples of 16.  Workspace / accumulate as mi355_conv_wgrad. */
size_t mi355_conv_wgrad_fp8_workspace(const mi355_conv_desc* d);
int mi355_conv_wgrad_fp8(const mi355_conv_desc* d, const void* x8, int x_fmt, const void* dy8, int dy_fmt, const float* descale_x,
                         const float* descale_dy, float* dw, int accumulate, void* ws, size_t ws_bytes, void* stream);
size_t mi355_conv_wgrad_workspace(const mi355_conv_desc* d);
int mi355_conv_wgrad(const mi355_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate,
                     void* ws, size_t ws_bytes, void* stream);
/* Many weight gradients in one call (the layers of one ResNet stage, collected during its backward pass).  Small problems --
 * each offers too few output tiles to fill 256 CUs, so mi355_conv_wgrad splits its pixel range 16..48 ways into fp32 slabs -- are
 * launched TOGETHER (up to 24 per launch, split counts chosen for the group, one grouped slab reduction); problems that have a
 * specialised kernel or fill the chip alone go through mi355_conv_wgrad unchanged.  items: HOST array; results as mi355_conv_wgrad.
 * NOTE: the non-grouped problems reuse `ws` one after the other (stream order), the grouped ones get disjoint regions. */
typedef struct mi355_wgrad_item { mi355_conv_desc d; const void* x; const void* dy; float* dw; int accumulate; int pad_; } mi355_wgrad_item;
size_t mi355_conv_wgrad_grouped_workspace(const mi355_wgrad_item* items, int n);
int mi355_conv_wgrad_grouped(const mi355_wgrad_item* items, int n, void* ws, size_t ws_bytes, void* stream);
/* fp32 master [O][T][I] -> packed `dtype` copies: wf [O][T][Ipad] (cast) and/or wt [Ipad][T][O] (transposed);
 * channels I..Ipad-1 are zero (the 3-channel stem is padded to one 16-byte chunk). */
int mi355_pack_weights(const float* w, void* wf, void* wt, int O, int T, int I, int Ipad, int dtype, void* stream);
/* The same for many weights in one launch (all convs of an optimizer group, right after its step).  items: DEVICE array;
 * blk0 = first block of the item = sum over earlier items of ceil(Ipad/32)*ceil(O/32)*T; total_blocks = that sum over all. */
typedef struct mi355_pack_item { const float* w; void* wf; void* wt; int O, T, I, Ipad, blk0, pad_; } mi355_pack_item;
int mi355_pack_weights_batched(const mi355_pack_item* items_dev, int nitems, int total_blocks, int dtype, void* stream);
/* dbias[C] (=|+=) column sums of dy[rows][C] (bias gradient of the biased head convs). */
size_t mi355_colsum_workspace(long rows, int C);
int mi355_colsum(const void* dy, float* out, long rows, int C, int dtype, int accumulate, void* ws,
                 size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- BatchNorm2d (+ReLU, +residual add)
 * Replace nn.BatchNorm2d (+nn.ReLU, + the residual add of torchvision blocks): 66 instances for
 * ResNet-50; train mode: batch statistics, running-stat update with momentum 0.1 and
 * the UNBIASED variance, eps 1e-5.
 *   y = relu?( (x-mean)*invstd*gamma + beta + residual? )
 * save_mean / save_invstd: fp32 [C] outputs consumed by mi355_bn_bwd.
 * stat_updates: how many times the running-stat momentum update (and num_batches_tracked += 1) is applied: 1 normally;
 *   2 when one forward stands for two identical forwards of the reference (train1.py:405 and :441 run the unchanged
 *   backbone / neck / main head twice on the same target batch).
 * bwd: dy_eff = relu ? dy*(y>0) : dy ; dx = gamma*invstd*(dy_eff - mean(dy_eff) - xhat*mean(dy_eff*xhat));
 *      dresidual (nullable) = dy_eff ; dgamma/dbeta (=|+=).
 *      With relu and y == NULL the mask is recomputed from x (valid when the forward had no residual): one
 *      tensor read less in each backward pass.
 * relu_mask (nullable, all four entry points): [rows][C / chunk] bytes, chunk = 8 (bf16) / 4 (fp32) channels, bit e of a
 *      byte = (y > 0) of channel chunk*chunk_size + e.  The forward writes it; a backward given the mask takes the ReLU
 *      mask from it and reads neither y nor beta: 1/16 of the bytes of y in each of the two backward passes of a
 *      BatchNorm + residual + ReLU (the last BatchNorm of every residual block).
 * q8_out / q8_state (nullable, both or none; bf16 only; 'fp8' compute mode): an fp8 copy of the result written on the side --
 *      forward: q8 = e4m3(y * q8_state[0]), backward: q8 = e5m2(dx * q8_state[0]) -- and max |.| recorded in q8_state[2]
 *      (mi355_fp8_quantize semantics): the consuming fp8 convolution then needs no quantisation pass of its own.
 */
size_t mi355_bn_workspace(long rows, int C);
int mi355_bn_train_fwd(const void* x, const void* residual, void* y, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked,
                       float* save_mean, float* save_invstd, long rows, int C, float eps, float momentum,
                       int stat_updates, int relu, int dtype, void* ws, size_t ws_bytes, void* relu_mask, void* q8_out,
                       float* q8_state, void* stream);
/* mi355_bn_train_fwd without its statistics pass: the partials come from mi355_conv_fwd_stats / _dgrad_stats.
 * scale_shift: 2*C floats of scratch. */
int mi355_bn_train_fwd_partials(const void* x, const void* residual, void* y, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                float* save_mean, float* save_invstd, long rows, int C, float eps, float momentum,
                                int stat_updates, int relu, int dtype, const float* partial, int nslices,
                                float* scale_shift, void* relu_mask, void* q8_out, float* q8_state, void* stream);
int mi355_bn_eval_fwd(const void* x, const void* residual, void* y, const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var, long rows, int C, float eps,
                      int relu, int dtype, void* stream);
int mi355_bn_bwd_partials(const void* dy, const void* x, const void* y, const float* gamma, const float* beta,
                          const float* save_mean, const float* save_invstd, void* dx, void* dresidual, float* dgamma,
                          float* dbeta, int accumulate, long rows, int C, int relu, int dtype, const float* partial,
                          int nslices, float* coeff, const void* relu_mask, void* q8_out, float* q8_state, void* stream);
int mi355_bn_bwd(const void* dy, const void* x, const void* y, const float* gamma, const float* beta,
                 const float* save_mean, const float* save_invstd, void* dx, void* dresidual, float* dgamma, float* dbeta,
                 int accumulate, long rows, int C, int relu, int dtype, void* ws, size_t ws_bytes,
                 const void* relu_mask, void* q8_out, float* q8_state, void* stream);
/* mi355_bn_bwd takes ONE launch when x and dy fit the chip's LDS together (<= ~16.8 MB each on 256 CUs), C is a multiple of
 * 64 (bf16) / 32 (fp32) and the mask does not come from y: each CU keeps its tile of both tensors in LDS between the
 * reduction and the apply pass (3 tensor passes over HBM instead of 5); the blocks exchange their partial sums inside the
 * launch behind a bounded spin.  MI355_BN_RESIDENT=0 keeps the three-launch form.  The one-launch form is only taken when the
 * occupancy query admits one block per CU at the largest LDS size (else the three-launch form runs).  A block whose spin
 * gives up (~0.3 s: another kernel kept a block of the grid off the chip) FAILS LOUDLY: it writes NaN into its rows of dx
 * (and dgamma / dbeta if it owns them) and counts the event.  *out = give-ups since the library was loaded or
 * mi355_bn_resident_reset.  Synchronises.  Callers poll it where they synchronise anyway (train1.py: once per epoch;
 * mi355.ops.bn_resident_check raises). */
int mi355_bn_resident_timeouts(unsigned* out);
/* Clears the give-up count and the exchange's device state (completion counts, granule slots) after a give-up has been
 * handled.  Synchronises the device. */
int mi355_bn_resident_reset(void);
/* TEST HOOK: how often a wave re-reads its share of the exchanged sums before its block gives up (0 restores the default,
 * 1 << 19: a fraction of a second).  Used by the tests to provoke a give-up and check that it is loud. */
int mi355_bn_resident_set_spin_limit(unsigned limit);
/* Run-time switch of the one-launch backward (1 on, 0 off, -1 back to the environment's choice); returns the previous value.
 * Switch it off while another kernel runs beside the backward on the same device (e.g. a collective overlapped with it): all
 * blocks of the one-launch form must be resident at once.  For the same reason two PROCESSES that share a GPU must not both use it
 * (train1.py / bench.py set MI355_BN_RESIDENT=0 when ranks share a device); a launch whose blocks could not all become resident
 * gives up after about 0.3 s, poisons its outputs with NaN and is counted by mi355_bn_resident_timeouts. */
int mi355_bn_set_resident(int on);
/* g <- (bit of relu_mask set) ? g : 0 in place; g [rows][C] bf16 / fp32, relu_mask as above.  The stand-alone form of what
 * mi355_conv_dgrad_masked_acc and mi355_bn_bwd (relu_mask) do on the fly: a residual block's last BatchNorm hands the
 * UNMASKED dy on to the other branch (no dresidual write) together with its bit mask (mi355/nn.py _LAZY_MASK). */
int mi355_apply_relu_mask(void* g, const void* relu_mask, long rows, int C, int dtype, void* stream);

/* Stem: BatchNorm (statistics partials from the conv epilogue, as mi355_bn_train_fwd_partials) + ReLU + MaxPool2d(3, 2, 1) in
 * one pass over the conv output: resnet.py:27-28 (`bn1`, `relu`, `maxpool` of the torchvision stem).  y_pool [N][Ho][Wo][C],
 * argidx as mi355_maxpool_fwd writes it (its backward: mi355_maxpool_bwd, then mi355_bn_bwd with relu = 1 and y = NULL). */
int mi355_bn_relu_maxpool_fwd_partials(const void* x, void* y_pool, uint8_t* argidx, const float* gamma, const float* beta,
                                       float* running_mean, float* running_var, int64_t* nbt, float* save_mean,
                                       float* save_invstd, int N, int H, int W, int C, float eps, float momentum,
                                       int stat_updates, int dtype, const float* partial, int nslices, float* scale_shift,
                                       void* stream);

/* ---------------------------------------------------------------- stem max-pool 3x3 s2 p1
 * Replaces nn.MaxPool2d(3,2,1) of the torchvision stem (uda/model/resnet.py:28).  argidx: uint8 window
 * position (first maximum in (kh,kw) scan order, as ATen) kept for the backward gather. */
int mi355_maxpool_fwd(const void* x, void* y, uint8_t* argidx, int N, int H, int W, int C, int dtype,
                      void* stream);
int mi355_maxpool_bwd(const void* dy, const uint8_t* argidx, void* dx, int N, int H, int W, int C, int dtype,
                      void* stream);

/* ---------------------------------------------------------------- layout changes at the API edge */
/* image / feature NCHW fp32 -> NHWC `dtype` with channels zero-padded to Cpad (stem input). */
int mi355_nchw_to_nhwc(const float* x, void* y, int N, int C, int H, int W, int Cpad, int dtype, void* stream);
/* The stem (resnet.py:23-28: Conv2d(3, 64, 7, stride 2, padding 3)) as a 4x4 / unit-stride conv over the image folded 2x2 into
 * channels: y [N][H/2][W/2][16] `dtype`, folded channel (dy*2 + dx)*4 + c (c = 3 zero), H and W even.  The conv then runs through
 * mi355_conv_fwd* / mi355_conv_wgrad with the descriptor {Hi = H/2, Wi = W/2, Ci = 16, kh = kw = 4, stride 1, pad 2, Ho = H/2,
 * Wo = W/2}: those entry points accept the top-left Ho x Wo crop of a unit-stride conv's output.  K = 256 instead of 49 x 8 = 392. */
int mi355_nchw_to_s2d(const float* x, void* y, int N, int H, int W, int dtype, void* stream);
/* stem weights fp32 [Co][7][7][3] -> folded forward operand `dtype` [Co][4][4][16]; and the folded weight gradient fp32
 * [Co][4][4][16] back onto g fp32 [Co][7][7][3] (g = / += per `accumulate`). */
int mi355_stem_s2d_pack(const float* w, void* out, int Co, int dtype, void* stream);
int mi355_stem_s2d_unpack_grad(const float* gs, float* g, int Co, int accumulate, void* stream);
/* NHWC `dtype` -> NCHW fp32 (the feature map `f` returned by PoseResNetx9.forward, regda_7.py:4944). */
int mi355_nhwc_to_nchw(const void* x, float* y, int N, int C, int H, int W, int dtype, void* stream);

/* ---------------------------------------------------------------- 21-channel pointwise convs
 * The 1x1 convs touching the K=21 heat-map tensors (regda_7.py:4916-4922 heads' last conv,
 * :4513 / :4588 heatmap_conv).  Heat-maps y are NCHW fp32 [N][K][HW]; features x are NHWC [N*HW][C].
 *  c2k : y[n][k][p] (=) bias[k] + sum_c x[n*HW+p][c] * w[k][c]          (w fp32 [K][C])
 *  k2c : out[n*HW+p][c] (=|+=residual) bias[c] + sum_k y[n][k][p]*w[c][k], times *scale_dev (w fp32 [C][K])
 *  wgrad: dw[K][C] (kc_layout=1) or dw[C][K] (kc_layout=0) (=|+=) sum_{n,p} y[n][k][p] * x[n*HW+p][c]
 *  rowsum: out[k] (=|+=) sum_{n,p} y[n][k][p]                             (bias gradient)
 *  w_transposed!=0: w is stored the other way round ([C][K] for c2k, [K][C] for k2c), which is how the
 *  input-gradient of each op reuses the other op with the same weight tensor.
 */
/* MFMA form of c2k (forward of the heads' last conv): w is the packed `dtype` copy [K][C]; K <= 32, C/chunk a power of 2. */
int mi355_conv1x1_heatmap(const void* x, const void* w, const float* bias, float* y, int N, int HW, int C, int K,
                          int dtype, void* stream);
int mi355_pw_c2k(const void* x, const float* w, const float* bias, float* y, int N, int HW, int C, int K,
                 int w_transposed, int dtype, void* stream);
int mi355_pw_k2c(const float* y, const float* w, const float* bias, const void* residual,
                 const float* scale_dev, void* out, int N, int HW, int C, int K, int w_transposed, int dtype,
                 void* stream);
/* mi355_pw_k2c with the BatchNorm statistics of its output from the epilogue (the BN in front of `last_lay`, regda_7.py:4551-4561):
 * partial[N * ceil(HW/64)][C][n, mean, M2], consumed by mi355_bn_train_fwd_partials */
int mi355_pw_k2c_stats(const float* y, const float* w, const float* bias, const void* residual, const float* scale_dev,
                       void* out, int N, int HW, int C, int K, int w_transposed, int dtype, float* partial,
                       size_t partial_bytes, int* nslices, void* stream);
size_t mi355_pw_wgrad_workspace(int N, int HW, int C, int K);
int mi355_pw_wgrad(const void* x, const float* y, float* dw, int kc_layout, int accumulate, int N, int HW,
                   int C, int K, int dtype, void* ws, size_t ws_bytes, void* stream);
int mi355_hm_rowsum(const float* y, float* out, int accumulate, int N, int K, int HW, void* ws, size_t ws_bytes,
                    void* stream); /* ws: >= N*K floats */

/* ---------------------------------------------------------------- heat-map decode / losses (rows = B*K maps)
 * argmax2d: utils/keypoint_detection.py:7-35 get_max_preds — first maximum (np.argmax tie rule, NaN
 *   counts as maximum), x = idx % W, y = floor(idx / W), both zeroed when max <= 0.  Bit-exact.
 * softargmax: utils/keypoint_detection.py:209-239 — softmax(beta*hm), (E[col], E[row]) * out_scale.
 */
int mi355_argmax2d(const float* hm, int32_t* idx, float* xy, float* maxval, int rows, int H, int W,
                   void* stream);
int mi355_softargmax(const float* hm, float* uv, int rows, int H, int W, float beta, float out_scale,
                     void* stream);
/* KL loss, uda/model/loss.py:145-158: per row r
 *   logp = log_softmax(pred[r]); t = (target[r]+eps)/sum(target[r]+eps);
 *   loss_rows[r] = weight[r] * sum_j xlogy-style t_j*(log t_j - logp_j)   (0 where t_j==0)
 *   unit_grad[r][j] (nullable) = weight[r]*inv_count * (softmax_j*sum(t) - t_j)   = d(mean loss)/d pred
 */
int mi355_kl_heatmap(const float* pred, const float* target, const float* weight, float eps,
                     float* loss_rows, float* unit_grad, int rows, int HW, float inv_count, void* stream);
/* Coordinate loss on a differentiable soft-arg-max, one launch.  The soft-arg-max is utils/keypoint_detection.py:209-239; the
 * loss on it is NOT in the reference: it is the integral-regression loss of Sun et al., ECCV 2018, trained beside
 * the heat-map loss.  pred [rows][H][W] fp32, coord [rows][2] = (x, y) in heat-map pixels, weight [rows] (nullable: all ones).
 * Per row r, x_i = i % W, y_i = i / W:
 *   m = max_i beta*z_i; e_i = expf(beta*z_i - m); s = sum e_i; p_i = e_i / s
 *   u = sum p_i x_i; v = sum p_i y_i;  uv[r] (nullable) = (u, v)        (= mi355_softargmax with out_scale 1)
 *   dx = u - coord[r][0]; dy = v - coord[r][1]
 *   h(d)  = delta > 0 ? (|d| < delta ? 0.5 d^2 / delta : |d| - 0.5 delta) : |d|     (torch smooth_l1_loss(beta=delta); 0: L1)
 *   h'(d) = delta > 0 ? (|d| < delta ? d / delta : sign(d)) : sign(d)                (sign(0) = 0)
 *   loss_rows[r] = w_r * (h(dx) + h(dy))
 *   unit_grad[r][i] (nullable) = coef * w_r * beta * p_i * ((x_i - u) h'(dx) + (y_i - v) h'(dy))
 * coef = the term's coefficient / rows: the scalar loss is mi355_reduce_sum(loss_rows, coef) and unit_grad its gradient.
 * A row with w_r == 0 is skipped by selection: loss 0 and a gradient row of exact zeros whatever pred[r] and coord[r] hold (NaN
 * and inf included; an invisible joint's coordinates mean nothing); uv[r] is still written.  In a weighted row a NaN of pred or
 * coord reaches that row's loss and its whole gradient row, and no other row.  No atomics, fixed summation order.
 * MI355_EINVAL: null pred / coord / loss_rows; rows, H or W < 1; H*W >= 2^31; beta not finite or <= 0; delta NaN, inf or < 0;
 * coef not finite. */
int mi355_coord_heatmap(const float* pred, const float* coord, const float* weight, float beta, float delta, float coef,
                        float* loss_rows, float* unit_grad, float* uv, int rows, int H, int W, void* stream);
/* Backward of the soft-arg-max for an arbitrary upstream gradient, one launch (NOT in the reference, whose soft-arg-max is
 * forward-only).  pred [rows][H][W] fp32, g_uv [rows][2] = d loss / d (u, v), grad [rows][H][W].  With m, e_i, s, p_i, u, v
 * exactly as mi355_coord_heatmap defines them (the forward is mi355_softargmax with out_scale 1):
 *   grad[r][i] = beta * p_i * ((x_i - u) * g_u + (y_i - v) * g_v)
 * A row whose g_u and g_v are both exactly 0 is skipped by selection: a row of +0 whatever pred[r] holds (NaN and inf included;
 * the map is not read).  Elsewhere a NaN of pred[r] or g_uv[r] reaches the whole of grad[r] and no other row.  Same forms as
 * mi355_coord_heatmap (register-resident with 16-byte stores at 64 x 64, 32 x 32 and 16 x 16 when pred and grad are 16-byte
 * aligned, a loop form otherwise).  No atomics, fixed summation order, no allocation.
 * MI355_EINVAL: null pred / g_uv / grad; rows, H or W < 1; H*W >= 2^31; beta not finite or <= 0. */
int mi355_softargmax_backward(const float* pred, const float* g_uv, float beta, float* grad, int rows, int H, int W, void* stream);
/* Bone-ratio skeleton prior (NOT in the reference; in the family of the bone-length-ratio constraint of Zhou et al., ICCV 2017:
 * PAPERS.md).  The skeleton is a table bones = int32 [E][2] of (parent, child) joint indices in device memory; an entry outside
 * [0, K) is no bone.  uv [B][K][2] fp32, weight [B][K] (nullable: all joints visible), mean / var [E] fp32 and seen [E] int32:
 * the running statistics of mi355_bone_stats_update.  fp64 arithmetic on the fp32 operands, every product and sum rounded on its
 * own, every sum in ascending bone order, one rounding to fp32 at each store.  Per sample b:
 *   bone e = (p, c) is present iff w[p] > 0 && w[c] > 0 && seen[e];  d_e = uv[c] - uv[p];  l_e = sqrt(dx*dx + dy*dy)
 *   n = number of present bones, S = sum of their l_e.  n < 2 || S == 0: the sample is skipped (loss 0, gradient rows exactly 0)
 *   lbar = S / n;  r_e = l_e / lbar;  sd_e = sqrt(var_e + eps);  z_e = (r_e - mean_e) / sd_e;  h_e = max(|z_e| - margin, 0)
 *   loss_rows[b] = (sum_e 0.5 * h_e^2) / n
 *   q_e = h_e * sign(z_e) / (n * sd_e);  Q = (sum_e q_e * r_e) / n;  gl_e = (q_e - Q) / lbar
 *   t_e = (coef * gl_e / l_e) * d_e  (nothing for l_e == 0);  g_uv[b][c] += t_e;  g_uv[b][p] -= t_e        (g_uv nullable)
 * coef = the term's coefficient / B: the scalar loss is mi355_reduce_sum(loss_rows, coef) and g_uv its gradient w.r.t. uv.
 * The loss does not change under a rotation, a scaling or a shift of the sample's points.  A NaN coordinate of a present bone
 * reaches that sample's loss and gradient and no other sample's.
 * MI355_EINVAL: null uv / bones / mean / var / seen / loss_rows; B < 1 or > MI355_BONE_MAX_BATCH; K < 2 or >
 * MI355_BONE_MAX_JOINTS; E < 1 or > MI355_BONE_MAX_BONES; margin not finite or < 0; eps not finite or <= 0; coef not finite. */
#define MI355_BONE_MAX_JOINTS 32
#define MI355_BONE_MAX_BONES 32
#define MI355_BONE_MAX_BATCH 4096
int mi355_bone_prior(const float* uv, const float* weight, const int* bones, const float* mean, const float* var, const int* seen,
                     float margin, float eps, float coef, float* loss_rows, float* g_uv, int B, int K, int E, void* stream);
/* Running statistics of the bone ratios, one launch of one workgroup, fp64.  kp [B][K][2], weight [B][K] (nullable).  r_e^b as
 * above, except that presence ignores `seen`; skipped samples are left out.  For every bone that c_e >= 1 samples show: m_e =
 * the mean and v_e = the biased variance (about m_e) of its ratios, samples in ascending order.  seen[e] == 0: mean = m, var =
 * v, seen = 1; else mean = (1 - rho) * mean + rho * m and likewise var.  A bone with c_e == 0 is not touched.  All three arrays
 * are updated in place on the device, so a captured launch handles the first batch like any other.
 * MI355_EINVAL: null kp / bones / mean / var / seen; shapes as above; rho outside [0, 1] or NaN. */
int mi355_bone_stats_update(const float* kp, const float* weight, const int* bones, float* mean, float* var, int* seen, float rho,
                            int B, int K, int E, void* stream);
/* out[0] = scale * sum(in[0..n)) in a fixed order (deterministic). */
int mi355_reduce_sum(const float* in, float* out, int n, float scale, void* stream);
/* out[i] = in[i] * (*g_dev) : backward of the KL loss (upstream scalar gradient on device). */
int mi355_scale_by_dev(const float* in, const float* g_dev, float* out, long n, void* stream);
/* out[i] = in[i] * (*g_dev) on a feature tensor (dtype MI355_F32 / MI355_BF16, n a multiple of one 16-byte chunk):
 * backward of utils/gl.py:8-18 (GradientFunction: grad * coeff) for consumers that cannot fold lambda into their own
 * input-gradient epilogue. */
int mi355_scale_feature(const void* in, const float* g_dev, void* out, long n, int dtype, void* stream);
/* Pseudo labels from arg-max coordinates xy[B*K][2] (of the 64x64-level main prediction):
 *   centre = trunc(xy / div); gt = clipped Gaussian patch (patch[(2r+1)^2], host table) at centre on an
 *   S x S map.  regda_4.py:76-86 (div 1, r 6), regda_7.py:3026-3039 (div 4, r 3), :3188-3201 (div 2, r 4).
 * kind: 0 base  : gf = clip(sum_{j!=k} gt_j, 0, 1)                                   (regda_4.py:83-84)
 *       1 x1/x5 : gf = clip(1 - 10 gt, 0, 1)                                         (regda_7.py:3255-3256)
 *       2 x6    : gf = clip(clip(sum_k gt_k,0,1) - 10 gt, 0, 1)                      (regda_7.py:3614-3616)
 * extra (nullable, [B*K][S*S]): gf = clip(gf + extra - 100 gt, 0, 1)                 (:3542-3544, :3618-3620)
 *                a non-finite extra behaves as under torch.clip / torch.max: +-inf clips to 1 / 0, a NaN stays in its
 *                pixel and, with normalise==1, makes its whole map NaN (normalise==2 leaves that map unscaled)
 * normalise==1 : gf /= max(gf) per map (0/0 -> NaN as in the reference)              (:3546-3548, :3623-3625)
 * normalise==2 : the same, but a map whose maximum is 0 is left at zero (synthetic-noise benchmarks: collapsed target
 *                predictions make such maps after a few dozen iterations; not the reference's behaviour)
 * gt / gf outputs nullable.
 */
int mi355_pseudo_label(const float* xy, const float* patch, int radius, int div, int S, int kind,
                       const float* extra, int normalise, float* gt, float* gf, int B, int K, void* stream);
/* nn.Upsample(size, mode='bilinear') (align_corners=False) on [rows][h][w] -> [rows][H][W];
 * out = alpha*up(in) + (accumulate ? out : 0)   (train1.py:410-424: target5 = 0.5*up(adv3) + up(adv2)). */
int mi355_bilinear_up(const float* in, float* out, int rows, int h, int w, int H, int W, float alpha,
                      int accumulate, void* stream);
/* PCK pieces of utils/keypoint_detection.py:38-92 on device: dist[B*K] = |pred-tgt| / (side/10) or -1. */
int mi355_pck_dists(const float* pred_xy, const float* tgt_xy, float* dists, int rows, float norm_x,
                    float norm_y, void* stream);

/* ---------------------------------------------------------------- evaluation at image resolution (csrc/eval.hip)
 * upsample_argmax: utils/keypoint_detection.py:172-205 (compute_uv_from_heatmaps2) in one launch.  The arg-max of the VIRTUAL
 *   map nn.Upsample(size=(H,W), mode='bilinear') (align_corners=False; index / weight rule and expression order of
 *   mi355_bilinear_up) of hm[rows][h][w], reduced by mi355_argmax2d's rules: first maximum in row-major order of the H x W grid,
 *   NaN counts as maximum, x = idx % W, y = idx / W, both zeroed when the maximum is <= 0, maxval = the value at idx.  Nothing of
 *   rows*H*W elements is allocated or written.  Any h, w, H, W >= 1 (H*W < 2^31); H == h and W == w is mi355_argmax2d itself.
 *   idx / xy / maxval nullable; pointers need 4-byte alignment only (16-byte loads where hm and h*w allow). */
int mi355_upsample_argmax(const float* hm, int32_t* idx, float* xy, float* maxval, int rows, int h, int w, int H, int W,
                          void* stream);
/* pose_metrics: the accumulation behind EPE (accuracy_2d, :128-136) and the PCK curve / AUC (the threshold loop of accuracy_3d,
 *   :95-126) on pred_xy, gt_xy [B][K][2] and vis [B][K].  sum_err[K], count[K], hits[K][T] are persistent DEVICE accumulators the
 *   caller zeroes; every call adds to them.  Per joint k, for b = 0 .. B-1 in that order, where vis[b][k] > 0:
 *     e = sqrt(dx^2 + dy^2) in float64 from the fp32 inputs;  sum_err[k] += e;  count[k] += 1;  hits[k][t] += (e < (double)thr[t])
 *   (strict).  The float64 sum is sequential in b: the same bits whether a data set arrives in one batch or in many. */
int mi355_pose_metrics(const float* pred_xy, const float* gt_xy, const float* vis, const float* thr, int T, int B, int K,
                       double* sum_err, int32_t* count, int32_t* hits, void* stream);
/* mirror_batch: the input half of the flip test of Simple Baselines / HRNet (lib/core/function.py validate(), TEST.FLIP_TEST:
 *   `input_flipped = np.flip(input, 3)`), for ONE forward of 2B images.  x [B][C][H][W] fp32 contiguous; out has room for 2B
 *   images: out[b] = x[b], out[B+b][c][y][X] = x[b][c][y][W-1-X].  One launch, 16-byte accesses when W % 4 == 0 and both
 *   pointers are 16-byte aligned, any W >= 1 otherwise.  x and out must not overlap. */
int mi355_mirror_batch(const float* x, float* out, int B, int C, int H, int W, void* stream);
/* flip_decode: the output half of that flip test and the sub-pixel decodes of the same code bases, one workgroup per map
 *   hm[rows][h][w].  The working map m is hm, or with hm_flip (the heat-maps of the mirrored image)
 *     m[y][x] = 0.5f * (hm[y][x] + f[y][x]),  f[y][x] = hm_flip[y][w-1-x]                      (shift 0)
 *                                             f[y][x] = hm_flip[y][w-x], f[y][0] = hm_flip[y][w-1]   (shift 1)
 *   (function.py `(output + output_flipped) * 0.5` after flip_back; shift 1 is its TEST.SHIFT_HEATMAP
 *   `output_flipped[:, :, :, 1:] = output_flipped.clone()[:, :, :, 0:-1]`), sum and product rounded separately.  avg_out
 *   (nullable) receives m.  The arg-max of m follows mi355_argmax2d (first maximum, NaN counts as maximum; idx, maxval as there,
 *   nullable); at the arg-max (px, py), in heat-map pixels:
 *     mode 0  no offset;
 *     mode 1  get_final_preds (lib/core/inference.py): 0.25 * sign(m[py][px+1] - m[py][px-1]) where 1 <= px <= w-2, likewise in
 *             y; sign(0) = 0, a NaN difference gives 0;
 *     mode 2  the second-order Taylor step of DARK (Zhang et al., CVPR 2020, "Distribution-Aware Coordinate Representation for
 *             Human Pose Estimation", eq. 8-10; mmpose post_dark_udp / its taylor()) where 2 <= px <= w-3 and 2 <= py <= h-3:
 *             S = m smoothed by the separable taps[0 .. 2*radius] (zero padding; fp32, for dy ascending: row = sum over dx
 *             ascending of taps[dx+radius] * m, tot += taps[dy+radius] * row, every product and sum rounded on its own) at the
 *             13 points (0,0), (+-1,0), (+-2,0), (0,+-1), (0,+-2), (+-1,+-1); then in float64 L = log(max(S, 1e-10)),
 *             gx = (L(1,0) - L(-1,0)) / 2, dxx = (L(2,0) - 2 L(0,0) + L(-2,0)) / 4 (gy, dyy likewise),
 *             dxy = (L(1,1) - L(-1,1) - L(1,-1) + L(-1,-1)) / 4, det = dxx dyy - dxy^2, and where det != 0 and both are finite
 *             ox = -(dyy gx - dxy gy) / det, oy = -(dxx gy - dxy gx) / det.  DARK's renormalisation of S to the maximum of m
 *             adds one constant to every L and cancels; it is left out.  radius 1..16; taps is not read in modes 0, 1.
 *   xy = ((float)(px + ox) * scale_x, (float)(py + oy) * scale_y), (0, 0) unless maxval > 0.  hm_flip == NULL, mode 0, scales 1:
 *   mi355_argmax2d's bits.  The map is staged in LDS up to 64 KB and read through the caches above; no workgroup waits on
 *   another.  Pointers need 4-byte alignment only. */
int mi355_flip_decode(const float* hm, const float* hm_flip, int shift, float* avg_out, int mode, const float* taps, int radius,
                      float scale_x, float scale_y, int32_t* idx, float* xy, float* maxval, int rows, int h, int w, void* stream);

/* ---------------------------------------------------------------- optimiser
 * torch.optim.SGD(momentum, weight_decay, nesterov=True) of train1.py:141-148 over a flat fp32 range:
 *   g' = g + wd*p ; buf = momentum*buf + g' ; p -= lr * (nesterov ? g' + momentum*buf : buf)
 * lr read from *lr_dev.  p_lowp (nullable): bf16 copy of the updated parameters (same flat layout).
 */
int mi355_sgd_nesterov(float* p, const float* g, float* buf, long n, const float* lr_dev, float momentum,
                       float wd, int nesterov, void* p_lowp, void* stream);
int mi355_cast_f32(const float* in, void* out, long n, int dtype, void* stream);
/* EMA ("mean teacher") update of uda/model/loss.py:252-261 (update_ema_variables5, the call at train1.py:461) over a flat
 * fp32 range:   e = fl(fl(e * k) + fl(p * c)),   k = coef_dev[0] = float32(m), c = coef_dev[1] = float32(1.0 - m)
 * -- torch's `v_ema * m + (1. - m) * v_main` bit for bit: two multiplies and one add, never contracted.  p is only read.
 * e and p 16-byte aligned (the mirror of a FusedSGD group and the group's parameter buffer). */
int mi355_ema_update(float* e, const float* p, long n, const float* coef_dev, void* stream);
/* The same for many tensors in one launch (BatchNorm running statistics, parameters outside flat storage, the
 * num_batches_tracked counters).  items: DEVICE array; kind MI355_EMA_F32: dst = EMA of n floats, MI355_EMA_COPY64: dst = src for
 * n 64-bit words (`v_ema.copy_(v_main)`); pointers need their element's natural alignment only.  blk0 = first block of the
 * item = sum over earlier items of ceil(n / MI355_EMA_CHUNK); total_blocks = that sum over all. */
#define MI355_EMA_CHUNK 2048
#define MI355_EMA_F32 0
#define MI355_EMA_COPY64 1
typedef struct mi355_ema_item { const void* src; void* dst; long n; int kind; int blk0; } mi355_ema_item;
int mi355_ema_update_batched(const mi355_ema_item* items_dev, int count, int total_blocks, const float* coef_dev, void* stream);
/* Global gradient-norm clipping with a non-finite step guard, on the device (no host read between backward and step; all three
 * entry points capture).  torch.nn.utils.clip_grad_norm_(params, max_norm) followed by the optimizer step, except that the
 * scale is applied inside the SGD kernel: the gradients themselves are never written.
 *   mi355_grad_sumsq_batched: items = DEVICE array of gradient ranges (g 16-byte aligned, n >= 1 floats; blk0 = first block of the
 *     item = sum over earlier items of ceil(n / MI355_GN_CHUNK); total_blocks = that sum over all).  Block b owns one
 *     MI355_GN_CHUNK slice of its item and writes  partials[b] = sum (double)g * (double)g  over it: every lane accumulates its
 *     elements in index order in fp64, the lanes are folded by a fixed xor tree, the four waves in wave order.  No atomics:
 *     the same bytes give the same bits, eagerly or replayed.  Nothing outside [g, g + n) of any item is read.
 *   mi355_grad_clip_coef: ONE block folds partials[0 .. total_blocks) (lane-strided, then the same tree) and fills the record:
 *       sumsq = the fp64 sum;  norm = (float)sqrt(sumsq), the fp64 root rounded once;
 *       coef  = fminf(1.0f, max_norm / (norm + 1e-6f))   in fp32 (torch: max_norm / (total_norm + 1e-6), clamp(max=1.0));
 *       sumsq not finite:  skip = 1, coef = 0, n_skipped += 1;  else skip = 0.
 *     max_norm is an INPUT field: the host writes it (outside capture); +inf measures and guards without ever scaling.
 *   mi355_sgd_nesterov_clipped: mi355_sgd_nesterov on g_c = fl32(g * rec->coef) -- the product is rounded on its own, never
 *     contracted into the weight-decay multiply-add, so coef == 1.0f gives the bits of mi355_sgd_nesterov.  With rec->skip set
 *     the launch writes nothing: p, buf and p_lowp keep their values (a skipped GradScaler step).  g is only read. */
#define MI355_GN_CHUNK 16384        /* floats per block */
typedef struct mi355_gn_item { const float* g; long n; int blk0; int pad; } mi355_gn_item;
typedef struct mi355_clip_rec { double sumsq; float max_norm; float norm; float coef; int skip; long long n_skipped; } mi355_clip_rec;
int mi355_grad_sumsq_batched(const mi355_gn_item* items_dev, int count, int total_blocks, double* partials_dev, void* stream);
int mi355_grad_clip_coef(const double* partials_dev, int total_blocks, mi355_clip_rec* rec_dev, void* stream);
int mi355_sgd_nesterov_clipped(float* p, const float* g, float* buf, long n, const float* lr_dev, const mi355_clip_rec* rec_dev,
                               float momentum, float wd, int nesterov, void* p_lowp, void* stream);
/* Adam / AdamW over many parameters in two launches (mi355.optim.FusedAdam): torch.optim.Adam / AdamW of the installed torch,
 * torch/optim/adam.py `_single_tensor_adam` with amsgrad, maximize, capturable and differentiable off, which does per parameter
 *     step_t += 1
 *     weight_decay != 0:  decoupled ? param.mul_(1 - lr * weight_decay) : grad = grad.add(param, alpha=weight_decay)
 *     exp_avg.lerp_(grad, 1 - beta1)
 *     exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
 *     bias_correction1 = 1 - beta1 ** step;  bias_correction2 = 1 - beta2 ** step          (Python floats: fp64)
 *     step_size = lr / bias_correction1;     bias_correction2_sqrt = bias_correction2 ** 0.5
 *     denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
 *     param.addcdiv_(exp_avg, denom, value=-step_size)
 * Here: items = DEVICE array, one item per parameter about to be stepped (p, g, m, v 16-byte aligned, n >= 1 floats each; blk0 =
 * first block of the item = sum over earlier items of ceil(n / MI355_ADAM_CHUNK); total_blocks = that sum over all).  Block b owns
 * one MI355_ADAM_CHUNK slice of its item (256 threads, a float4 per lane, a scalar tail; no atomics) and computes once, in fp64,
 * from t = *step + 1 and lr = *item.lr:
 *     bc1 = 1 - beta1^t;  bc2s = sqrt(1 - beta2^t);  step_size = fl32((double)lr / bc1);  bc2s_f = fl32(bc2s);
 *     decay = fl32(1 - (double)lr * wd)
 * then per element in fp32, every operation rounded on its own (nothing is contracted into an FMA), divide and square root
 * correctly rounded:
 *     gc = rec ? fl32(g * rec->coef) : g
 *     decoupled ? p *= decay : gc = gc + wd * p          (the second only when wd != 0)
 *     m = m + (1 - beta1) * (gc - m)
 *     v = beta2 * v + (1 - beta2) * gc * gc              (((1 - beta2) * gc) * gc, the order of addcmul_)
 *     p = p - step_size * (m / (sqrt(v) / bc2s_f + eps))
 * The betas travel as fp64, as torch keeps them: beta^t and 1 - beta are formed in fp64 ((1 - beta) and beta2 are then rounded to
 * fp32 once, as torch's scalar arguments are) -- from an fp32 beta2 = 0.999 both 1 - beta2 and 1 - beta2^t at small t would be off
 * by 3e-5 of their value.  Differences from torch: lr is an fp32 value on the device (rounded before the division), and lerp_ is
 * always the form above (torch switches to  gc - (gc - m) * beta1  when 1 - beta1 >= 0.5).  With rec->skip set the
 * launch writes nothing: p, m and v keep their bits; rec->coef == 1.0f gives the bits of the rec == NULL launch.  g, step and lr
 * are only read, nothing outside [x, x + n) of any item is touched, and blocks of one parameter never race on its step count:
 * mi355_adam_tick_batched, one tiny launch BEHIND the step, does  *step += 1  for every item unless rec->skip.  The counts are
 * fp32 (torch's state_dict dtype): exact up to 2^24 steps.  Host validation happens before any launch (null table, count < 1,
 * total_blocks < 1 or < count, table not 8-byte aligned, record not 8-byte aligned).  Never allocates; capturable. */
#define MI355_ADAM_CHUNK 16384      /* floats per block */
typedef struct mi355_adam_item {
  float* p; const float* g; float* m; float* v;      /* 16-byte aligned, n >= 1 floats each */
  float* step;                                       /* this parameter's step count, one fp32 on the device */
  const float* lr;                                   /* its group's learning rate, one fp32 on the device */
  long n; double beta1, beta2;                       /* fp64, as torch keeps them: see above */
  float eps, wd; int decoupled; int blk0;
} mi355_adam_item;
int mi355_adam_step_batched(const mi355_adam_item* items_dev, int count, int total_blocks,
                            const mi355_clip_rec* rec_dev /* NULL: no clipping */, void* stream);
int mi355_adam_tick_batched(const mi355_adam_item* items_dev, int count,
                            const mi355_clip_rec* rec_dev /* NULL */, void* stream);

/* ---------------------------------------------------------------- mean-teacher consistency (csrc/teacher.hip)
 * Eval-mode BatchNorm folded into the conv in front of it, for many (conv, bn) pairs in ONE launch and into caller-owned
 * storage: the device form of mi355/nn.py's _fold_scale_shift + multiply, which the teacher of train1.py:364 / :461 needs
 * once per iteration (its weights move with every EMA update).  Per item, with c the channel of an element:
 *   scale[c]    = gamma[c] / sqrtf(var[c] + eps)                       (correctly rounded divide and square root)
 *   out_bias[c] = fl(beta[c] - fl(mean[c] * scale[c]))                 (+ fl(conv_bias[c] * scale[c]) when conv_bias is given)
 *   out_w[e]    = fl(w[e] * scale[c(e)])                               w, out_w: fp32 in memory order [O][T][I]
 * axis 0: c(e) = e / (T * I), C = O (a conv);  axis 1: c(e) = e % I, C = I (the conv-form of a transposed conv).  Nothing is
 * contracted into an FMA.  blk0 = first block of the item = sum over earlier items of ceil(O*T*I / MI355_FOLD_CHUNK);
 * total_blocks = that sum over all.  As with mi355_augment the records are passed twice: `items_host` (host memory) is what the
 * argument checks read before anything is enqueued, `items_dev` (an identical copy in device memory) is what the kernel reads.
 * Pointers need 4-byte alignment only (16-byte accesses are used where w and out_w allow).  Never allocates; capturable. */
#define MI355_FOLD_CHUNK 2048
typedef struct mi355_fold_item {
  const float* w; const float* gamma; const float* beta; const float* mean; const float* var;
  const float* conv_bias;      /* nullable */
  float* out_w; float* out_bias;
  float eps; int O, T, I, axis, blk0;
} mi355_fold_item;
int mi355_bn_fold_batched(const mi355_fold_item* items_host, const mi355_fold_item* items_dev, int count, int total_blocks,
                          void* stream);
/* mt_loss of uda/model/loss.py:265-297 (MSELoss over the joint subset its curriculum selects; the weight `m` of
 * train1.py:351-353 rides in grad_scale) on fp32 NCHW heat-maps pred, target [B][K][HW], K <= 32, HW >= 1.  rec: DEVICE record
 * (refreshed per epoch without recapturing a graph).  Row r = b * K + k:
 *   rows[r]         = sum_j fl(fl(p_j - t_j)^2) in a fixed order          (exactly 0 when bit k of joint_mask is clear)
 *   unit_grad[r][j] = fl(fl(p_j - t_j) * grad_scale)   (nullable)         (exactly 0 when bit k of joint_mask is clear)
 * The scalar loss is mi355_reduce_sum(rows) times a device-resident m / n (mi355_scale_by_dev). */
typedef struct mi355_mse_rec { int32_t joint_mask; float grad_scale; } mi355_mse_rec;
int mi355_mse_heatmap(const float* pred, const float* target, const mi355_mse_rec* rec_dev, float* rows, float* unit_grad,
                      int B, int K, int HW, void* stream);

/* ---------------------------------------------------------------- MMD alignment (csrc/mmd.hip)
 * MMD_loss3 of uda/model/loss.py:1061-1104 (per joint, the multi-Gaussian-kernel MMD between a batch of source and a batch of
 * target heat-maps; with K = 1 the MMD_loss / mmd_rbf of uda/model/loss.py:1107-1196 on (n, D) features) and its gradient, on
 * fp32 source, target [B][K][HW] (row (b, k) contiguous; the same B on both sides), without the n x n x HW temporaries of the
 * reference's expression.  n = 2 B <= MI355_MMD_MAX_ROWS; rows x_0 .. x_{n-1} of joint k are source[0..B)[k], then
 * target[0..B)[k].  Three launches (two when both gradient pointers are null):
 *   mmd_dist  D[k][i][j] = sum_p (x_i[p] - x_j[p])^2, the difference form; every unordered pair once, written to both places
 *             (D symmetric bit for bit), D[k][i][i] = 0; into `work`
 *   mmd_coef  bw = sum_ij D_ij / (n^2 - n), or fix_sigma when fix_sigma > 0;  bw /= kernel_mul^(kernel_num / 2);
 *             bw_m = bw * kernel_mul^m, m < kernel_num;  Kmat_ij = sum_m exp(-D_ij / bw_m);
 *             loss_rows[k] = (1 / B^2) sum_{a,b<B} ((Kmat[a][b] + Kmat[B+a][B+b]) - Kmat[a][B+b]) - Kmat[B+a][b];
 *             `work` is overwritten with c_ij = s_ij * scale / (B^2 K) * sum_m (-1 / bw_m) exp(-D_ij / bw_m), s_ij = +1 inside a
 *             domain, -1 across
 *   mmd_grad  grad[i][p] = 4 sum_j c_ij (x_i[p] - x_j[p])  = d (scale * mean_k loss_rows[k]) / d x_i[p], the bandwidth taken as
 *             a constant (`.data` in the reference); grad_source [B][K][HW] and grad_target [B][K][HW] are each nullable: a null
 *             pointer means that side is detached and nothing is written for it
 * The scalar loss is mi355_reduce_sum(loss_rows, scale / K).  A joint whose distances are ALL zero has bw = 0 and the reference
 * returns NaN (0 / 0); here it contributes loss_rows[k] = 0 and zero gradient rows (as `guard_empty_maps` does for empty maps).
 * work: mi355_mmd_workspace(B, K) bytes (K n^2 floats; 0 when the shape is refused).  Pointers need 4-byte alignment; 16-byte
 * accesses are used when HW % 4 == 0 and the bases allow.  1 <= kernel_num <= MI355_MMD_MAX_KERNELS, kernel_mul > 0, K <= 65535,
 * HW <= 2^30.  Deterministic: no atomics, fixed summation orders.  Never allocates; capturable. */
#define MI355_MMD_MAX_ROWS 256
#define MI355_MMD_MAX_KERNELS 8
size_t mi355_mmd_workspace(int B, int K);
int mi355_mmd_heatmap(const float* source, const float* target, float* work, size_t work_bytes, float* loss_rows,
                      float* grad_source, float* grad_target, int B, int K, int HW, float kernel_mul, int kernel_num,
                      float fix_sigma, float scale, void* stream);

/* ---------------------------------------------------------------- joint feature alignment (csrc/jfa.hip)
 * loss1 / loss3 of uda/model/loss.py:331-378, the per-joint feature alignment term the reference imports (train1.py:25) and
 * never connects, without its Python loop over B x 21 windows and the two host reads of each.  Features are NHWC [B][H][W][C]
 * (dtype MI355_F32 / MI355_BF16), key points xy [B][K][2] = (x, y) fp32 in pixels of the map, on the device.
 * The window of joint (b, j), with (cr, cc) = (x, y) when rows_by_x (the reference's indexing, :353) and (y, x) otherwise:
 *   r0 = int(max(cr - radius, 0)), r1 = int(min(cr + radius, H - 1)), q0 = int(max(cc - radius, 0)), q1 = int(min(cc + radius, W - 1))
 * in fp32, truncated towards zero (.int(), :349-352), rows [r0, r1) x columns [q0, q1); the reference's constant 63 is H - 1 =
 * W - 1 of its 64 x 64 map.  r1 <= r0 or q1 <= q0 is an empty window (a coordinate outside the map: the reference falls into
 * negative-index slicing there); a NaN coordinate gives an empty window too.
 *   mi355_jfa_pool     desc[b][j][c] = (sum of feature[b][r][q][c] over the window) / divisor, fp32, one IEEE division (:353-357;
 *                      divisor = (2 radius + 1)^2 = 169 there); an empty window gives zeros
 *   mi355_jfa_kl       on a, b [nrows][C] fp32 (loss3, :368-378): lp = log_softmax(a), q = (b + 1e-6) / S, S = sum_c (b_c + 1e-6),
 *                      rows[i] = sum_c q_c (log q_c - lp_c); grad_a = coef (softmax(a) - q) and grad_b = coef ((log q - lp) -
 *                      rows[i]) / S, each nullable (nothing is written for a null one).  The scalar loss is
 *                      mi355_reduce_sum(rows, scale / nrows) and coef = scale / nrows.  b + 1e-6 must be positive.  The arithmetic
 *                      behind the fp32 operands and results is fp64 (the row is a small difference of large logarithms).
 *   mi355_jfa_scatter  the backward of mi355_jfa_pool as a gather: gd[b][j][c] = grad_desc[b][j][c] / divisor, and for every pixel
 *                      s = sum of gd[b][j][:] over the joints whose window holds it, j ascending, in fp32.  accumulate = 0:
 *                      grad_feature = s rounded to dtype (+0 where no window covers); accumulate = 1: a covered pixel becomes
 *                      round(grad_feature + s), one rounding, an uncovered one is not touched.
 * C a multiple of 8, 1 <= K <= MI355_JFA_MAX_JOINTS, H, W >= 1, radius >= 1, divisor > 0; feature, desc, a, b and the gradients
 * 16-byte aligned.  Deterministic: no atomics, fixed summation orders.  Never allocates; capturable. */
#define MI355_JFA_MAX_JOINTS 32
int mi355_jfa_pool(const void* feature, const float* xy, float* desc, int B, int K, int C, int H, int W, int radius, float divisor,
                   int rows_by_x, int dtype, void* stream);
int mi355_jfa_kl(const float* a, const float* b, float* rows, float* grad_a, float* grad_b, int nrows, int C, float coef, void* stream);
int mi355_jfa_scatter(const float* grad_desc, const float* xy, void* grad_feature, int accumulate, int B, int K, int C, int H, int W,
                      int radius, float divisor, int rows_by_x, int dtype, void* stream);

/* ---------------------------------------------------------------- prototype alignment with running memory (csrc/proto.hip)
 * lossx (uda/model/loss.py:381-466) and lossx3 (:560-652): per joint, the descriptors of a batch averaged into one class prototype,
 * blended with a memory kept from call to call, and the KL divergence between the channel distributions of the target and the
 * source prototypes -- without the Python loop over B x 21 windows and the host reads of each.  Layouts, key points, windows,
 * `rows_by_x` and the empty-window rule as in the joint feature alignment section above; the reference's constants 6 and 63 are
 * `radius` and the side - 1 (:410-417, :588-595).  blend = {m, 1 - m}, two fp32 in device memory (m = 0.999 at :400 / :578).
 *   mi355_proto_pool     desc[b][j][c] = (sum of feature[b][r][q][c] over the window) / (s_row s_col), s = hi - lo + 1 on either axis,
 *                        one more than the pixels summed (:418-425, :596-603); fp32 sum, one IEEE division; an empty window gives zeros
 *   mi355_proto_update   pbar[j][c] = (sum_b desc[b][j][c]) / B, b ascending in fp32 (:433-437, :611-615); proto = m pbar + (1 - m)
 *                        memory (:448, :626); memory <- proto in place (self.val1 = fea_c1.detach(), :454 / :460, :632 / :639)
 *   mi355_proto_kl       on proto_t, proto_s [K][C] fp32: lp = log_softmax(proto_t); MI355_PROTO_KL (:455-466): q = proto_s / S, S =
 *                        sum_c proto_s; MI355_PROTO_SOFTKL (:645): q = softmax(proto_s).  rows[j] = sum_c q_c (log q_c - lp_c), an
 *                        element with q_c = 0 adding 0.  grad_t = coef (softmax(proto_t) - q); grad_s = coef ((log q - lp) - rows[j])
 *                        / S (kl; 0 where q_c = 0) or coef q ((log q - lp) - rows[j]) (softkl); each nullable (nothing is written for a
 *                        null one).  The scalar loss is mi355_reduce_sum(rows, scale / K) with coef = scale / K for kl (.mean(), :466),
 *                        mi355_reduce_sum(rows, scale) with coef = scale for softkl (reduction='sum').  kl with S <= 0: rows[j] = 0 and
 *                        zero gradients (the reference gives NaN).  fp64 arithmetic behind the fp32 operands and results.
 *   mi355_proto_scatter  the backward of pool + update as a gather: gd[b][j][c] = (grad_proto[j][c] * (m / B)) / (s_row s_col)(b, j),
 *                        and for every pixel s = sum of gd[b][j][:] over the joints whose window holds it, j ascending, in fp32.
 *                        accumulate = 0: grad_feature = s rounded to dtype (+0 where no window covers); accumulate = 1: a covered
 *                        pixel becomes round(grad_feature + s), one rounding, an uncovered one is not touched.
 * C a multiple of 8, 1 <= K <= MI355_JFA_MAX_JOINTS, H, W >= 1, radius >= 1; feature, desc, memory, the prototypes and the gradients
 * 16-byte aligned; proto != memory.  Deterministic: no atomics, fixed summation orders.  Never allocates; capturable. */
#define MI355_PROTO_KL 0
#define MI355_PROTO_SOFTKL 1
int mi355_proto_pool(const void* feature, const float* xy, float* desc, int B, int K, int C, int H, int W, int radius, int rows_by_x,
                     int dtype, void* stream);
int mi355_proto_update(const float* desc, float* memory, const float* blend, float* proto, int B, int K, int C, void* stream);
int mi355_proto_kl(const float* proto_t, const float* proto_s, float* rows, float* grad_t, float* grad_s, int K, int C, int mode,
                   float coef, void* stream);
int mi355_proto_scatter(const float* grad_proto, const float* xy, const float* blend, void* grad_feature, int accumulate, int B, int K,
                        int C, int H, int W, int radius, int rows_by_x, int dtype, void* stream);

/* ---------------------------------------------------------------- cross-domain mixup (csrc/mixup.hip)
 * mixup of uda/model/loss.py:13-24, the first function of that file, which the reference never calls: every source sample
 * blended with the target sample of the same index by a per-sample coefficient, images, heat-maps and joint weights in ONE
 * launch.  Dense fp32 operands: x_s, x_t [B][img_plane] (img_plane = C * S * S of an NCHW image), hm_s, hm_t [B][hm_plane]
 * (hm_plane = K * H * W), w_s, w_t [B][K], lam [B] in DEVICE memory, already max(mix, 1 - mix) (:17).  With om = fl(1.0f - lam[b]):
 *   x_mix[b]      = fl(fl(x_s[b] * lam[b]) + fl(x_t[b] * om))       the source-dominant blend (:19-20), rows [0, B)
 *   x_mix[B + b]  = fl(fl(x_t[b] * lam[b]) + fl(x_s[b] * om))       the target-dominant blend (:21-22), rows [B, 2B)
 * and hm_mix [2B][hm_plane] likewise; w_mix [2B][K] = max(w_s, w_t) in both halves (:23-24).  Three fp32 roundings per element
 * as in torch's expression, nothing contracted into an FMA.  Every input element is read once and feeds both blends.  A stream:
 * at most MI355_MIXUP_MAX_BLOCKS blocks of 256 lanes with a grid-stride loop, 16-byte accesses when x_s, x_t, x_mix (hm_s, hm_t,
 * hm_mix) are all 16-byte aligned -- the coefficient is looked up per element, a vector may straddle samples -- and scalar
 * accesses otherwise; pointers need 4-byte alignment only.  Refused with MI355_EINVAL before any launch: a null pointer, B < 1, a
 * plane or K below 1, B * plane above 2^40, an output range that overlaps an input range or another output.  Finite operands;
 * what a NaN weight gives is not part of the contract.  Never allocates; capturable. */
#define MI355_MIXUP_MAX_BLOCKS 2048
int mi355_mixup_pairs(const float* x_s, const float* x_t, const float* hm_s, const float* hm_t, const float* w_s, const float* w_t,
                      const float* lam, float* x_mix, float* hm_mix, float* w_mix, int B, long img_plane, long hm_plane, int K,
                      void* stream);

/* ---------------------------------------------------------------- Fourier-domain stylisation (csrc/fda.hip)
 * Fourier Domain Adaptation (Yang and Soatto, "FDA: Fourier Domain Adaptation for Semantic Segmentation", CVPR 2020).  The
 * reference has no such function, so there is no file:line to cite; the semantics are those of the paper's published
 * low_freq_mutate (fft2 -> fftshift -> swap the centre window of the amplitude -> ifftshift -> ifft2 -> real), stated here.
 * x_s, x_t, out [B][C][H][W] dense fp32 (NCHW), normalised as the loaders deliver them ((p - mean_c) / std_c); source image i
 * is paired with target image i.  b = floor(min(H, W) * beta) is computed by the caller; the window is u, v in [-b, b].
 * Spectra are those of the DE-NORMALISED planes p = x * std_c + mean_c (non-negative pixels, so the DC term has phase 0); the
 * affine is folded into the coefficients, not applied per pixel: F01[u,v] = std_c * Fnorm[u,v], plus mean_c * H * W at [0,0].
 *   D[u,v]    = (|Ft[u,v]| - |Fs[u,v]|) * Fs[u,v] / |Fs[u,v]|        (phase factor 1 where |Fs[u,v]| == 0, as np.angle(0) = 0)
 *   out[y,x]  = fl32(x_s[y,x] + 1 / (H W std_c) * Re sum_{u,v} D[u,v] e^{+2 pi i (u y / H + v x / W)})
 * No clamp to the pixel range (the published code has none).  x_s and x_t are only read.  Twiddles (arguments reduced in
 * integers, from a table built per block), sums, magnitudes and the inverse sum are fp64 on the fp32 operands; the only
 * rounding to fp32 is the store.  D is Hermitian: only v >= 0 is computed and doubled, and the v = 0 column is summed from
 * u >= 0 alone, so the result is real by construction.  Two launches whatever B is: (1) per stripe of 32 rows of a plane, the
 * partial (2b+1) x (b+1) window of both spectra into ws; (2) per block the stripe partials folded in stripe order, D, and the
 * output rows.  No atomics, fixed summation orders: the same bits on every run, eagerly and under graph replay.  Rows are read
 * and written as 16-byte vectors when the bases are 16-byte aligned and W % 4 == 0, float by float otherwise.
 * mean, std: HOST arrays of C floats, passed to the kernels by value.  ws: mi355_fda_workspace_bytes(B, C, H, W, b) bytes of
 * device memory, 16-byte aligned, written by launch 1 and read by launch 2.  Refused with MI355_EINVAL before any launch,
 * the message naming the argument (mi355_fda_workspace_bytes returns -1): b < 0, b > MI355_FDA_MAX_B, 2b+1 > min(H, W), C
 * outside 1..4, B < 1 (or B * C * ceil(H / 32) above 2^31 - 1), H or W outside 1..1024, std_c <= 0 or not finite, mean_c not
 * finite, a null pointer, x_s / x_t / out not 4-byte aligned, ws not 16-byte aligned or smaller than needed, out or ws
 * overlapping an input or each other.  A non-finite pixel makes every pixel of that output plane non-finite and leaves the
 * other planes as they are.  Never allocates; capturable. */
#define MI355_FDA_MAX_B 32
long mi355_fda_workspace_bytes(int B, int C, int H, int W, int b);
int mi355_fda_transfer(const float* x_s, const float* x_t, float* out, const float* mean, const float* std, int B, int C, int H,
                       int W, int b, void* ws, long ws_bytes, void* stream);

/* ---------------------------------------------------------------- geometric teacher view (csrc/warp.hip)
 * The teacher of a consistency term sees another view of the target image -- rotated, scaled, shifted per sample -- and its
 * heat-maps are mapped back before they are compared (Kim et al., "A Unified Framework for Domain Adaptive Pose Estimation",
 * ECCV 2022).  The reference has no such function, so there is no file:line to cite; the semantics are stated here.  Forward
 * only: the teacher is detached, nothing is differentiated through either warp.
 * The view of sample b maps a point p of the loader's frame to q = A p = s R(a) (p - c) + c + t, c = ((W-1)/2, (H-1)/2).  Its
 * record holds three row-major 2 x 3 fp32 matrices acting on (column, row, 1), composed on the host in float64 and rounded once:
 * img = A^-1 (output pixel of the warped image -> input pixel), hm = A in heat-map pixels (image coordinate = stride * heat-map
 * coordinate: the same linear part, the translation divided by the stride), hm_inv = the inverse of hm.
 * Arithmetic of both warps, fp32, no FMA contraction, for output pixel (row i, column j) under the matrix m:
 *   xs = fl(fl(fl(m00 * j) + fl(m01 * i)) + m02), ys likewise with the second row;
 *   the sample is +0 unless xs > -1 && xs < W && ys > -1 && ys < H, tested before any conversion to an integer (NaN and inf
 *   coordinates give +0);  x0 = floor(xs), fx = fl(xs - x0);  a tap outside the plane has the value +0;
 *   horizontally r = (fx == 0) ? v0 : fl(fl(v0 * fl(1 - fx)) + fl(v1 * fx)), vertically the same form on the two row results;
 *   a tap whose weight is exactly 0 is not read.
 * So the identity record, integer shifts and exact quarter turns are exact copies, -0, inf and NaN included.  No atomics, the
 * same bits on every run, eagerly and under graph replay.  Dense fp32 operands, pointers 4-byte aligned; an output must not
 * overlap an input or another output; sides up to MI355_WARP_MAX_SIDE.  Never allocates; capturable.
 * affine_warp_images: out[b][c] = x[b][c] sampled under recs[b].img, x and out [B][C][H][W].  Every output pixel is written once;
 *   a stream whose gathers are served by the caches.  16-byte stores when out is 16-byte aligned and W % 4 == 0, scalar otherwise.
 * affine_unwarp_heatmaps: out[b][k] = y[b][k] sampled under recs[b].hm, y and out [B][K][h][w], one workgroup per map, the map
 *   staged in LDS when h * w * 4 <= 65536 (read from global memory otherwise: the same bits).  In the same launch
 *   valid[b][k] = 1.0f or 0.0f: with u* the arg-max of y[b][k] by mi355_argmax2d's rules (first index on ties, a NaN counts as the
 *   maximum), 1 iff margin <= u*_x <= (w-1) - margin and margin <= u*_y <= (h-1) - margin (fp32) and p* = hm_inv u* (the order
 *   above) lies in [0, w-1] x [0, h-1].  The location decides, not the peak's value.  w_out[b][k] = fl(w_in[b][k] * valid[b][k]);
 *   w_in and w_out are both given or both null.  margin: finite and >= 0.
 * mse_heatmap_w: mi355_mse_heatmap with a per-map fp32 weight wmap[B * K] in device memory: with s the row sum of
 *   mi355_mse_heatmap in its order, rows[r] = fl(s * w) and unit_grad[r][j] = fl(fl(fl(p_j - t_j) * grad_scale) * w).  A row with
 *   w == 0 or outside the joint mask is exact zeros and pred / target are not read for it.  grad_scale is the caller's: n stays
 *   B * |subset| * H * W whatever the weights are. */
#define MI355_WARP_MAX_SIDE 4096
typedef struct mi355_view_rec { float img[6]; float hm[6]; float hm_inv[6]; } mi355_view_rec;
int mi355_affine_warp_images(const float* x, const mi355_view_rec* recs, float* out, int B, int C, int H, int W, void* stream);
int mi355_affine_unwarp_heatmaps(const float* y, const mi355_view_rec* recs, float margin, const float* w_in, float* out, float* valid,
                                 float* w_out, int B, int K, int h, int w, void* stream);
int mi355_mse_heatmap_w(const float* pred, const float* target, const mi355_mse_rec* rec_dev, const float* wmap, float* rows,
                        float* unit_grad, int B, int K, int HW, void* stream);

/* ---------------------------------------------------------------- adaptive occlusion, teacher confidence (csrc/occlude.hip)
 * The student of a consistency term sees the target image with a patch around a key point the teacher is sure of blanked out,
 * and the teacher-driven terms weigh a map by whether the teacher is sure of it (Kim et al., "A Unified Framework for Domain
 * Adaptive Pose Estimation", ECCV 2022; the patch rule is this project's, the paper's is not quoted: PAPERS.md).  The reference has
 * no such function, so there is no file:line to cite; the semantics are stated here.  Forward only.  No atomics; the same bits on
 * every run, eagerly and under graph replay.  Dense operands, pointers 4-byte aligned.  Never allocates; capturable.  Every
 * refusal is MI355_EINVAL before any launch, the message naming the argument.
 * peak_prob: per map of hm [rows][H][W] fp32, idx[rows] and xy[rows][2] are mi355_argmax2d's bit for bit (first index on ties, a
 *   NaN counts as the maximum, xy = 0 unless the maximum is > 0) and p[rows] = 1 / s rounded once to fp32, s = the fp64 sum over the
 *   map of exp((double)v * beta - (double)max * beta) in a fixed order: the peak of softmax(beta * y), this project's stand-in for the paper's
 *   normalised activation (the main head is trained with a KL against normalised Gaussians, so the raw maximum is an unbounded
 *   logit; a perfect sigma = 2 label has p = 1 / (8 pi)).  A map that holds a NaN or +-inf has p = NaN.  Forms as mi355_softargmax:
 *   register-resident at 64 x 64, 32 x 32, 16 x 16 for a 16-byte-aligned hm (the map is read once), the loop form otherwise
 *   (walked twice).  beta: finite and > 0; H * W below 2^31.
 * teacher_select: one thread per sample.  pass[b][k] = p >= tau && (gate_in null || gate_in > 0); conf[b][k] = 1.0f or 0.0f (a NaN p
 *   never passes); with w_in (and w_out; both or neither) w_out = fl(w_in * conf).  N > 0: the candidates of sample b are its joints
 *   with pass and (w_in null || w_in > 0) in ascending order, m of them.  u[b][1 + 2N] are uniform draws in [0, 1).  u[b][0] >= prob:
 *   no box.  Otherwise for slot i < min(N, m), with mm = m - i candidates left: j = min(int(fl(u[b][1+2i] * mm)), mm - 1) (fp32
 *   product, truncated) is taken out of the list; side = min(lo + int(fl(u[b][2+2i] * (hi - lo + 1))), hi); with (x, y) = xy[b][k]
 *   clamped to the map (NaN -> 0), cx = int(x) * (S / W) + (S / W) / 2, cy = int(y) * (S / H) + (S / H) / 2; the box is
 *   x0 = cx - side / 2, x1 = x0 + side, likewise in y, clipped to [0, S]: boxes[b][i] = (x0, y0, x1, y1), half-open.  Unused slots
 *   are (0, 0, 0, 0); count[b] = boxes drawn.  N == 0: gate only (xy, u, boxes, count may be null).  stats (nullable): two floats,
 *   the mean of count over B and the mean of conf over B * K, from integer sums.  tau finite; prob in [0, 1]; N in 0 ..
 *   MI355_OCC_MAX_BOXES; 1 <= lo <= hi <= S; S a multiple of H and of W; K up to MI355_OCC_MAX_JOINTS.
 * occlude_images: out = x [B][C][H][W] with every pixel inside any of the N boxes of its sample (all channels) set to +0.0 -- 0
 *   is the data-set mean in normalised space -- and every other word copied bit for bit (NaN payloads, -0.0).  x is only read,
 *   every word of out is written exactly once, out is never read.  boxes [B][N][4] int32 (x0, y0, x1, y1), half-open, any values
 *   (they are only compared with); a sample's records are read once per workgroup.  A stream: 16-byte accesses when W % 4 == 0
 *   and x and out are 16-byte aligned, 4-byte otherwise.  out must not overlap x or boxes; C * H * W below 2^31. */
#define MI355_OCC_MAX_BOXES 8
#define MI355_OCC_MAX_JOINTS 64
#define MI355_OCC_MAX_BATCH 65535
#define MI355_OCC_MAX_SIDE 4096
int mi355_peak_prob(const float* hm, float beta, int32_t* idx, float* xy, float* p, int rows, int H, int W, void* stream);
int mi355_teacher_select(const float* p, const float* xy, const float* gate_in, const float* w_in, const float* u, float tau,
                         float prob, int N, int lo, int hi, int S, int H, int W, float* conf, float* w_out, int32_t* boxes,
                         int32_t* count, float* stats, int B, int K, void* stream);
int mi355_occlude_images(const float* x, const int32_t* boxes, int N, float* out, int B, int C, int H, int W, void* stream);

/* ---------------------------------------------------------------- rendered hands (csrc/render.hip)
 * A batch of S x S RGB images drawn from one fixed-size record per sample: 20 bone capsules between 21 projected joints, one
 * optional occluder capsule, a two-colour gradient background with value noise, Lambert shading, sensor noise and a photometric
 * gain / bias (utils/rendered_dataset.py fills the records; the reference has no such function).  The arithmetic, restated in numpy
 * by tests/render_ref.py: fp32, only + - * / sqrt, every operation rounded on its own, no FMA contraction, sums left to right.
 *   Primitive k = 0 .. 19 is bone k of the hand (parent a = joint (k % 4 == 0 ? 0 : k), child b = joint k + 1; x, y in pixels, z a
 *   depth in pixels, smaller is nearer) with radius[k]; primitive 20 is the occluder (occ_a, occ_b, occ_r, depth occ_z at both
 *   ends).  A primitive is VALID iff ax, ay, az, bx, by, bz and r all have a magnitude <= MI355_RENDER_MAX_COORD (which a NaN and
 *   an infinity fail) and r > 0; one that is not covers nothing.
 *   At a point p = (px, py): e = b - a; ee = ex*ex + ey*ey; d = p - a; q = (dx*ex + dy*ey) / ee when ee > 0, else 0 -- chosen by
 *   selection, the quotient is not formed; t = q < 0 ? 0 : (q > 1 ? 1 : q); c = a + t*e; w = p - c; d2 = wx*wx + wy*wy; r2 = r*r;
 *   p is covered iff d2 <= r2; depth = (az + t*(bz - az)) - sqrt(r2 - d2).  The front-most primitive is the covered one of
 *   strictly smallest depth below +inf, the lower index on ties.
 *   Colour there: n = (wx / r, wy / r, sqrt(1 - d2 / r2)); lam = n.x*l.x + n.y*l.y + n.z*l.z, 0 unless > 0;
 *   shade = ambient + (1 - ambient) * lam; colour[c] = base[c] * shade, base = skin, or occ_col for the occluder.
 *   Background: g = (px*grad[0] + py*grad[1]) + grad_off clamped to [0, 1] as t is; colour[c] = bg0[c] + g*(bg1[c] - bg0[c]); when
 *   noise_amp > 0 and 0 < noise_inv_cell <= 1 (else no noise): u = (px + 1)*inv_cell, v = (py + 1)*inv_cell, ix = floor(u),
 *   fx = u - ix, sx = (fx*fx)*(3 - 2*fx), likewise y; with L(i, j) = H(noise_seed, i, j) the lattice values,
 *   top = L(ix,iy) + sx*(L(ix+1,iy) - L(ix,iy)), bot likewise on iy + 1, val = top + sy*(bot - top), and amp*(val - 0.5) is added
 *   to each channel.  H(s, a, b) = float(h >> 8) * 2^-24 in [0, 1) with, on uint32, h = s ^ a*0x9E3779B1; h ^= h >> 16;
 *   h *= 0x85EBCA6B; h ^= b*0xC2B2AE35; h ^= h >> 13; h *= 0x27D4EB2F; h ^= h >> 16.
 *   Pixel (row i, column j), channel c: m[c] = 0.25 * (((s0 + s1) + s2) + s3) over the colours at (j - .25, i - .25),
 *   (j + .25, i - .25), (j - .25, i + .25), (j + .25, i + .25);  out_ema = (m[c] - mean[c]) * inv_std[c];
 *   out = ((m[c]*gain[c] + bias[c] + noise) - mean[c]) * inv_std[c], noise = sensor_sigma * ((((u0 + u1) + u2) + u3) - 2) with
 *   uk = H(sensor_seed ^ (4c + k + 1)*0x632BE5AB, i, j) when sensor_sigma > 0, else absent;  ids = 1 + the front-most
 *   primitive at the pixel centre (j, i), 0 for background.
 * out, out_ema (nullable) [B][3][S][S] fp32, ids (nullable) [B][S][S] uint8; mean3, inv_std3: HOST pointers to three floats.  S: a
 * multiple of 16 from 16 to 512.  recs, out, out_ema 16-byte aligned, ids 4-byte.  No output may overlap recs or another output.
 * One launch: one workgroup per 32 x 32 tile of one sample, the record staged in LDS, the primitives culled against the tile by
 * float comparisons only (nothing in a record is ever converted to an index except the noise lattice coordinate, whose range
 * the inv_cell test bounds); the culling never changes the image.  No atomics: the same bits on every run, eagerly and under
 * graph replay.  Never allocates; capturable.  Every refusal is MI355_EINVAL before any launch, naming the argument. */
#define MI355_RENDER_MAX_COORD 1048576.0f
#define MI355_RENDER_MAX_SIDE 512
typedef struct mi355_hand_rec {
  float jx[21], jy[21], jz[21];      /* projected joints: pixels, depth in pixels */
  float radius[20];                  /* per bone, pixels */
  float skin[3], light[3], ambient;  /* base colour, unit light direction (z towards the camera), ambient share */
  float bg0[3], bg1[3], grad[2], grad_off;
  float noise_amp, noise_inv_cell; uint32_t noise_seed;
  float occ_a[2], occ_b[2], occ_r, occ_z, occ_col[3];     /* occ_r = 0: no occluder */
  float sensor_sigma; uint32_t sensor_seed;
  float gain[3], bias[3];
  uint32_t reserved;                 /* pads the record to 480 bytes, a multiple of 16 */
} mi355_hand_rec;
size_t mi355_hand_rec_size(void);
int mi355_render_hands(const mi355_hand_rec* recs, float* out, float* out_ema, unsigned char* ids, int B, int S,
                       const float* mean3, const float* inv_std3, void* stream);

/* ---------------------------------------------------------------- hand tracking (csrc/track.hip)
 * From a camera frame and a rough hand box to key points in that frame, and from those to the next frame's box, without the host:
 * the boxes are records in DEVICE memory that one kernel crops by and the other rewrites.  Tracking a hand by the box of its
 * previous key points is the common practice of hand-pose pipelines; the box rule below is this project's.  The
 * reference has no such function, so there is no file:line to cite; the semantics are stated here and restated in numpy by
 * tests/track_ref.py.  Forward only.  No atomics: the same bits on every run, eagerly and under graph replay.  Never allocates;
 * capturable.  fp32 throughout, every operation rounded on its own, no FMA contraction.
 * The record: (x0, y0) is the left / upper EDGE of a square of `side` frame pixels -- PIL's crop box, the convention of
 * uda/dataset/keypoint_detection.crop -- in frame `frame` of the batch; mirror != 0 flips the crop along W (a left hand shown to
 * a right-hand network); live == 0 is an empty slot; lost counts the frames since the hand was last seen.  The host never reads
 * a record before a launch, so both kernels are safe for ANY bit pattern in it.  A record is USABLE iff live != 0 and
 * 0 <= frame < F and |x0| <= MI355_TRACK_MAX_COORD and |y0| <= MI355_TRACK_MAX_COORD (a NaN and an infinity fail) and
 * 1 <= side <= 4 S (mi355_track_update has no F: there `frame` is not tested).  Every test on a float is a float comparison made
 * before any conversion to an integer; no address is formed from an unbounded value.
 * roi_crop_normalize: out[n] [3][S][S] fp32 = the square of record n resized to S x S and normalised; frames [F][Hf][Wf][3] uint8 RGB,
 *   dense, 1 <= Hf, Wf <= MI355_TRACK_MAX_FRAME (the row pitch 3 Wf need not be a multiple of 4); norm: HOST pointer to six floats,
 *   mean[3] then std[3] (std > 0, all finite).  An unusable record writes +0.0 to its whole image and reads no pixel.  Otherwise
 *     value of a byte p in channel c: T[c][p] = fl(fl((float)p / 255.0f - mean[c]) / std[c]), what mi355_resize_normalize writes for
 *       it; a tap outside the frame has the value +0 (the data-set mean), chosen by selection, nothing is read;
 *     step = fl(side / (float)S); n = 1 if side <= S, 2 if side <= 2 S, 3 if side <= 3 S, else 4 sub-samples per axis;
 *     off_a = fl(((float)a + 0.5f) / (float)n), a = 0 .. n-1; for output column j: jj = mirror ? S - 1 - j : j and
 *       xs = fl(fl(x0 + fl(fl((float)jj + off_a) * step)) - 0.5f); ys likewise from y0 and the row i (never mirrored);
 *     one sample at (xs, ys), per channel, by the rule stated above for mi355_affine_warp_images on the Hf x Wf plane of T-values:
 *       +0 unless xs > -1 && xs < Wf && ys > -1 && ys < Hf; x0i = floor(xs), fx = fl(xs - x0i); horizontally
 *       r = (fx == 0) ? v0 : fl(fl(v0 * fl(1 - fx)) + fl(v1 * fx)), vertically the same form on the two row results with fy; with
 *       fx == 0 (fy == 0) the second tap (row) is not read -- the only skipped read: when fx rounds to 1 the first tap is read
 *       with weight 0, inside the frame like every read;
 *     the pixel = fl(sum / (float)(n n)), sum = the n n samples added left to right starting from the first, sub-sample rows
 *       ascending and columns ascending within a row.
 *   So an integer box with side == S is mi355_resize_normalize of that square bit for bit, and mirror is that image flipped.
 *   One workgroup per 32 x 32 output tile of one hand; the record is read once per workgroup and T is built in LDS.  16-byte stores
 *   when out is 16-byte aligned, 4-byte stores otherwise; out and recs need 4-byte alignment, frames none.  S: a multiple of 16 from
 *   16 to MI355_TRACK_MAX_SIDE.  out must not overlap frames or recs.
 * track_update: one thread per hand, joints in ascending order.  xy [N][K][2] key points in crop pixels (as the decoders write
 *   them), conf [N][K]; kp [N][K][2], vis [N][K], score [N] are written; rec_out may be rec_in itself (a thread reads its record
 *   completely before it writes) and may not overlap it otherwise.  With Sf = (float)S, Wff = (float)Wf, Hff = (float)Hf of params:
 *   unusable record: kp, vis, score = +0 and rec_out = rec_in with live = 0.  Otherwise
 *     st = fl(side / Sf); xm = mirror ? fl(fl(Sf - 1.0f) - x) : x; kx = fl(x0 + fl(xm * st)), ky = fl(y0 + fl(y * st));
 *     vis[k] = 1.0f iff conf[k] >= tau (a NaN fails) and kx and ky are finite, else 0.0f; kp[k] = (kx, ky), or (+0, +0) when either
 *     is not finite.  m = the visible joints; score = fl(sum / (float)m), sum = their conf added left to right from +0; 0 when m = 0.
 *     cap = min(min(Wff, Hff), 4 Sf); clamp(s) = (t = s < min_side ? min_side : s; t > cap ? cap : t); hx = fl(side * 0.5f);
 *     cx = fl(x0 + hx), cy = fl(y0 + hx) the old centre.
 *     m >= min_joints: over the visible kp, (lx, ux) = (min, max) of kx, (ly, uy) of ky; e = max(fl(ux - lx), fl(uy - ly));
 *       sn = clamp(fl(scale * e)); nx = fl(fl(lx + ux) * 0.5f), ny likewise; cx' = fl(cx + fl(alpha * fl(nx - cx))), cy' likewise,
 *       side' = clamp(fl(side + fl(alpha * fl(sn - side)))); lost' = 0.
 *     else: lost' = lost < 0 ? 1 : (lost >= max_lost ? max_lost + 1 : lost + 1).  lost' > max_lost: live' = 0 and x0, y0, side are
 *       kept as they are.  Otherwise cx' = cx, cy' = cy, side' = (t = fl(side * grow); t > cap ? cap : t).
 *     In every case but the dead one: x0' = shift(fl(cx' - fl(side' * 0.5f)), Wff), y0' = shift(fl(cy' - fl(side' * 0.5f)), Hff),
 *       shift(v, L) = (t = v < 0 ? 0 : v; h = fl(L - side'); t > h ? h : t), the rule of uda/dataset/util.scale_box without its
 *       rounding to whole pixels.  frame and mirror are copied, reserved is written as 0, live' = 1 unless dead.
 *   params, checked on the host: tau finite; 1 <= min_joints <= K; scale finite and > 0; 0 <= alpha <= 1; grow finite and >= 1;
 *   0 <= max_lost <= 2^30; min_side finite and >= 1; 1 <= Wf, Hf <= MI355_TRACK_MAX_FRAME; S as above.  1 <= K <= MI355_TRACK_MAX_JOINTS.
 *   Pointers 4-byte aligned; no output may overlap an input (rec_out == rec_in apart) or another output.
 * Every refusal is MI355_EINVAL before any launch, the message naming the argument. */
#define MI355_TRACK_MAX_COORD 1048576.0f
#define MI355_TRACK_MAX_FRAME 4096
#define MI355_TRACK_MAX_SIDE 512
#define MI355_TRACK_MAX_JOINTS 64
typedef struct mi355_track_rec { int32_t frame; float x0, y0, side; int32_t mirror, live, lost, reserved; } mi355_track_rec;
typedef struct mi355_track_params {
  float tau; int32_t min_joints; float scale, alpha, grow; int32_t max_lost; float min_side; int32_t Wf, Hf, S;
} mi355_track_params;
int mi355_roi_crop_normalize(const unsigned char* frames, int F, int Hf, int Wf, const mi355_track_rec* recs, int N, int S,
                             const float* norm, float* out, void* stream);
int mi355_track_update(const mi355_track_rec* rec_in, const float* xy, const float* conf, mi355_track_params params, float* kp,
                       float* vis, float* score, mi355_track_rec* rec_out, int N, int K, void* stream);

/* ---------------------------------------------------------------- training augmentation (csrc/augment.hip)
 * The reference's per-sample CPU chain (train1.py:54-66: RandomRotation, RandomResizedCrop, ColorJitter(0.25, 0.25, 0.25),
 * GaussianBlur, ToTensor, Normalize, plus the image_ema copy of uda/dataset/keypoint_detection.py:171-181) on a batch of B
 * ragged HWC uint8 RGB sources packed into one buffer, bit-exact with Pillow's arithmetic:
 *   rotate    Image.rotate NEAREST as Pillow's 16.16 fixed-point affine (or its copy / transpose shortcuts);
 *   crop      square (top, left, side) of the rotated image, resized to S x S by Image.resize BILINEAR
 *             (22-bit coefficients from double math, horizontal pass to uint8, then the vertical pass);
 *   jitter    ImageEnhance brightness / contrast / saturation as float32 Image.blend, in the drawn order; contrast
 *             blends with int(mean(L) + 0.5) of the image it is applied to (exact integer sum over the image);
 *   blur      ImagingGaussianBlur with integer box radius 0: 3 horizontal then 3 vertical 3-tap passes,
 *             (ww * centre + fw * (left + right) + 2^23) >> 24 with edge clamp;
 *   output    out[b][c][y][x] = (v / 255 - mean[c]) / std[c] fp32 NCHW; ema (nullable): the same normalisation of the
 *             geometry image (before jitter and blur).
 * Unlike the rest of this header, the records are passed twice: `rec_host` (host memory) is what the argument checks read
 * before anything is enqueued, `rec_dev` (device memory, an identical copy) is what the kernels read.  Two launches.
 * S: a multiple of 16 from 16 to 512; sources up to 4096 x 4096; crop side <= 4 S; box radius 0.  Above S = 384 the
 * kernels need more than the default 64 KB of dynamic LDS (85 504 B and 67 584 B at 512): the cap is raised on first use,
 * MI355_ELAUNCH when the runtime refuses. */
typedef struct {
  int64_t offset;           /* byte offset of the source image (h x w x 3, row-major) in the packed buffer */
  int32_t h, w;             /* source size */
  int32_t rot;              /* 0 affine a[], 1 copy, 2 rotate 180, 3 rotate 90 (square), 4 rotate 270 (square) */
  int32_t a[6];             /* 16.16 fixed point: xs = (a2 + y*a1 + x*a0) >> 16, ys = (a5 + y*a4 + x*a3) >> 16 */
  int32_t top, left, side;  /* square crop of the rotated image (inside it), resized to S x S */
  float factor[3];          /* blend factors: brightness, contrast, saturation */
  int32_t order[3];         /* op ids (0 brightness, 1 contrast, 2 saturation) in application order, -1 = no op */
  int32_t blur;             /* 0 none, 1 the 3 + 3 box passes with weights ww, fw */
  uint32_t ww, fw;
  int32_t reserved;
} mi355_aug_rec;
/* workspace bytes of mi355_augment for B images of S x S */
size_t mi355_augment_workspace(int B, int S);
/* norm: host pointer to 6 floats (mean[3], std[3]); out: fp32 [B][3][S][S]; ema (nullable): fp32 [B][3][S][S] */
int mi355_augment(const uint8_t* src, int64_t src_bytes, const mi355_aug_rec* rec_host, const mi355_aug_rec* rec_dev,
                  int B, int S, const float* norm, float* out, float* ema, void* ws, size_t ws_bytes, void* stream);
/* The validation chain (train1.py:67-71: Resize, ToTensor, Normalize) and, in general, the geometry stage of mi355_augment
 * alone: out[b][c][y][x] is bit for bit what mi355_augment writes to `ema` for the same records (rotate, crop, BILINEAR
 * resize to S x S, normalisation).  Reads offset, h, w, rot, a[], top, left, side of every record; the photometric fields are
 * checked like mi355_augment checks them and otherwise ignored.  A validation sample is the identity record: rot 1 (copy),
 * top = left = 0, side = w = h.  Same argument checks, limits and rec_host / rec_dev convention as mi355_augment.
 * ONE launch: no workspace, no memset, no uint8 intermediate in memory. */
int mi355_resize_normalize(const uint8_t* src, int64_t src_bytes, const mi355_aug_rec* rec_host, const mi355_aug_rec* rec_dev,
                           int B, int S, const float* norm, float* out, void* stream);

/* ---------------------------------------------------------------- in-library kernel timing (bench.py roofline)
 * on = 1: every launch of the MFMA conv family is bracketed by hipEvents on its stream; on = 2: the BatchNorm kernels and
 * the weight-gradient slab reductions as well (family 1 / 2; they never enter the totals below).  mi355_prof_read
 * synchronises the recorded events and returns the conv family's totals since the last reset. */
int mi355_prof_enable(int on);
/* The launches logged since the last reset, one by one in launch order: family (0 conv MFMA, 1 BatchNorm, 2 other), event-timed
 * duration in microseconds (contains the dispatch latency mi355_prof_event_overhead_us measures), algorithmic FLOPs and bytes,
 * and a label naming the layer ("fwd k3s1 256>256 @64x64 n64 +stats", "bn_bwd_res rows262144 C256 ...").  The launches of the
 * implicit-GEMM convolutions also name the kernel build that ran, in brackets at the end of the label: "[g128x128 dma kg2 epi1]"
 * (gather kernel, 128 x 128 tile, LDS-DMA ring, two K groups, statistics epilogue; "f32", "small", "hm", "kw3", a leading "cat"
 * and "epi2" name the fp32, small-channel, heat-map-output, shared-A-tile and concat-K builds and the BatchNorm-backward
 * epilogue), "[pgemm bm64 bn128 ns8 add]" (persistent GEMM: tile, ring depth, addend ring), "[f8 g64x128 bf8]" / "[mx g64x64]"
 * (fp8 / MX kernels; bf8: e5m2 operand).  Consumers match labels by prefix.  Each entry is ONE
 * kernel launch, so the list joins in order with a rocprofv3 kernel trace of the same iteration (profiles/insitu_table.py). */
int mi355_prof_launch_count(long* n);
int mi355_prof_read_launch(long i, int* family, double* us, double* flops, double* bytes, char* label, int label_cap);
/* idle spin of `us` microseconds on the stream (measurement aid: queue launches behind it so the GPU never waits for the host) */
int mi355_spin_us(long us, void* stream);
/* the timed launches split at an arithmetic intensity (FLOP / byte): out[0..3] = {ms, flops, bytes, launches} below it, out[4..7] above */
int mi355_prof_read_split(double flop_per_byte, double* out);
/* mean reading of an event pair around an empty kernel (the dispatch latency contained in every event-timed launch) */
int mi355_prof_event_overhead_us(int n, void* stream, double* us);
int mi355_prof_reset(void);
int mi355_prof_read(double* total_ms, long* launches, double* flops, double* algorithmic_bytes);

#ifdef __cplusplus
}
#endif
#endif
