"""Thin tensor-level wrappers over the C ABI (one per entry point of include/mi355pose.h).

Tensors are torch CUDA tensors used as device-memory handles.  Feature maps are *logical* NCHW
tensors in channels_last memory (= the NHWC layout the kernels use), dtype bf16 or fp32; heat-maps
are contiguous NCHW fp32.  Nothing here falls back to torch math.
"""
import ctypes
import math

import numpy as _np

import torch

from . import (BnBwdSrc, ConvDesc, FP8, Mi355Error, WgradItem, call, compute_dtype, dtype_code, load, ptr, stream_ptr, workspace)


# ---------------------------------------------------------------- layout helpers
def nhwc_empty(N, C, H, W, dtype, device):
    return torch.empty((N, H, W, C), dtype=dtype, device=device).permute(0, 3, 1, 2)


def is_nhwc(x):
    return x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous()


def _chk_room(what, t, need):
    """Raise before any launch when the caller-provided buffer `t` holds fewer than `need` elements: the kernels index it
    from the problem size alone and would read or write past its end."""
    if t is not None and t.numel() < need:
        raise Mi355Error('%s: buffer of %d elements, the launch indexes %d' % (what, t.numel(), need))


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise Mi355Error('mi355 ops need CUDA/HIP tensors (got a %s tensor); there is no CPU fallback' % t.device)


def _chk_feature(what, t, shape=None):
    """`t` must be a channels_last (NHWC memory) bf16 / fp32 feature tensor, of logical shape `shape` when given: the kernels
    index it from the problem size alone."""
    if t is None:
        return
    if not is_nhwc(t):
        raise Mi355Error('%s: needs a channels_last (NHWC memory) tensor, got shape %s strides %s' % (what, tuple(t.shape), t.stride()))
    if t.dtype not in (torch.bfloat16, torch.float32):
        raise Mi355Error('%s: needs a bf16 or fp32 tensor, got %s' % (what, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise Mi355Error('%s: shape %s, the launch indexes %s' % (what, tuple(t.shape), tuple(shape)))


def _chk_heatmap(what, t):
    if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous():
        raise Mi355Error('%s: needs a contiguous fp32 (N, K, H, W) heat-map, got %s %s strides %s' % (what, t.dtype, tuple(t.shape), t.stride()))


def to_nhwc(x, dtype=None, cpad=None):
    """NCHW fp32 (contiguous) -> channels_last `dtype`, channels zero-padded to `cpad`."""
    dtype = dtype or compute_dtype()
    N, C, H, W = x.shape
    per = 8 if dtype == torch.bfloat16 else 4
    cpad = cpad or ((C + per - 1) // per) * per
    if is_nhwc(x) and x.dtype == dtype and C == cpad:
        return x
    _chk_dev(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    y = nhwc_empty(N, cpad, H, W, dtype, x.device)
    call('mi355_nchw_to_nhwc', ptr(x), ptr(y), N, C, H, W, cpad, dtype_code(dtype), stream_ptr())
    return y


def to_nchw_f32(x):
    """channels_last bf16/fp32 -> contiguous NCHW fp32."""
    if not is_nhwc(x):
        raise Mi355Error('to_nchw_f32 expects a channels_last tensor')
    _chk_dev(x)
    N, C, H, W = x.shape
    y = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    call('mi355_nhwc_to_nchw', ptr(x), ptr(y), N, C, H, W, dtype_code(x.dtype), stream_ptr())
    return y


def to_nhwc_s2d(x, dtype=None):
    """3-channel NCHW fp32 image (even extents) -> the 2x2 space-to-depth image (N, 16, H/2, W/2), channels_last `dtype`: the
    input of the stem in its folded 4x4 form (mi355_nchw_to_s2d)."""
    dtype = dtype or compute_dtype()
    N, C, H, W = x.shape
    if C != 3 or H % 2 or W % 2:
        raise Mi355Error('to_nhwc_s2d: a 3-channel image with even extents, got %s' % (tuple(x.shape),))
    _chk_dev(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    y = nhwc_empty(N, 16, H // 2, W // 2, dtype, x.device)
    call('mi355_nchw_to_s2d', ptr(x), ptr(y), N, H, W, dtype_code(dtype), stream_ptr())
    return y


def stem_s2d_pack(w, dtype, out=None):
    """w: fp32 [Co][7][7][3] memory order -> flat `dtype` [Co][4][4][16], the folded stem's forward operand."""
    _chk_dev(w)
    Co = w.numel() // 147
    if out is None:
        out = torch.empty(Co * 256, dtype=dtype, device=w.device)
    _chk_room('stem_s2d_pack out', out, Co * 256)
    call('mi355_stem_s2d_pack', ptr(w), ptr(out), Co, dtype_code(dtype), stream_ptr())
    return out


def stem_s2d_unpack_grad(gs, g, accumulate):
    """gs: fp32 [Co][4][4][16] weight gradient of the folded stem; g: fp32 gradient in [Co][7][7][3] memory order (= / +=)."""
    _chk_dev(gs, g)
    if g.numel() % 147:
        raise Mi355Error('stem_s2d_unpack_grad: g is not a (Co, 3, 7, 7) gradient (%d elements)' % g.numel())
    _chk_room('stem_s2d_unpack_grad gs', gs, g.numel() // 147 * 256)
    call('mi355_stem_s2d_unpack_grad', ptr(gs), ptr(g), g.numel() // 147, int(bool(accumulate)), stream_ptr())


def make_desc(N, Hi, Wi, Ci, Co, kh, kw, stride, pad, dtype, out_hw=None):
    """out_hw: (Ho, Wo) of a cropped output (unit stride; forward and weight gradient only)."""
    Ho = (Hi + 2 * pad - kh) // stride + 1
    Wo = (Wi + 2 * pad - kw) // stride + 1
    if out_hw is not None:
        Ho, Wo = out_hw
    return ConvDesc(N, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, stride, pad, dtype_code(dtype))


# ---------------------------------------------------------------- convolution family
def conv_fwd(desc, x, w, bias=None, residual=None, relu=False):
    _chk_dev(x, w)
    y = nhwc_empty(desc.N, desc.Co, desc.Ho, desc.Wo, x.dtype, x.device)
    if relu:
        call('mi355_conv_fwd_act', ctypes.byref(desc), ptr(x), ptr(w), ptr(bias), ptr(residual), 1, ptr(y), stream_ptr())
    else:
        call('mi355_conv_fwd', ctypes.byref(desc), ptr(x), ptr(w), ptr(bias), ptr(residual), ptr(y), stream_ptr())
    return y


def deconv_fwd_act(desc, x, wT, bias=None, relu=False):
    """Inference ConvTranspose2d forward (conv-form dgrad) + bias + ReLU in one launch."""
    _chk_dev(x, wT)
    y = nhwc_empty(desc.N, desc.Ci, desc.Hi, desc.Wi, x.dtype, x.device)
    call('mi355_conv_dgrad_act', ctypes.byref(desc), ptr(x), ptr(wT), ptr(bias), int(bool(relu)), ptr(y), stream_ptr())
    return y


def _stats_buf(rows, C, device):
    nbytes = load().mi355_conv_stats_bytes(rows, C)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), nbytes


def conv_fwd_stats(desc, x, w, bias=None):
    """conv forward + BatchNorm statistics partials of y from the epilogue.  Returns (y, (partial, nslices) | None)."""
    _chk_dev(x, w)
    y = nhwc_empty(desc.N, desc.Co, desc.Ho, desc.Wo, x.dtype, x.device)
    partial, nbytes = _stats_buf(desc.N * desc.Ho * desc.Wo, desc.Co, x.device)
    ns = ctypes.c_int(0)
    call('mi355_conv_fwd_stats', ctypes.byref(desc), ptr(x), ptr(w), ptr(bias), ptr(y), ptr(partial), nbytes,
         ctypes.byref(ns), stream_ptr())
    return y, ((partial, ns.value) if ns.value > 0 else None)


def conv_fwd_cat(desc, x, w, bias, x2, w2, bias2, want_stats=False):
    """y = conv(x, w) + x2 * w2^T + bias + bias2 as one implicit GEMM (mi355_conv_fwd_cat).  x2: channels_last [N, c2, Ho, Wo] at
    the output resolution, w2: [Co, c2], both in x's dtype.  Returns y, or (y, (partial, nslices) | None) with want_stats."""
    _chk_dev(x, w, x2, w2)
    c2 = x2.shape[1]
    if x2.dtype != x.dtype or w2.dtype != x.dtype or not is_nhwc(x2) or tuple(x2.shape) != (desc.N, c2, desc.Ho, desc.Wo) or \
            tuple(w2.shape) != (desc.Co, c2) or not w2.is_contiguous():
        raise Mi355Error('conv_fwd_cat: second operand pair must be channels_last [N, c2, Ho, Wo] / contiguous [Co, c2] in the dtype of x')
    y = nhwc_empty(desc.N, desc.Co, desc.Ho, desc.Wo, x.dtype, x.device)
    if not want_stats:
        call('mi355_conv_fwd_cat', ctypes.byref(desc), ptr(x), ptr(w), ptr(bias), ptr(x2), ptr(w2), ptr(bias2), c2, ptr(y),
             None, 0, None, stream_ptr())
        return y
    partial, nbytes = _stats_buf(desc.N * desc.Ho * desc.Wo, desc.Co, x.device)
    ns = ctypes.c_int(0)
    call('mi355_conv_fwd_cat', ctypes.byref(desc), ptr(x), ptr(w), ptr(bias), ptr(x2), ptr(w2), ptr(bias2), c2, ptr(y),
         ptr(partial), nbytes, ctypes.byref(ns), stream_ptr())
    return y, ((partial, ns.value) if ns.value > 0 else None)


def conv_dgrad_stats(desc, dy, wT):
    """ConvTranspose2d forward (conv-form dgrad) + BatchNorm statistics partials of its output."""
    _chk_dev(dy, wT)
    dx = nhwc_empty(desc.N, desc.Ci, desc.Hi, desc.Wi, dy.dtype, dy.device)
    partial, nbytes = _stats_buf(desc.N * desc.Hi * desc.Wi, desc.Ci, dy.device)
    ns = ctypes.c_int(0)
    call('mi355_conv_dgrad_stats', ctypes.byref(desc), ptr(dy), ptr(wT), ptr(dx), ptr(partial), nbytes,
         ctypes.byref(ns), stream_ptr())
    return dx, ((partial, ns.value) if ns.value > 0 else None)


def _bn_src(bn):
    """bn = (x, y_or_None, gamma, beta, mean, invstd, relu) -> BnBwdSrc (the tuple keeps the tensors alive)."""
    x, y, gamma, beta, mean, invstd, relu = bn
    return BnBwdSrc(ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), int(bool(relu)))


def conv_dgrad_bnbwd(desc, dy, wT, bn, scale_dev=None, out=None, accumulate=False):
    """conv_dgrad whose result is the dy of the BatchNorm described by `bn`; also returns that BatchNorm's backward
    reduction partials (buffer, nslices) from the epilogue, or None when the launch could not fuse them."""
    _chk_dev(dy, wT)
    _chk_room('conv_dgrad_bnbwd out', out, desc.N * desc.Ci * desc.Hi * desc.Wi)
    dx = out if out is not None else nhwc_empty(desc.N, desc.Ci, desc.Hi, desc.Wi, dy.dtype, dy.device)
    partial, nbytes = _stats_buf(desc.N * desc.Hi * desc.Wi, desc.Ci, dy.device)
    ns = ctypes.c_int(0)
    src = _bn_src(bn)
    call('mi355_conv_dgrad_bnbwd', ctypes.byref(desc), ptr(dy), ptr(wT), ptr(scale_dev), int(accumulate), ptr(dx),
         ctypes.byref(src), ptr(partial), nbytes, ctypes.byref(ns), stream_ptr())
    return dx, ((partial, ns.value) if ns.value > 0 else None)


def conv_fwd_bnbwd(desc, x, w, bn):
    """conv_fwd (the input gradient of a ConvTranspose2d) whose result is the dy of the BatchNorm `bn`."""
    _chk_dev(x, w)
    y = nhwc_empty(desc.N, desc.Co, desc.Ho, desc.Wo, x.dtype, x.device)
    partial, nbytes = _stats_buf(desc.N * desc.Ho * desc.Wo, desc.Co, x.device)
    ns = ctypes.c_int(0)
    src = _bn_src(bn)
    call('mi355_conv_fwd_bnbwd', ctypes.byref(desc), ptr(x), ptr(w), ptr(y), ctypes.byref(src), ptr(partial), nbytes,
         ctypes.byref(ns), stream_ptr())
    return y, ((partial, ns.value) if ns.value > 0 else None)


def conv_dgrad(desc, dy, wT, scale_dev=None, out=None, accumulate=False):
    _chk_dev(dy, wT)
    _chk_room('conv_dgrad out', out, desc.N * desc.Ci * desc.Hi * desc.Wi)
    dx = out if out is not None else nhwc_empty(desc.N, desc.Ci, desc.Hi, desc.Wi, dy.dtype, dy.device)
    call('mi355_conv_dgrad', ctypes.byref(desc), ptr(dy), ptr(wT), 0, ptr(scale_dev), int(accumulate), ptr(dx),
         stream_ptr())
    return dx


def conv_dgrad_masked_acc(desc, dy, wT, out, acc_mask, scale_dev=None):
    """out <- conv_dgrad(dy) + (bit of acc_mask set ? out : 0), in place; returns out."""
    _chk_dev(dy, wT, out, acc_mask)
    n = desc.N * desc.Ci * desc.Hi * desc.Wi
    _chk_room('conv_dgrad_masked_acc out', out, n)
    _chk_room('conv_dgrad_masked_acc acc_mask', acc_mask, n // (8 if out.dtype == torch.bfloat16 else 4))
    call('mi355_conv_dgrad_masked_acc', ctypes.byref(desc), ptr(dy), ptr(wT), ptr(scale_dev), ptr(out), ptr(acc_mask), stream_ptr())
    return out


def apply_relu_mask(g, mask):
    """g <- bit of mask set ? g : 0, in place (g channels_last bf16 / fp32, mask from bn_relu_mask); returns g."""
    _chk_dev(g, mask)
    N, C, H, W = g.shape
    _chk_room('apply_relu_mask mask', mask, g.numel() // (8 if g.dtype == torch.bfloat16 else 4))
    call('mi355_apply_relu_mask', ptr(g), ptr(mask), N * H * W, C, dtype_code(g.dtype), stream_ptr())
    return g


def conv_wgrad(desc, x, dy, dw, accumulate, ws_tag='main'):
    """dw: fp32 buffer in [Co][kh][kw][Ci] memory order (Ci = desc.Ci, i.e. padded for the stem)."""
    _chk_dev(x, dy, dw)
    _chk_room('conv_wgrad dw', dw, desc.Co * desc.kh * desc.kw * desc.Ci)
    need = load().mi355_conv_wgrad_workspace(ctypes.byref(desc))
    ws = workspace(need, x.device, ws_tag)
    call('mi355_conv_wgrad', ctypes.byref(desc), ptr(x), ptr(dy), ptr(dw), int(accumulate), ptr(ws), ws.numel(),
         stream_ptr())


def conv_wgrad_grouped(items, ws_tag='main'):
    """items: list of (desc, x, dy, dw, accumulate) as for conv_wgrad.  One C call: small problems share launches."""
    n = len(items)
    arr = (WgradItem * n)()
    for i, (desc, x, dy, dw, acc) in enumerate(items):
        _chk_dev(x, dy, dw)
        _chk_room('conv_wgrad_grouped dw', dw, desc.Co * desc.kh * desc.kw * desc.Ci)
        arr[i].d = desc
        arr[i].x, arr[i].dy, arr[i].dw, arr[i].accumulate = ptr(x), ptr(dy), ptr(dw), int(acc)
    need = load().mi355_conv_wgrad_grouped_workspace(arr, n)
    ws = workspace(need, items[0][1].device, ws_tag)
    call('mi355_conv_wgrad_grouped', arr, n, ptr(ws), ws.numel(), stream_ptr())


def pack_weights(w_master, O, T, I, Ipad, dtype, want_f=True, want_t=True):
    """fp32 master in [O][T][I] memory order -> (wf [O][T][Ipad], wt [Ipad][T][O]) in `dtype`."""
    _chk_dev(w_master)
    dev = w_master.device
    wf = torch.empty(O * T * Ipad, dtype=dtype, device=dev) if want_f else None
    wt = torch.empty(Ipad * T * O, dtype=dtype, device=dev) if want_t else None
    call('mi355_pack_weights', ptr(w_master), ptr(wf), ptr(wt), O, T, I, Ipad, dtype_code(dtype), stream_ptr())
    return wf, wt


def pack_weights_batched(table, nitems, total_blocks, dtype):
    """table: uint8 device tensor holding `nitems` mi355_pack_item records."""
    call('mi355_pack_weights_batched', ptr(table), int(nitems), int(total_blocks), dtype_code(dtype), stream_ptr())


def pack_weights_into(w_master, wf, wt, O, T, I, Ipad, dtype):
    call('mi355_pack_weights', ptr(w_master), ptr(wf), ptr(wt), O, T, I, Ipad, dtype_code(dtype), stream_ptr())


def colsum(dy, out, accumulate):
    """out[C] (=|+=) column sums of the channels_last tensor dy."""
    N, C, H, W = dy.shape
    _chk_room('colsum out', out, C)
    rows = N * H * W
    ws = workspace(load().mi355_colsum_workspace(rows, C), dy.device)
    call('mi355_colsum', ptr(dy), ptr(out), rows, C, dtype_code(dy.dtype), int(accumulate), ptr(ws), ws.numel(),
         stream_ptr())


# ---------------------------------------------------------------- fp8 operand path (conv forward / input gradient)
E4M3, E5M2 = 0, 1
FP8_MARGIN = 0          # scale = 2^k, k = the largest integer with amax * 2^margin * 2^k <= fmt_max, clamped to [-126, 126]


def fp8_state(device):
    """{scale, descale, amax bits, pad} of one per-tensor scaled fp8 operand (device floats)."""
    return torch.zeros(4, dtype=torch.float32, device=device)


def fp8_amax(x, state):
    _chk_dev(x, state)
    call('mi355_fp8_quantize', ptr(x), 0, ptr(state), x.numel(), dtype_code(x.dtype), 0, 0, stream_ptr())


def fp8_update_scale(states, n=1, fmt=E4M3, margin=None):
    call('mi355_fp8_update_scale', ptr(states), int(n), 4, int(fmt), FP8_MARGIN if margin is None else int(margin), stream_ptr())


def fp8_quantize(x, state, fmt=E4M3, jit=False):
    """bf16 / fp32 device tensor (any dense layout) -> uint8 tensor of the same shape and strides holding
    saturate_fmt(x * state[0]).  jit=True: first take amax(|x|) and derive the scale from it (one extra read of x);
    otherwise the scale already in `state` is used and the amax of x is recorded for the next update (delayed scaling).
    The returned tensor's `_mi_rec` is a 4-float record {scale, descale, 0, 0} of THIS copy, usable wherever a state is."""
    _chk_dev(x, state)
    if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        raise Mi355Error('fp8_quantize needs a dense tensor')
    if x.numel() % 16:
        raise Mi355Error('fp8_quantize needs a multiple of 16 elements, got %d' % x.numel())
    if jit:
        fp8_amax(x, state)
        fp8_update_scale(state, 1, fmt)
    # the copy carries its own {scale, descale, 0, 0} record in 16 bytes behind the data (q._mi_rec): the stream's state is
    # refreshed at every optimizer step, a copy may be consumed after that (weight gradient of a forward shared by two backwards)
    n = x.numel()
    full = torch.empty(n + 16, dtype=torch.uint8, device=x.device)
    q = full.as_strided(x.shape, x.stride())
    call('mi355_fp8_quantize', ptr(x), ptr(full), ptr(state), n, dtype_code(x.dtype), int(fmt), 2, stream_ptr())
    q._mi_rec = full[n:].view(torch.float32)
    return q


def pack_weights_fp8(w_master, O, T, I, state, wf=None, wt=None, jit=True):
    """fp32 master in [O][T][I] memory order -> e4m3 (wf [O][T][I], wt [I][T][O]); jit: per-tensor scale from this very
    tensor (3 launches), else the scale already in `state` (1 launch; the amax is recorded for the next update)."""
    _chk_dev(w_master, state)
    dev = w_master.device
    wf = torch.empty(O * T * I, dtype=torch.uint8, device=dev) if wf is None else wf
    wt = torch.empty(O * T * I, dtype=torch.uint8, device=dev) if wt is None else wt
    call('mi355_pack_weights_fp8', ptr(w_master), ptr(wf), ptr(wt), ptr(state), O, T, I, FP8_MARGIN if jit else -1, stream_ptr())
    return wf, wt


def pack_weights_fp8_batched(table, nitems, total_blocks):
    """table: uint8 device tensor holding `nitems` mi355_pack8_item records."""
    call('mi355_pack_weights_fp8_batched', ptr(table), int(nitems), int(total_blocks), stream_ptr())


def make_desc_fp8(N, Hi, Wi, Ci, Co, kh, kw, stride, pad):
    Ho = (Hi + 2 * pad - kh) // stride + 1
    Wo = (Wi + 2 * pad - kw) // stride + 1
    return ConvDesc(N, Hi, Wi, Ci, Ho, Wo, Co, kh, kw, stride, pad, FP8)


def conv_fwd_fp8(desc, x8, x_state, w8, w_state, bias=None, residual=None, want_stats=False, x_fmt=E4M3):
    """y (bf16, channels_last) = conv(x8, w8) * descale_x * descale_w + bias (+ residual); optionally the BatchNorm
    statistics partials of y.  Returns y or (y, (partial, nslices) | None)."""
    _chk_dev(x8, w8)
    y = nhwc_empty(desc.N, desc.Co, desc.Ho, desc.Wo, torch.bfloat16, x8.device)
    partial, nbytes, ns = None, 0, ctypes.c_int(0)
    if want_stats:
        partial, nbytes = _stats_buf(desc.N * desc.Ho * desc.Wo, desc.Co, x8.device)
    call('mi355_conv_fwd_fp8', ctypes.byref(desc), ptr(x8), int(x_fmt), ptr(w8), ptr(x_state[1:2]), ptr(w_state[1:2]), ptr(bias),
         ptr(residual), ptr(y), ptr(partial), nbytes, ctypes.byref(ns), stream_ptr())
    if want_stats:
        return y, ((partial, ns.value) if ns.value > 0 else None)
    return y


def conv_dgrad_fp8(desc, dy8, dy_state, wT8, w_state, scale_dev=None, out=None, accumulate=False, want_stats=False, dy_fmt=E5M2):
    """dx (bf16) = dgrad(dy8, wT8) * descale_dy * descale_w (* *scale_dev) (+ dx when accumulate)."""
    _chk_dev(dy8, wT8)
    _chk_room('conv_dgrad_fp8 out', out, desc.N * desc.Ci * desc.Hi * desc.Wi)
    dx = out if out is not None else nhwc_empty(desc.N, desc.Ci, desc.Hi, desc.Wi, torch.bfloat16, dy8.device)
    partial, nbytes, ns = None, 0, ctypes.c_int(0)
    if want_stats:
        partial, nbytes = _stats_buf(desc.N * desc.Hi * desc.Wi, desc.Ci, dy8.device)
    call('mi355_conv_dgrad_fp8', ctypes.byref(desc), ptr(dy8), int(dy_fmt), ptr(wT8), ptr(dy_state[1:2]), ptr(w_state[1:2]),
         ptr(scale_dev), int(accumulate), ptr(dx), ptr(partial), nbytes, ctypes.byref(ns), stream_ptr())
    if want_stats:
        return dx, ((partial, ns.value) if ns.value > 0 else None)
    return dx


def conv_wgrad_fp8(desc, x8, x_state, dy8, dy_state, dw, accumulate, dy_fmt=E5M2, x_fmt=E4M3, ws_tag='main'):
    """dw (fp32, [Co][kh][kw][Ci]) (+)= wgrad(x8, dy8) * descale_x * descale_dy for the 3x3 / stride-1 and the 3x3 / 4x4 /
    stride-2 layers: both operands are the fp8 copies the forward / input-gradient launches of the layer already made."""
    _chk_dev(x8, dy8, dw)
    _chk_room('conv_wgrad_fp8 dw', dw, desc.Co * desc.kh * desc.kw * desc.Ci)
    need = load().mi355_conv_wgrad_fp8_workspace(ctypes.byref(desc))
    ws = workspace(need, x8.device, ws_tag)
    call('mi355_conv_wgrad_fp8', ctypes.byref(desc), ptr(x8), int(x_fmt), ptr(dy8), int(dy_fmt), ptr(x_state[1:2]),
         ptr(dy_state[1:2]), ptr(dw), int(accumulate), ptr(ws), ws.numel(), stream_ptr())


# ---------------------------------------------------------------- MX (block-scaled) fp8 operand path ('mxfp8' mode)
MX_BLOCK = 32


def mx_quantize(x, q=None, scales=None):
    """bf16 / fp32 device tensor whose last memory axis (C, a multiple of 32) is contiguous -- an NHWC feature map or any
    [rows][C] array -> (q, scales): e4m3 bytes shaped and strided like x, and one E8M0 byte per 32 consecutive elements of
    a row, a uint8 tensor of x.numel() / 32 elements ([rows][C/32]).  No state (mx_fp8.hip has the scale rule)."""
    _chk_dev(x)
    if x.dim() == 4 and is_nhwc(x):
        C = x.shape[1]
    elif x.is_contiguous():
        C = x.shape[-1] if x.dim() else 1
    else:
        raise Mi355Error('mx_quantize needs a contiguous or channels_last tensor')
    if C % MX_BLOCK or C < MX_BLOCK:
        raise Mi355Error('mx_quantize: the contiguous axis (%d) must be a multiple of %d' % (C, MX_BLOCK))
    n = x.numel()
    _chk_room('mx_quantize q', q, n)
    _chk_room('mx_quantize scales', scales, n // MX_BLOCK)
    q = q if q is not None else torch.empty_strided(x.shape, x.stride(), dtype=torch.uint8, device=x.device)
    scales = scales if scales is not None else torch.empty(n // MX_BLOCK, dtype=torch.uint8, device=x.device)
    _chk_dev(q, scales)
    call('mi355_mx_quantize', ptr(x), ptr(q), ptr(scales), n // C, C, dtype_code(x.dtype), stream_ptr())
    return q, scales


def pack_weights_mx(w_master, O, T, I, wf=None, sf=None, wt=None, st=None):
    """fp32 master in [O][T][I] memory order -> (wf e4m3 [O][T][I], sf [O][T][I/32], wt e4m3 [I][T][O], st [I][T][O/32]),
    flat uint8 tensors; both packs quantised from the master."""
    _chk_dev(w_master)
    if w_master.dtype != torch.float32:
        raise Mi355Error('pack_weights_mx: the master must be fp32')
    n = O * T * I
    _chk_room('pack_weights_mx master', w_master, n)
    dev = w_master.device
    for what, t, need in (('wf', wf, n), ('sf', sf, n // MX_BLOCK), ('wt', wt, n), ('st', st, n // MX_BLOCK)):
        _chk_room('pack_weights_mx ' + what, t, need)
    wf = torch.empty(n, dtype=torch.uint8, device=dev) if wf is None else wf
    wt = torch.empty(n, dtype=torch.uint8, device=dev) if wt is None else wt
    sf = torch.empty(n // MX_BLOCK, dtype=torch.uint8, device=dev) if sf is None else sf
    st = torch.empty(n // MX_BLOCK, dtype=torch.uint8, device=dev) if st is None else st
    _chk_dev(wf, sf, wt, st)
    call('mi355_pack_weights_mx', ptr(w_master), ptr(wf), ptr(sf), ptr(wt), ptr(st), int(O), int(T), int(I), stream_ptr())
    return wf, sf, wt, st


def pack_weights_mx_batched(table, nitems, total_blocks):
    """table: uint8 device tensor holding `nitems` mi355_packmx_item records."""
    _chk_dev(table)
    _chk_room('pack_weights_mx_batched table', table, nitems * 56)
    call('mi355_pack_weights_mx_batched', ptr(table), int(nitems), int(total_blocks), stream_ptr())


def conv_fwd_mx(desc, x8, sx, w8, sw, bias=None, residual=None, want_stats=False, out=None):
    """y (bf16, channels_last) = conv(x8 * 2^sx, w8 * 2^sw) + bias (+ residual) on MX operands (desc from make_desc_fp8);
    optionally the BatchNorm statistics partials of y.  Returns y or (y, (partial, nslices) | None)."""
    _chk_dev(x8, sx, w8, sw)
    nx, nw = desc.N * desc.Hi * desc.Wi * desc.Ci, desc.Co * desc.kh * desc.kw * desc.Ci
    for what, t, need in (('x8', x8, nx), ('sx', sx, nx // MX_BLOCK), ('w8', w8, nw), ('sw', sw, nw // MX_BLOCK),
                          ('residual', residual, desc.N * desc.Ho * desc.Wo * desc.Co), ('bias', bias, desc.Co),
                          ('out', out, desc.N * desc.Ho * desc.Wo * desc.Co)):
        _chk_room('conv_fwd_mx ' + what, t, need)
    y = out if out is not None else nhwc_empty(desc.N, desc.Co, desc.Ho, desc.Wo, torch.bfloat16, x8.device)
    partial, nbytes, ns = None, 0, ctypes.c_int(0)
    if want_stats:
        partial, nbytes = _stats_buf(desc.N * desc.Ho * desc.Wo, desc.Co, x8.device)
    call('mi355_conv_fwd_mx', ctypes.byref(desc), ptr(x8), ptr(sx), ptr(w8), ptr(sw), ptr(bias), ptr(residual), ptr(y),
         ptr(partial), nbytes, ctypes.byref(ns) if want_stats else None, stream_ptr())
    if want_stats:
        return y, ((partial, ns.value) if ns.value > 0 else None)
    return y


def conv_dgrad_mx(desc, dy8, sdy, wT8, swT, scale_dev=None, out=None, accumulate=False, want_stats=False):
    """dx (bf16) = dgrad(dy8 * 2^sdy, wT8 * 2^swT) (* *scale_dev) (+ dx when accumulate) on MX operands."""
    _chk_dev(dy8, sdy, wT8, swT)
    ndy, nw = desc.N * desc.Ho * desc.Wo * desc.Co, desc.Co * desc.kh * desc.kw * desc.Ci
    for what, t, need in (('dy8', dy8, ndy), ('sdy', sdy, ndy // MX_BLOCK), ('wT8', wT8, nw), ('swT', swT, nw // MX_BLOCK),
                          ('out', out, desc.N * desc.Ci * desc.Hi * desc.Wi)):
        _chk_room('conv_dgrad_mx ' + what, t, need)
    dx = out if out is not None else nhwc_empty(desc.N, desc.Ci, desc.Hi, desc.Wi, torch.bfloat16, dy8.device)
    partial, nbytes, ns = None, 0, ctypes.c_int(0)
    if want_stats:
        partial, nbytes = _stats_buf(desc.N * desc.Hi * desc.Wi, desc.Ci, dy8.device)
    call('mi355_conv_dgrad_mx', ctypes.byref(desc), ptr(dy8), ptr(sdy), ptr(wT8), ptr(swT), ptr(scale_dev), int(accumulate),
         ptr(dx), ptr(partial), nbytes, ctypes.byref(ns) if want_stats else None, stream_ptr())
    if want_stats:
        return dx, ((partial, ns.value) if ns.value > 0 else None)
    return dx


def conv_fwd_mx_act(desc, x8, sx, w8, sw, bias=None, residual=None, relu=False, want_copy=False, out=None, out8=None, out_scales=None):
    """Inference: y (bf16, channels_last) = act(conv(x8 * 2^sx, w8 * 2^sw) + bias (+ residual)) on MX operands (desc from
    make_desc_fp8), the BatchNorm behind the conv folded into w8 / bias by the caller.  want_copy: the launch also writes the MX
    copy of y -- (y8 e4m3 shaped and strided like y, sy [pixels][Co/32]) = what mx_quantize(y) returns -- and the result is
    (y, y8, sy)."""
    _chk_dev(x8, sx, w8, sw)
    nx, nw, ny = desc.N * desc.Hi * desc.Wi * desc.Ci, desc.Co * desc.kh * desc.kw * desc.Ci, desc.N * desc.Ho * desc.Wo * desc.Co
    want_copy = bool(want_copy) or out8 is not None or out_scales is not None
    for what, t, need in (('x8', x8, nx), ('sx', sx, nx // MX_BLOCK), ('w8', w8, nw), ('sw', sw, nw // MX_BLOCK),
                          ('residual', residual, ny), ('bias', bias, desc.Co), ('out', out, ny), ('out8', out8, ny),
                          ('out_scales', out_scales, ny // MX_BLOCK)):
        _chk_room('conv_fwd_mx_act ' + what, t, need)
    y = out if out is not None else nhwc_empty(desc.N, desc.Co, desc.Ho, desc.Wo, torch.bfloat16, x8.device)
    y8 = sy = None
    if want_copy:
        if desc.Co % MX_BLOCK:
            raise Mi355Error('conv_fwd_mx_act: an MX copy of the output needs a multiple of %d output channels (%d)' % (MX_BLOCK, desc.Co))
        y8 = out8 if out8 is not None else torch.empty_strided(y.shape, y.stride(), dtype=torch.uint8, device=y.device)
        sy = out_scales if out_scales is not None else torch.empty(ny // MX_BLOCK, dtype=torch.uint8, device=y.device)
        _chk_dev(y8, sy)
    call('mi355_conv_fwd_mx_act', ctypes.byref(desc), ptr(x8), ptr(sx), ptr(w8), ptr(sw), ptr(bias), ptr(residual), int(bool(relu)),
         ptr(y), ptr(y8), ptr(sy), stream_ptr())
    return (y, y8, sy) if want_copy else y


def conv_dgrad_mx_act(desc, dy8, sdy, wT8, swT, bias=None, relu=False, want_copy=False, out=None, out8=None, out_scales=None):
    """Inference ConvTranspose2d forward on MX operands: dx (bf16) = act(dgrad(dy8 * 2^sdy, wT8 * 2^swT) + bias); want_copy as in
    conv_fwd_mx_act: (dx, dx8, sdx) with the MX copy of dx written by the same launch."""
    _chk_dev(dy8, sdy, wT8, swT)
    ndy, nw, nx = desc.N * desc.Ho * desc.Wo * desc.Co, desc.Co * desc.kh * desc.kw * desc.Ci, desc.N * desc.Ci * desc.Hi * desc.Wi
    want_copy = bool(want_copy) or out8 is not None or out_scales is not None
    for what, t, need in (('dy8', dy8, ndy), ('sdy', sdy, ndy // MX_BLOCK), ('wT8', wT8, nw), ('swT', swT, nw // MX_BLOCK),
                          ('bias', bias, desc.Ci), ('out', out, nx), ('out8', out8, nx), ('out_scales', out_scales, nx // MX_BLOCK)):
        _chk_room('conv_dgrad_mx_act ' + what, t, need)
    dx = out if out is not None else nhwc_empty(desc.N, desc.Ci, desc.Hi, desc.Wi, torch.bfloat16, dy8.device)
    dx8 = sdx = None
    if want_copy:
        if desc.Ci % MX_BLOCK:
            raise Mi355Error('conv_dgrad_mx_act: an MX copy of the output needs a multiple of %d output channels (%d)' % (MX_BLOCK, desc.Ci))
        dx8 = out8 if out8 is not None else torch.empty_strided(dx.shape, dx.stride(), dtype=torch.uint8, device=dx.device)
        sdx = out_scales if out_scales is not None else torch.empty(nx // MX_BLOCK, dtype=torch.uint8, device=dx.device)
        _chk_dev(dx8, sdx)
    call('mi355_conv_dgrad_mx_act', ctypes.byref(desc), ptr(dy8), ptr(sdy), ptr(wT8), ptr(swT), ptr(bias), int(bool(relu)),
         ptr(dx), ptr(dx8), ptr(sdx), stream_ptr())
    return (dx, dx8, sdx) if want_copy else dx


# ---------------------------------------------------------------- batch norm
def bn_relu_mask(x):
    """uint8 buffer for the ReLU bit mask of a BatchNorm over x: one byte per 16-byte chunk of every row."""
    per = 8 if x.dtype == torch.bfloat16 else 4
    return torch.empty(x.numel() // per, dtype=torch.uint8, device=x.device)


def bn_train_fwd(x, residual, gamma, beta, running_mean, running_var, nbt, eps, momentum, relu, stat_updates=1,
                 partial=None, relu_mask=None, q8=None):
    """partial: (buffer, nslices) from conv_fwd_stats / conv_dgrad_stats of the conv that produced x -> no statistics pass.
    relu_mask: bn_relu_mask(x) buffer that receives the (y > 0) bits for the backward (instead of keeping y).
    q8: (uint8 tensor shaped like y, fp8 state) -> also the e4m3 copy of y, scaled by state[0], and its amax."""
    q8_out, q8_state = q8 if q8 is not None else (None, None)
    _chk_dev(x, gamma)
    N, C, H, W = x.shape
    rows = N * H * W
    y = nhwc_empty(N, C, H, W, x.dtype, x.device)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    if partial is not None:
        buf, ns = partial
        ss = torch.empty(2 * C, dtype=torch.float32, device=x.device)
        call('mi355_bn_train_fwd_partials', ptr(x), ptr(residual), ptr(y), ptr(gamma), ptr(beta), ptr(running_mean),
             ptr(running_var), ptr(nbt), ptr(mean), ptr(invstd), rows, C, float(eps), float(momentum), int(stat_updates),
             int(relu), dtype_code(x.dtype), ptr(buf), int(ns), ptr(ss), ptr(relu_mask), ptr(q8_out), ptr(q8_state), stream_ptr())
        return y, mean, invstd
    ws = workspace(load().mi355_bn_workspace(rows, C), x.device)
    call('mi355_bn_train_fwd', ptr(x), ptr(residual), ptr(y), ptr(gamma), ptr(beta), ptr(running_mean),
         ptr(running_var), ptr(nbt), ptr(mean), ptr(invstd), rows, C, float(eps), float(momentum), int(stat_updates), int(relu),
         dtype_code(x.dtype), ptr(ws), ws.numel(), ptr(relu_mask), ptr(q8_out), ptr(q8_state), stream_ptr())
    return y, mean, invstd


def bn_relu_maxpool_fwd(x, gamma, beta, running_mean, running_var, nbt, eps, momentum, stat_updates, partial):
    """BatchNorm (train, statistics partials of the producing conv) + ReLU + MaxPool2d(3, 2, 1) in one pass; returns
    (y_pool, argidx, mean, invstd)."""
    _chk_dev(x, gamma)
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = nhwc_empty(N, C, Ho, Wo, x.dtype, x.device)
    arg = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    ss = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    buf, ns = partial
    call('mi355_bn_relu_maxpool_fwd_partials', ptr(x), ptr(y), ptr(arg), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
         ptr(nbt), ptr(mean), ptr(invstd), N, H, W, C, float(eps), float(momentum), int(stat_updates), dtype_code(x.dtype), ptr(buf),
         int(ns), ptr(ss), stream_ptr())
    return y, arg, mean, invstd


def bn_eval_fwd(x, residual, gamma, beta, running_mean, running_var, eps, relu):
    _chk_dev(x, gamma)
    N, C, H, W = x.shape
    y = nhwc_empty(N, C, H, W, x.dtype, x.device)
    call('mi355_bn_eval_fwd', ptr(x), ptr(residual), ptr(y), ptr(gamma), ptr(beta), ptr(running_mean),
         ptr(running_var), N * H * W, C, float(eps), int(relu), dtype_code(x.dtype), stream_ptr())
    return y


def bn_bwd(dy, x, y, gamma, mean, invstd, dgamma, dbeta, accumulate, relu, want_dres, beta=None, partial=None, relu_mask=None,
           q8=None):
    """partial: (buffer, nslices) reduction partials from the GEMM epilogue that produced dy -> no reduction pass.
    relu_mask: the bit mask the forward wrote (then y is not needed).
    q8: (uint8 tensor shaped like dx, fp8 state) -> also the e5m2 copy of dx, scaled by state[0], and its amax."""
    q8_out, q8_state = q8 if q8 is not None else (None, None)
    N, C, H, W = x.shape
    rows = N * H * W
    dx = nhwc_empty(N, C, H, W, x.dtype, x.device)
    dres = nhwc_empty(N, C, H, W, x.dtype, x.device) if want_dres else None
    if partial is not None:
        buf, ns = partial
        coeff = torch.empty(3 * C, dtype=torch.float32, device=x.device)
        call('mi355_bn_bwd_partials', ptr(dy), ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), ptr(dx),
             ptr(dres), ptr(dgamma), ptr(dbeta), int(accumulate), rows, C, int(relu), dtype_code(x.dtype), ptr(buf), int(ns),
             ptr(coeff), ptr(relu_mask), ptr(q8_out), ptr(q8_state), stream_ptr())
        return dx, dres
    ws = workspace(load().mi355_bn_workspace(rows, C), x.device)
    call('mi355_bn_bwd', ptr(dy), ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), ptr(dx), ptr(dres),
         ptr(dgamma), ptr(dbeta), int(accumulate), rows, C, int(relu), dtype_code(x.dtype), ptr(ws), ws.numel(),
         ptr(relu_mask), ptr(q8_out), ptr(q8_state), stream_ptr())
    return dx, dres


# ---------------------------------------------------------------- max pool
def bn_resident_timeouts():
    """Grid-barrier spins of the one-launch BatchNorm backward that gave up since the library was loaded or the last reset
    (0 = healthy).  Every such launch has written NaN into the gradients it produced.  Synchronises the device."""
    n = ctypes.c_uint(0)
    call('mi355_bn_resident_timeouts', ctypes.byref(n))
    return n.value


def bn_resident_reset():
    call('mi355_bn_resident_reset')


def bn_set_resident(on):
    """Switch the one-launch BatchNorm backward on (1), off (0: always reduce + finalize + apply) or back to the environment's
    choice (-1); returns the previous setting, to be handed back to this function."""
    return int(load().mi355_bn_set_resident(int(on)))


def bn_resident_set_spin_limit(limit):
    """Test hook: poll iterations before a block of the one-launch BatchNorm backward gives up (0 = default)."""
    call('mi355_bn_resident_set_spin_limit', int(limit))


def bn_resident_check(where=''):
    """Raise when a one-launch BatchNorm backward could not get all its blocks onto the chip since the last check: its gradients
    are NaN (csrc/bn.hip bn_bwd_resident_kernel).  The one-launch form is switched off for the rest of the process and the counters
    are cleared, so a caller that catches the error can redo the step on the three-launch path.  Synchronises the device: call it
    where the host waits anyway (train1.py: once per epoch; bench.py / smoke: at the end)."""
    n = bn_resident_timeouts()
    if n:
        load().mi355_bn_set_resident(0)
        bn_resident_reset()
        raise Mi355Error('%d grid-barrier give-up(s) in the one-launch BatchNorm backward%s: another kernel or process held CUs while '
                         'it ran, the gradients of those launches are NaN.  The one-launch form is now off for this process '
                         '(MI355_BN_RESIDENT=0 makes that the default); redo the affected steps.' % (n, (' (' + where + ')') if where else ''))


def maxpool_fwd(x):
    _chk_dev(x)
    _chk_feature('maxpool_fwd x', x)
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = nhwc_empty(N, C, Ho, Wo, x.dtype, x.device)
    arg = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    call('mi355_maxpool_fwd', ptr(x), ptr(y), ptr(arg), N, H, W, C, dtype_code(x.dtype), stream_ptr())
    return y, arg


def maxpool_bwd(dy, arg, in_shape):
    N, C, H, W = in_shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _chk_dev(dy, arg)
    _chk_feature('maxpool_bwd dy', dy, (N, C, Ho, Wo))
    if arg.dtype != torch.uint8 or not arg.is_contiguous():
        raise Mi355Error('maxpool_bwd arg: needs the contiguous uint8 window codes of maxpool_fwd, got %s strides %s' % (arg.dtype, arg.stride()))
    _chk_room('maxpool_bwd arg', arg, N * Ho * Wo * C)
    dx = nhwc_empty(N, C, H, W, dy.dtype, dy.device)
    call('mi355_maxpool_bwd', ptr(dy), ptr(arg), ptr(dx), N, H, W, C, dtype_code(dy.dtype), stream_ptr())
    return dx


# ---------------------------------------------------------------- 21-channel pointwise convs
def conv1x1_heatmap(x, w_packed, bias, K):
    """MFMA form of the C -> K heat-map conv: x channels_last [N,C,H,W], w_packed [K][C] in x.dtype -> [N,K,H,W] fp32."""
    N, C, H, W = x.shape
    y = torch.empty((N, K, H, W), dtype=torch.float32, device=x.device)
    call('mi355_conv1x1_heatmap', ptr(x), ptr(w_packed), ptr(bias), ptr(y), N, H * W, C, K, dtype_code(x.dtype), stream_ptr())
    return y


def pw_c2k(x, w, bias, K, w_transposed=False):
    """x channels_last [N,C,H,W] -> heat-map [N,K,H,W] fp32 contiguous."""
    _chk_dev(x, w, bias)
    _chk_feature('pw_c2k x', x)
    N, C, H, W = x.shape
    _chk_room('pw_c2k w', w, K * C)
    _chk_room('pw_c2k bias', bias, K)
    y = torch.empty((N, K, H, W), dtype=torch.float32, device=x.device)
    call('mi355_pw_c2k', ptr(x), ptr(w), ptr(bias), ptr(y), N, H * W, C, K, int(w_transposed), dtype_code(x.dtype),
         stream_ptr())
    return y


def _chk_k2c(what, y, w, bias, C, dtype, residual, scale_dev):
    _chk_dev(y, w, bias, residual, scale_dev)
    _chk_heatmap(what + ' y', y)
    N, K, H, W = y.shape
    _chk_room(what + ' w', w, K * C)
    _chk_room(what + ' bias', bias, C)
    _chk_feature(what + ' residual', residual, (N, C, H, W))
    if residual is not None and residual.dtype != dtype:
        raise Mi355Error('%s residual: %s, the output is %s' % (what, residual.dtype, dtype))


def pw_k2c(y, w, bias, C, dtype, residual=None, scale_dev=None, w_transposed=False):
    """heat-map [N,K,H,W] fp32 -> channels_last [N,C,H,W] `dtype`."""
    _chk_k2c('pw_k2c', y, w, bias, C, dtype, residual, scale_dev)
    N, K, H, W = y.shape
    out = nhwc_empty(N, C, H, W, dtype, y.device)
    call('mi355_pw_k2c', ptr(y), ptr(w), ptr(bias), ptr(residual), ptr(scale_dev), ptr(out), N, H * W, C, K,
         int(w_transposed), dtype_code(dtype), stream_ptr())
    return out


def pw_k2c_stats(y, w, bias, C, dtype, residual=None):
    """pw_k2c + BatchNorm statistics partials of its output.  Returns (out, (partial, nslices))."""
    _chk_k2c('pw_k2c_stats', y, w, bias, C, dtype, residual, None)
    N, K, H, W = y.shape
    out = nhwc_empty(N, C, H, W, dtype, y.device)
    ns_max = N * ((H * W + 63) // 64)
    partial = torch.empty(ns_max * C * 3, dtype=torch.float32, device=y.device)
    ns = ctypes.c_int(0)
    call('mi355_pw_k2c_stats', ptr(y), ptr(w), ptr(bias), ptr(residual), None, ptr(out), N, H * W, C, K, 0,
         dtype_code(dtype), ptr(partial), partial.numel() * 4, ctypes.byref(ns), stream_ptr())
    return out, (partial, ns.value)


def pw_wgrad(x, y, dw, kc_layout, accumulate):
    _chk_dev(x, y, dw)
    _chk_feature('pw_wgrad x', x)
    _chk_heatmap('pw_wgrad y', y)
    N, C, H, W = x.shape
    K = y.shape[1]
    if (y.shape[0], y.shape[2], y.shape[3]) != (N, H, W):
        raise Mi355Error('pw_wgrad y: shape %s does not match the features %s' % (tuple(y.shape), tuple(x.shape)))
    _chk_room('pw_wgrad dw', dw, C * K)
    ws = workspace(load().mi355_pw_wgrad_workspace(N, H * W, C, K), x.device)
    call('mi355_pw_wgrad', ptr(x), ptr(y), ptr(dw), int(kc_layout), int(accumulate), N, H * W, C, K,
         dtype_code(x.dtype), ptr(ws), ws.numel(), stream_ptr())


def hm_rowsum(y, out, accumulate):
    N, K, H, W = y.shape
    _chk_room('hm_rowsum out', out, K)
    ws = workspace(N * K * 4, y.device)
    call('mi355_hm_rowsum', ptr(y), ptr(out), int(accumulate), N, K, H * W, ptr(ws), ws.numel(), stream_ptr())


# ---------------------------------------------------------------- heat-map decode / losses
def _hm(t):
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    _chk_dev(t)
    return t


def argmax2d(hm):
    """(idx int32 [B,K], xy fp32 [B,K,2], maxval fp32 [B,K,1]) with numpy's first-max tie rule."""
    hm = _hm(hm)
    B, K, H, W = hm.shape
    idx = torch.empty((B, K), dtype=torch.int32, device=hm.device)
    xy = torch.empty((B, K, 2), dtype=torch.float32, device=hm.device)
    mv = torch.empty((B, K, 1), dtype=torch.float32, device=hm.device)
    call('mi355_argmax2d', ptr(hm), ptr(idx), ptr(xy), ptr(mv), B * K, H, W, stream_ptr())
    return idx, xy, mv


def softargmax(hm, beta=100.0, out_scale=4.0):
    hm = _hm(hm)
    B, K, H, W = hm.shape
    uv = torch.empty((B, K, 2), dtype=torch.float32, device=hm.device)
    call('mi355_softargmax', ptr(hm), ptr(uv), B * K, H, W, float(beta), float(out_scale), stream_ptr())
    return uv


def kl_heatmap(pred, target, weight, eps, want_grad, coeff=1.0):
    """Returns (loss_rows [B,K], unit_grad [B,K,H,W] or None); unit_grad = d(coeff * mean over B*K)/d pred."""
    pred, target = _hm(pred), _hm(target)
    B, K, H, W = pred.shape
    if tuple(target.shape) != (B, K, H, W):
        raise Mi355Error('kl_heatmap: pred %s vs target %s' % (tuple(pred.shape), tuple(target.shape)))
    rows = torch.empty((B, K), dtype=torch.float32, device=pred.device)
    g = torch.empty_like(pred) if want_grad else None
    if weight is not None:
        weight = weight.reshape(B, K).float().contiguous()
    call('mi355_kl_heatmap', ptr(pred), ptr(target), ptr(weight), float(eps), ptr(rows), ptr(g), B * K, H * W,
         float(coeff) / (B * K), stream_ptr())
    return rows, g


def coord_heatmap(pred, coord, weight, beta=1.0, delta=1.0, coef=1.0, want_grad=False):
    """The coordinate loss on the soft-arg-max of ``pred`` (B, K, H, W) against ``coord`` (B, K, 2) = (x, y) in heat-map pixels
    (mi355_coord_heatmap).  Returns (loss_rows [B,K], unit_grad [B,K,H,W] or None, uv [B,K,2]); ``coef`` is the term's
    coefficient: unit_grad = d(coef * mean over B*K of the rows)/d pred."""
    pred = _hm(pred)
    B, K, H, W = pred.shape
    if tuple(coord.shape) != (B, K, 2):
        raise Mi355Error('coord_heatmap: pred %s needs coordinates (%d, %d, 2), got %s' % (tuple(pred.shape), B, K, tuple(coord.shape)))
    coord = _hm(coord)
    if weight is not None:
        if weight.numel() != B * K:
            raise Mi355Error('coord_heatmap: %d weights for %d maps' % (weight.numel(), B * K))
        weight = _hm(weight.reshape(B, K))
    rows = torch.empty((B, K), dtype=torch.float32, device=pred.device)
    uv = torch.empty((B, K, 2), dtype=torch.float32, device=pred.device)
    g = torch.empty_like(pred) if want_grad else None
    call('mi355_coord_heatmap', ptr(pred), ptr(coord), ptr(weight), float(beta), float(delta), float(coef) / (B * K), ptr(rows),
         ptr(g), ptr(uv), B * K, H, W, stream_ptr())
    return rows, g, uv


def softargmax_backward(pred, g_uv, beta=1.0):
    """d loss / d ``pred`` (B, K, H, W) of a loss on the soft-arg-max of ``softmax(beta * pred)``, from ``g_uv`` (B, K, 2) =
    d loss / d (u, v) (mi355_softargmax_backward).  A joint whose two components are exactly 0 gets a map of zeros unread."""
    pred = _hm(pred)
    B, K, H, W = pred.shape
    if tuple(g_uv.shape) != (B, K, 2):
        raise Mi355Error('softargmax_backward: pred %s needs a gradient (%d, %d, 2), got %s' % (tuple(pred.shape), B, K, tuple(g_uv.shape)))
    g_uv = _hm(g_uv)
    g = torch.empty_like(pred)
    call('mi355_softargmax_backward', ptr(pred), ptr(g_uv), float(beta), ptr(g), B * K, H, W, stream_ptr())
    return g


def _bone_args(who, uv, weight, bones, mean, var, seen):
    uv = _hm(uv)
    if uv.dim() != 3 or uv.shape[2] != 2:
        raise Mi355Error('%s: the points must be (B, K, 2), got %s' % (who, tuple(uv.shape)))
    B, K, _ = uv.shape
    if weight is not None:
        if weight.numel() != B * K:
            raise Mi355Error('%s: %d weights for %d joints' % (who, weight.numel(), B * K))
        weight = _hm(weight.reshape(B, K))
    if bones.dtype != torch.int32 or bones.dim() != 2 or bones.shape[1] != 2 or not bones.is_contiguous():
        raise Mi355Error('%s: the bone table must be a contiguous int32 (E, 2) tensor, got %s %s' % (who, bones.dtype, tuple(bones.shape)))
    E = bones.shape[0]
    for name, t, dt in (('mean', mean, torch.float32), ('var', var, torch.float32), ('seen', seen, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (E,) or not t.is_contiguous():
            raise Mi355Error('%s: %s must be a contiguous %s (%d,) tensor, got %s %s' % (who, name, dt, E, t.dtype, tuple(t.shape)))
        _chk_dev(t)
    _chk_dev(bones)
    return uv, weight, B, K, E


def bone_prior(uv, weight, bones, mean, var, seen, margin=1.0, eps=1e-4, coef=1.0, want_grad=True):
    """The bone-ratio prior of ``uv`` (B, K, 2) against the running statistics (mi355_bone_prior).  Returns (loss_rows [B], g_uv
    [B, K, 2] or None); ``coef`` is the term's coefficient: g_uv = d(coef * mean over B of the rows) / d uv."""
    uv, weight, B, K, E = _bone_args('bone_prior', uv, weight, bones, mean, var, seen)
    rows = torch.empty((B,), dtype=torch.float32, device=uv.device)
    g = torch.empty_like(uv) if want_grad else None
    call('mi355_bone_prior', ptr(uv), ptr(weight), ptr(bones), ptr(mean), ptr(var), ptr(seen), float(margin), float(eps),
         float(coef) / B, ptr(rows), ptr(g), B, K, E, stream_ptr())
    return rows, g


def bone_stats_update(kp, weight, bones, mean, var, seen, rho):
    """Blend the bone-ratio statistics of the batch ``kp`` (B, K, 2) into ``mean`` / ``var`` / ``seen``, in place
    (mi355_bone_stats_update)."""
    kp, weight, B, K, E = _bone_args('bone_stats_update', kp, weight, bones, mean, var, seen)
    call('mi355_bone_stats_update', ptr(kp), ptr(weight), ptr(bones), ptr(mean), ptr(var), ptr(seen), float(rho), B, K, E, stream_ptr())


def reduce_sum(v, scale=1.0):
    v = v.contiguous()
    out = torch.empty((), dtype=torch.float32, device=v.device)
    call('mi355_reduce_sum', ptr(v), ptr(out), v.numel(), float(scale), stream_ptr())
    return out


def scale_by_dev(t, g_dev):
    out = torch.empty_like(t)
    call('mi355_scale_by_dev', ptr(t), ptr(g_dev), ptr(out), t.numel(), stream_ptr())
    return out


def scale_feature(t, g_dev):
    """t * (*g_dev) for a dense fp32 / bf16 device tensor of any layout (same strides out)."""
    if not t.is_cuda:
        raise Mi355Error('mi355 ops need CUDA/HIP tensors; there is no CPU fallback')
    if not (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)):
        t = t.contiguous()
    per = 8 if t.dtype == torch.bfloat16 else 4
    if t.numel() % per:
        raise Mi355Error('scale_feature needs a multiple of %d elements, got %d' % (per, t.numel()))
    out = torch.empty_like(t)
    call('mi355_scale_feature', ptr(t), ptr(g_dev), ptr(out), t.numel(), dtype_code(t.dtype), stream_ptr())
    return out


def pseudo_label(xy, patch, radius, div, S, kind, extra=None, normalise=False, want_gt=True, want_gf=True):
    B, K, _ = xy.shape
    dev = xy.device
    gt = torch.empty((B, K, S, S), dtype=torch.float32, device=dev) if want_gt else None
    gf = torch.empty((B, K, S, S), dtype=torch.float32, device=dev) if want_gf else None
    if extra is not None:
        extra = _hm(extra)
        if tuple(extra.shape) != (B, K, S, S):
            raise Mi355Error('pseudo_label: extra has shape %s, expected %s' % (tuple(extra.shape), (B, K, S, S)))
    call('mi355_pseudo_label', ptr(xy), ptr(patch), int(radius), int(div), int(S), int(kind), ptr(extra),
         int(normalise), ptr(gt), ptr(gf), B, K, stream_ptr())
    return gt, gf


def bilinear_up(x, size, alpha=1.0, out=None):
    """alpha * nn.Upsample(size, mode='bilinear')(x) (+ out when given)."""
    x = _hm(x)
    B, K, h, w = x.shape
    acc = out is not None
    _chk_room('bilinear_up out', out, B * K * size * size)
    if out is None:
        out = torch.empty((B, K, size, size), dtype=torch.float32, device=x.device)
    call('mi355_bilinear_up', ptr(x), ptr(out), B * K, h, w, size, size, float(alpha), int(acc), stream_ptr())
    return out


def pck_dists(pred_xy, tgt_xy, norm_x, norm_y):
    rows = pred_xy.shape[0] * pred_xy.shape[1]
    d = torch.empty(pred_xy.shape[:2], dtype=torch.float32, device=pred_xy.device)
    call('mi355_pck_dists', ptr(pred_xy.contiguous()), ptr(tgt_xy.contiguous()), ptr(d), rows, float(norm_x),
         float(norm_y), stream_ptr())
    return d


# ---------------------------------------------------------------- evaluation at image resolution
def _size2(size):
    H, W = (size, size) if isinstance(size, int) else size
    return int(H), int(W)


def upsample_argmax(hm, size, out=None):
    """Arg-max of nn.Upsample(size, mode='bilinear')(hm) without the up-sampled maps: (idx int32 [B,K], xy fp32 [B,K,2],
    maxval fp32 [B,K,1]), argmax2d's rules on the size[0] x size[1] grid.  `out`: an (idx, xy, maxval) triple to write into."""
    hm = _hm(hm)
    if hm.dim() != 4:
        raise Mi355Error('upsample_argmax: heat-maps must be (B, K, h, w), got %s' % (tuple(hm.shape),))
    B, K, h, w = hm.shape
    H, W = _size2(size)
    if min(B * K, h, w, H, W) < 1 or H * W >= 2 ** 31 - 1:
        raise Mi355Error('upsample_argmax: %s -> %d x %d' % (tuple(hm.shape), H, W))
    if out is None:
        out = (torch.empty((B, K), dtype=torch.int32, device=hm.device), torch.empty((B, K, 2), dtype=torch.float32, device=hm.device),
               torch.empty((B, K, 1), dtype=torch.float32, device=hm.device))
    idx, xy, mv = out
    _chk_dev(idx, xy, mv)
    for what, t, need, dt in (('idx', idx, B * K, torch.int32), ('xy', xy, 2 * B * K, torch.float32), ('maxval', mv, B * K, torch.float32)):
        _chk_room('upsample_argmax ' + what, t, need)
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise Mi355Error('upsample_argmax %s: needs a contiguous %s tensor' % (what, dt))
    call('mi355_upsample_argmax', ptr(hm), ptr(idx), ptr(xy), ptr(mv), B * K, h, w, H, W, stream_ptr())
    return idx, xy, mv


def mirror_batch(x):
    """(2B,C,H,W): the batch x (B,C,H,W) fp32 followed by its images mirrored along W -- the input of one flip-test forward."""
    if x.dim() != 4:
        raise Mi355Error('mirror_batch: the input must be (B, C, H, W), got %s' % (tuple(x.shape),))
    x = _hm(x)
    B, C, H, W = x.shape
    if min(B, C, H, W) < 1:
        raise Mi355Error('mirror_batch: empty input %s' % (tuple(x.shape),))
    out = torch.empty((2 * B, C, H, W), dtype=torch.float32, device=x.device)
    call('mi355_mirror_batch', ptr(x), ptr(out), B, C, H, W, stream_ptr())
    return out


DECODE_MODES = {'argmax': 0, 'quarter': 1, 'taylor': 2}
_TAPS = {}


def gaussian_taps(sigma):
    """(fp32 numpy taps [2 r + 1], r) of the smoothing in front of the taylor decode: r = ceil(2.5 sigma),
    exp(-i^2 / (2 sigma^2)) in float64, normalised to sum 1, rounded to fp32 (11 taps at sigma 2: DARK's kernel)."""
    import math
    import numpy as np
    sigma = float(sigma)
    if not (sigma > 0 and math.isfinite(sigma)):
        raise Mi355Error('flip_decode: sigma must be a positive number, got %r' % (sigma,))
    r = int(math.ceil(2.5 * sigma))
    if not 1 <= r <= 16:
        raise Mi355Error('flip_decode: sigma %g gives a smoothing radius of %d, outside 1..16' % (sigma, r))
    i = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32), r


def _taps_on(sigma, device):
    key = (float(sigma), torch.device(device))
    ent = _TAPS.get(key)
    if ent is None:
        g, r = gaussian_taps(sigma)
        ent = _TAPS[key] = (torch.from_numpy(g).to(device), r)
    return ent


def flip_decode(hm, hm_flip=None, shift=1, mode='argmax', sigma=2.0, scale=(1., 1.), want_avg=False):
    """Flip-test average and key-point decode in one launch: (idx int32 [B,K], xy fp32 [B,K,2], maxval fp32 [B,K,1], avg or
    None).  The working map is hm, or 0.5 * (hm + hm_flip mirrored back) where hm_flip holds the heat-maps of the mirrored
    images (`shift` = 1 moves them one column to the right first, Simple Baselines' SHIFT_HEATMAP); `want_avg` returns it.
    mode 'argmax' | 'quarter' (a quarter pixel towards the higher neighbour) | 'taylor' (DARK's second-order step on the log of
    the map smoothed by a Gaussian of `sigma`); xy = (x * scale[0], y * scale[1]) in heat-map pixels times the scales, zero where
    the maximum is not positive."""
    hm = _hm(hm)
    if hm.dim() != 4:
        raise Mi355Error('flip_decode: heat-maps must be (B, K, h, w), got %s' % (tuple(hm.shape),))
    B, K, h, w = hm.shape
    if min(B * K, h, w) < 1 or h * w > 2 ** 31 - 1:
        raise Mi355Error('flip_decode: %s' % (tuple(hm.shape),))
    if mode not in DECODE_MODES:
        raise Mi355Error("flip_decode: mode must be one of %s, got %r" % (sorted(DECODE_MODES), mode))
    if shift not in (0, 1):
        raise Mi355Error('flip_decode: shift must be 0 or 1, got %r' % (shift,))
    if hm_flip is not None:
        hm_flip = _hm(hm_flip)
        if tuple(hm_flip.shape) != tuple(hm.shape) or hm_flip.device != hm.device:
            raise Mi355Error('flip_decode: hm %s on %s vs hm_flip %s on %s' % (tuple(hm.shape), hm.device, tuple(hm_flip.shape), hm_flip.device))
    taps, radius = _taps_on(sigma, hm.device) if mode == 'taylor' else (None, 0)
    idx = torch.empty((B, K), dtype=torch.int32, device=hm.device)
    xy = torch.empty((B, K, 2), dtype=torch.float32, device=hm.device)
    mv = torch.empty((B, K, 1), dtype=torch.float32, device=hm.device)
    avg = torch.empty_like(hm) if want_avg else None
    call('mi355_flip_decode', ptr(hm), ptr(hm_flip), int(shift), ptr(avg), DECODE_MODES[mode], ptr(taps), radius, float(scale[0]),
         float(scale[1]), ptr(idx), ptr(xy), ptr(mv), B * K, h, w, stream_ptr())
    return idx, xy, mv, avg


def pose_metrics_state(K, T, device):
    """Zeroed accumulators of pose_metrics: (sum_err float64 [K], count int32 [K], hits int32 [K,T])."""
    return (torch.zeros(K, dtype=torch.float64, device=device), torch.zeros(K, dtype=torch.int32, device=device),
            torch.zeros((K, T), dtype=torch.int32, device=device))


def pose_metrics(pred, gt, vis, thr, state):
    """Add one batch to `state` = (sum_err [K] float64, count [K] int32, hits [K,T] int32): per visible joint the float64
    end-point error of pred against gt (B,K,2) and a hit per threshold of `thr` (T,) it stays strictly below."""
    if pred.dim() != 3 or pred.shape[2] != 2 or tuple(gt.shape) != tuple(pred.shape):
        raise Mi355Error('pose_metrics: pred %s vs gt %s, both must be (B, K, 2)' % (tuple(pred.shape), tuple(gt.shape)))
    B, K, _ = pred.shape
    if vis.numel() != B * K:
        raise Mi355Error('pose_metrics: vis has %d elements for %d x %d joints' % (vis.numel(), B, K))
    f = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
    pred, gt, vis, thr = f(pred), f(gt), f(vis), f(thr)
    sum_err, count, hits = state
    _chk_dev(pred, gt, vis, thr, sum_err, count, hits)
    T = thr.numel()
    if B < 1 or K < 1 or T < 1:
        raise Mi355Error('pose_metrics: B=%d K=%d T=%d' % (B, K, T))
    for what, t, need, dt in (('sum_err', sum_err, K, torch.float64), ('count', count, K, torch.int32), ('hits', hits, K * T, torch.int32)):
        _chk_room('pose_metrics ' + what, t, need)
        if t.dtype != dt or not t.is_contiguous():
            raise Mi355Error('pose_metrics %s: needs a contiguous %s tensor' % (what, dt))
    call('mi355_pose_metrics', ptr(pred), ptr(gt), ptr(vis), ptr(thr), T, B, K, ptr(sum_err), ptr(count), ptr(hits), stream_ptr())


# ---------------------------------------------------------------- optimiser
def sgd_nesterov(p, g, buf, lr_dev, momentum, wd, nesterov, p_lowp=None):
    _chk_dev(p, g, buf, lr_dev, p_lowp)
    for what, t in (('g', g), ('buf', buf), ('p_lowp', p_lowp)):
        _chk_room('sgd_nesterov ' + what, t, p.numel())
    call('mi355_sgd_nesterov', ptr(p), ptr(g), ptr(buf), p.numel(), ptr(lr_dev), float(momentum), float(wd),
         int(nesterov), ptr(p_lowp), stream_ptr())


def cast_f32(src, dst):
    _chk_dev(src, dst)
    _chk_room('cast_f32 dst', dst, src.numel())
    call('mi355_cast_f32', ptr(src), ptr(dst), src.numel(), dtype_code(dst.dtype), stream_ptr())


EMA_CHUNK, EMA_F32, EMA_COPY64 = 2048, 0, 1        # MI355_EMA_CHUNK and the record kinds of mi355_ema_item
EMA_ITEM_BYTES = 32


def ema_update(e, p, coef_dev):
    """e = e * k + c * p over the flat fp32 range e (k, c = coef_dev[0], coef_dev[1]); p is only read."""
    _chk_dev(e, p, coef_dev)
    _chk_room('ema_update p', p, e.numel())
    _chk_room('ema_update coef_dev', coef_dev, 2)
    call('mi355_ema_update', ptr(e), ptr(p), e.numel(), ptr(coef_dev), stream_ptr())


def ema_table(records, device):
    """records: (src tensor, dst tensor, kind) -> (uint8 device tensor of mi355_ema_item records, their number, total blocks).
    Each pair must share one dense memory layout: the kernel walks the two storages element by element."""
    import numpy as np
    rec = np.zeros(len(records), dtype=[('src', '<u8'), ('dst', '<u8'), ('n', '<i8'), ('kind', '<i4'), ('blk0', '<i4')])
    blk = 0
    for i, (src, dst, kind) in enumerate(records):
        _chk_dev(src, dst)
        want = torch.int64 if kind == EMA_COPY64 else torch.float32
        n = dst.numel()
        if src.dtype != want or dst.dtype != want or src.shape != dst.shape or src.stride() != dst.stride() or n < 1 or \
                1 + sum((s - 1) * st for s, st in zip(dst.shape, dst.stride())) != n:
            raise Mi355Error('ema_table: record %d needs two dense %s tensors of one layout' % (i, want))
        rec[i] = (src.data_ptr(), dst.data_ptr(), n, kind, blk)
        blk += (n + EMA_CHUNK - 1) // EMA_CHUNK
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device), len(records), blk


def ema_update_batched(table, count, total_blocks, coef_dev):
    """table: uint8 device tensor holding `count` mi355_ema_item records (ema_table)."""
    _chk_dev(table, coef_dev)
    _chk_room('ema_update_batched table', table, count * EMA_ITEM_BYTES)
    _chk_room('ema_update_batched coef_dev', coef_dev, 2)
    call('mi355_ema_update_batched', ptr(table), int(count), int(total_blocks), ptr(coef_dev), stream_ptr())


GN_CHUNK = 16384                                    # MI355_GN_CHUNK
GN_ITEM_BYTES, CLIP_REC_BYTES = 24, 32


def clip_rec_dtype():
    """numpy layout of mi355_clip_rec."""
    import numpy as np
    return np.dtype([('sumsq', '<f8'), ('max_norm', '<f4'), ('norm', '<f4'), ('coef', '<f4'), ('skip', '<i4'), ('n_skipped', '<i8')])


def clip_records(count, max_norm, device):
    """`count` zeroed mi355_clip_rec records with their max_norm field set, as one uint8 device tensor; record i is the view
    [i * CLIP_REC_BYTES : (i + 1) * CLIP_REC_BYTES]."""
    import numpy as np
    rec = np.zeros(count, dtype=clip_rec_dtype())
    assert rec.dtype.itemsize == CLIP_REC_BYTES
    rec['max_norm'] = np.float32(max_norm)
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device)


def gn_table(ranges, device):
    """ranges: 1-D dense fp32 device tensors (views of the gradient buffers), 16-byte aligned -> (uint8 device tensor of
    mi355_gn_item records, their number, total blocks): the arguments of grad_sumsq_batched.  The table holds addresses only:
    the caller keeps the buffers alive."""
    import numpy as np
    rec = np.zeros(len(ranges), dtype=[('g', '<u8'), ('n', '<i8'), ('blk0', '<i4'), ('pad', '<i4')])
    assert rec.dtype.itemsize == GN_ITEM_BYTES
    if not len(ranges):
        raise Mi355Error('gn_table: no ranges')
    blk = 0
    for i, g in enumerate(ranges):
        _chk_dev(g)
        n = g.numel()
        if g.dtype != torch.float32 or g.dim() != 1 or n < 1 or g.stride(0) != 1 or g.data_ptr() % 16:
            raise Mi355Error('gn_table: range %d needs a dense 1-D fp32 tensor of at least one element on a 16-byte boundary' % i)
        rec[i] = (g.data_ptr(), n, blk, 0)
        blk += (n + GN_CHUNK - 1) // GN_CHUNK
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device), len(ranges), blk


def _chk_clip_rec(what, rec):
    _chk_room(what + ' rec', rec, CLIP_REC_BYTES)
    if rec.dtype != torch.uint8 or not rec.is_contiguous():
        raise Mi355Error('%s rec: needs a contiguous uint8 tensor holding one mi355_clip_rec' % what)


def grad_sumsq_batched(table, count, total_blocks, partials):
    """partials[b] = fp64 sum of squares of block b's slice of the ranges in `table` (gn_table); partials: float64, one per block."""
    _chk_dev(table, partials)
    _chk_room('grad_sumsq_batched table', table, count * GN_ITEM_BYTES)
    _chk_room('grad_sumsq_batched partials', partials, total_blocks)
    if partials.dtype != torch.float64 or not partials.is_contiguous():
        raise Mi355Error('grad_sumsq_batched partials: needs a contiguous float64 tensor')
    call('mi355_grad_sumsq_batched', ptr(table), int(count), int(total_blocks), ptr(partials), stream_ptr())


def grad_clip_coef(partials, total_blocks, rec):
    """Fold partials[0 .. total_blocks) into the mi355_clip_rec `rec` (uint8 view): sumsq, norm, coef, skip, n_skipped."""
    _chk_dev(partials, rec)
    _chk_room('grad_clip_coef partials', partials, total_blocks)
    if partials.dtype != torch.float64 or not partials.is_contiguous():
        raise Mi355Error('grad_clip_coef partials: needs a contiguous float64 tensor')
    _chk_clip_rec('grad_clip_coef', rec)
    call('mi355_grad_clip_coef', ptr(partials), int(total_blocks), ptr(rec), stream_ptr())


def sgd_nesterov_clipped(p, g, buf, lr_dev, rec, momentum, wd, nesterov, p_lowp=None):
    """sgd_nesterov on fl32(g * rec.coef); writes nothing when rec.skip is set.  g is only read."""
    _chk_dev(p, g, buf, lr_dev, rec, p_lowp)
    for what, t in (('g', g), ('buf', buf), ('p_lowp', p_lowp)):
        _chk_room('sgd_nesterov_clipped ' + what, t, p.numel())
    _chk_clip_rec('sgd_nesterov_clipped', rec)
    call('mi355_sgd_nesterov_clipped', ptr(p), ptr(g), ptr(buf), p.numel(), ptr(lr_dev), ptr(rec), float(momentum), float(wd),
         int(nesterov), ptr(p_lowp), stream_ptr())


ADAM_CHUNK = 16384                                  # MI355_ADAM_CHUNK
ADAM_ITEM_BYTES = 88


def adam_item_dtype():
    """numpy layout of mi355_adam_item."""
    import numpy as np
    return np.dtype([(k, '<u8') for k in ('p', 'g', 'm', 'v', 'step', 'lr')] + [('n', '<i8')] +
                    [('beta1', '<f8'), ('beta2', '<f8'), ('eps', '<f4'), ('wd', '<f4'), ('decoupled', '<i4'), ('blk0', '<i4')])


def adam_table(items, device):
    """items: (p, g, m, v, step, lr, beta1, beta2, eps, wd, decoupled) per parameter about to be stepped -- p, g, m, v dense fp32
    device tensors of one size on 16-byte boundaries, step and lr one fp32 each on the device -> (uint8 device tensor of
    mi355_adam_item records, their number, total blocks): the arguments of adam_step_batched / adam_tick_batched.  The table
    holds addresses only: the caller keeps the tensors alive."""
    import numpy as np
    rec = np.zeros(len(items), dtype=adam_item_dtype())
    assert rec.dtype.itemsize == ADAM_ITEM_BYTES
    if not len(items):
        raise Mi355Error('adam_table: no items')
    blk = 0
    for i, (p, g, m, v, step, lr, beta1, beta2, eps, wd, decoupled) in enumerate(items):
        _chk_dev(p, g, m, v, step, lr)
        n = p.numel()
        for what, t in (('p', p), ('g', g), ('m', m), ('v', v)):
            if t.dtype != torch.float32 or t.numel() != n or n < 1 or t.data_ptr() % 16 or \
                    1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) != n:
                raise Mi355Error('adam_table: item %d %s needs a dense fp32 tensor of %d element(s) on a 16-byte boundary' % (i, what, n))
        for what, t in (('step', step), ('lr', lr)):
            if t.dtype != torch.float32 or t.numel() != 1:
                raise Mi355Error('adam_table: item %d %s needs one fp32 value on the device' % (i, what))
        rec[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), lr.data_ptr(), n,
                  beta1, beta2, eps, wd, int(bool(decoupled)), blk)
        blk += (n + ADAM_CHUNK - 1) // ADAM_CHUNK
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device), len(items), blk


def adam_step_batched(table, count, total_blocks, rec=None):
    """One Adam / AdamW step of every item in `table` (adam_table) on fl32(g * rec.coef), or on g when rec is None; writes nothing
    when rec.skip is set.  The step counts are only read: adam_tick_batched advances them."""
    _chk_dev(table, rec)
    _chk_room('adam_step_batched table', table, count * ADAM_ITEM_BYTES)
    if rec is not None:
        _chk_clip_rec('adam_step_batched', rec)
    call('mi355_adam_step_batched', ptr(table), int(count), int(total_blocks), ptr(rec), stream_ptr())


def adam_tick_batched(table, count, rec=None):
    """*step += 1 for every item in `table` unless rec.skip is set: the launch behind adam_step_batched."""
    _chk_dev(table, rec)
    _chk_room('adam_tick_batched table', table, count * ADAM_ITEM_BYTES)
    if rec is not None:
        _chk_clip_rec('adam_tick_batched', rec)
    call('mi355_adam_tick_batched', ptr(table), int(count), ptr(rec), stream_ptr())


# ---------------------------------------------------------------- mean-teacher consistency (csrc/teacher.hip)
FOLD_CHUNK = 2048                                   # MI355_FOLD_CHUNK
FOLD_ITEM_BYTES = 88


def _fold_dtype():
    import numpy as np
    return np.dtype([(n, '<u8') for n in ('w', 'gamma', 'beta', 'mean', 'var', 'conv_bias', 'out_w', 'out_bias')] +
                    [('eps', '<f4'), ('O', '<i4'), ('T', '<i4'), ('I', '<i4'), ('axis', '<i4'), ('blk0', '<i4')])


def fold_table(records, device):
    """records: (w, gamma, beta, mean, var, conv_bias or None, out_w, out_bias, eps, O, T, I, axis) with fp32 device tensors ->
    (host record array, uint8 device copy of it, number of records, total blocks): the arguments of bn_fold_batched.  w and
    out_w are dense in memory order [O][T][I] (any view whose storage walks that order)."""
    import numpy as np
    rec = np.zeros(len(records), dtype=_fold_dtype())
    assert rec.dtype.itemsize == FOLD_ITEM_BYTES
    blk = 0
    for i, (w, gamma, beta, mean, var, cbias, out_w, out_bias, eps, O, T, I, axis) in enumerate(records):
        ts = (w, gamma, beta, mean, var, cbias, out_w, out_bias)
        _chk_dev(*ts)
        if any(t is not None and t.dtype != torch.float32 for t in ts):
            raise Mi355Error('fold_table: record %d needs fp32 tensors' % i)
        if axis not in (0, 1) or min(O, T, I) < 1:
            raise Mi355Error('fold_table: record %d: O=%r T=%r I=%r axis=%r' % (i, O, T, I, axis))
        n, C = O * T * I, (O if axis == 0 else I)
        _chk_room('fold_table w', w, n)
        _chk_room('fold_table out_w', out_w, n)
        for what, t in (('gamma', gamma), ('beta', beta), ('mean', mean), ('var', var), ('conv_bias', cbias), ('out_bias', out_bias)):
            _chk_room('fold_table ' + what, t, C)
        rec[i] = tuple(ptr(t) for t in ts) + (float(eps), O, T, I, axis, blk)
        blk += (n + FOLD_CHUNK - 1) // FOLD_CHUNK
    return rec, torch.from_numpy(rec.view(np.uint8).copy()).to(device), len(records), blk


def bn_fold_batched(rec_host, table, count, total_blocks):
    """One launch: fold every record's eval-mode BatchNorm into out_w / out_bias (fold_table).  Capturable; allocates nothing."""
    _chk_dev(table)
    _chk_room('bn_fold_batched table', table, count * FOLD_ITEM_BYTES)
    if rec_host.dtype.itemsize != FOLD_ITEM_BYTES or rec_host.size < count or not rec_host.flags['C_CONTIGUOUS']:
        raise Mi355Error('bn_fold_batched: the host table does not hold %d records' % count)
    call('mi355_bn_fold_batched', rec_host.ctypes.data, ptr(table), int(count), int(total_blocks), stream_ptr())


def mse_record(joint_mask, grad_scale, device=None, out=None):
    """The device record {int32 joint_mask, float grad_scale} of mse_heatmap as a 2-element int32 tensor (new, or `out` rewritten)."""
    import numpy as np
    host = np.zeros(1, dtype=[('mask', '<u4'), ('gs', '<f4')])
    host[0] = (int(joint_mask) & 0xffffffff, np.float32(grad_scale))
    t = torch.from_numpy(host.view(np.int32).copy())
    if out is None:
        return t.to(device)
    _chk_room('mse_record out', out, 2)
    out.copy_(t)
    return out


def mse_heatmap(pred, target, rec, want_grad, rows=None, grad=None):
    """Returns (rows [B,K] = per-map sums of squared differences, unit_grad [B,K,H,W] or None); maps whose joint is outside the
    record's mask give exact zeros.  rec: mse_record()."""
    pred, target = _hm(pred), _hm(target)
    B, K, H, W = pred.shape
    if tuple(target.shape) != (B, K, H, W):
        raise Mi355Error('mse_heatmap: pred %s vs target %s' % (tuple(pred.shape), tuple(target.shape)))
    _chk_dev(rec)
    if rec.dtype != torch.int32:
        raise Mi355Error('mse_heatmap: rec must be the int32 pair of mse_record')
    _chk_room('mse_heatmap rec', rec, 2)
    if rows is None:
        rows = torch.empty((B, K), dtype=torch.float32, device=pred.device)
    if want_grad and grad is None:
        grad = torch.empty_like(pred)
    _chk_room('mse_heatmap rows', rows, B * K)
    _chk_room('mse_heatmap unit_grad', grad, B * K * H * W)
    call('mi355_mse_heatmap', ptr(pred), ptr(target), ptr(rec), ptr(rows), ptr(grad) if want_grad else 0, B, K, H * W, stream_ptr())
    return rows, (grad if want_grad else None)


# ---------------------------------------------------------------- cross-domain mixup (csrc/mixup.hip)
def _dense_f32(who, what, t):
    """`t` must be an fp32 device tensor whose elements lie in memory in index order without gaps (its first byte may sit
    anywhere: the kernel takes scalar accesses when a base is not 16-byte aligned)."""
    _chk_dev(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise Mi355Error('%s: %s must be a dense fp32 tensor, got %s %s strides %s' % (who, what, t.dtype, tuple(t.shape), t.stride()))


def mixup_pairs(x_s, hm_s, w_s, x_t, hm_t, w_t, lam, out=None):
    """The two blends of uda/model/loss.py:13-24 in one launch.  x_s, x_t (B, C, S, S); hm_s, hm_t (B, K, H, W); w_s, w_t (B, K) or
    (B, K, 1); lam: B fp32 values on the device, already max(mix, 1 - mix).  Returns (x_mix (2B, C, S, S), hm_mix (2B, K, H, W),
    w_mix (2B,) + w_s.shape[1:]): rows [0, B) are a_s * lam + a_t * (1 - lam), rows [B, 2B) a_t * lam + a_s * (1 - lam), w_mix is
    max(w_s, w_t) twice.  `out`: that triple, to be written in place (a training step keeps it at fixed addresses)."""
    who = 'mixup_pairs'
    for what, t in (('x_s', x_s), ('x_t', x_t), ('hm_s', hm_s), ('hm_t', hm_t), ('w_s', w_s), ('w_t', w_t), ('lam', lam)):
        _dense_f32(who, what, t)
    if x_s.dim() != 4 or hm_s.dim() != 4 or w_s.dim() not in (2, 3):
        raise Mi355Error('%s: needs (B, C, S, S) images, (B, K, H, W) heat-maps and (B, K) weights, got %s, %s, %s'
                         % (who, tuple(x_s.shape), tuple(hm_s.shape), tuple(w_s.shape)))
    for what, a, b in (('x', x_s, x_t), ('hm', hm_s, hm_t), ('w', w_s, w_t)):
        if tuple(a.shape) != tuple(b.shape):
            raise Mi355Error('%s: %s_s %s vs %s_t %s' % (who, what, tuple(a.shape), what, tuple(b.shape)))
    B, K = x_s.shape[0], hm_s.shape[1]
    if hm_s.shape[0] != B or w_s.shape[0] != B or w_s.numel() != B * K or lam.numel() != B:
        raise Mi355Error('%s: %d images, heat-maps %s, weights %s, %d coefficients' % (who, B, tuple(hm_s.shape), tuple(w_s.shape), lam.numel()))
    if B < 1 or x_s[0].numel() < 1 or hm_s[0].numel() < 1:
        raise Mi355Error('%s: empty operand (images %s, heat-maps %s)' % (who, tuple(x_s.shape), tuple(hm_s.shape)))
    shapes = ((2 * B,) + tuple(x_s.shape[1:]), (2 * B,) + tuple(hm_s.shape[1:]), (2 * B,) + tuple(w_s.shape[1:]))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=x_s.device) for s in shapes)
    x_mix, hm_mix, w_mix = out
    for what, t, s in (('x_mix', x_mix, shapes[0]), ('hm_mix', hm_mix, shapes[1]), ('w_mix', w_mix, shapes[2])):
        _dense_f32(who, what, t)
        if tuple(t.shape) != s:                      # (dense and of this shape: room for everything the launch writes)
            raise Mi355Error('%s: %s has shape %s, the launch writes %s' % (who, what, tuple(t.shape), s))
    if len({t.device for t in (x_s, x_t, hm_s, hm_t, w_s, w_t, lam, x_mix, hm_mix, w_mix)}) != 1:
        raise Mi355Error('%s: the operands live on different devices' % who)
    call('mi355_mixup_pairs', ptr(x_s), ptr(x_t), ptr(hm_s), ptr(hm_t), ptr(w_s), ptr(w_t), ptr(lam), ptr(x_mix), ptr(hm_mix),
         ptr(w_mix), int(B), x_s[0].numel(), hm_s[0].numel(), int(K), stream_ptr())
    return x_mix, hm_mix, w_mix


# ---------------------------------------------------------------- Fourier-domain stylisation (csrc/fda.hip)
from .augment import MEAN, STD          # noqa: E402  (the normalisation the loaders apply)

FDA_MAX_B = 32


def fda_band(H, W, beta):
    """b of the (2b+1)^2 window: int(floor(min(H, W) * beta)) in Python doubles, as the published low_freq_mutate takes it."""
    return int(math.floor(min(int(H), int(W)) * float(beta)))


def fda_transfer(x_s, x_t, beta, mean=MEAN, std=STD, out=None, ws=None):
    """Fourier Domain Adaptation (Yang and Soatto, CVPR 2020) of a source batch: the amplitude of the (2b+1)^2 lowest frequencies
    of every plane of x_s replaced by that of the same plane of x_t, the phase kept (mi355_fda_transfer, include/mi355pose.h).
    x_s, x_t: (B, C, H, W) dense fp32, normalised with `mean` / `std` (default: those of mi355.augment); b = fda_band(H, W, beta).
    Returns `out`; `out` and the workspace `ws` (a uint8 tensor) are allocated only when not given, and never during graph capture."""
    who = 'fda_transfer'
    for what, t in (('x_s', x_s), ('x_t', x_t)):
        _dense_f32(who, what, t)
    if x_s.dim() != 4 or tuple(x_s.shape) != tuple(x_t.shape):
        raise Mi355Error('%s: x_s %s and x_t %s must be (B, C, H, W) of one shape' % (who, tuple(x_s.shape), tuple(x_t.shape)))
    if x_s.device != x_t.device:
        raise Mi355Error('%s: x_s and x_t live on different devices' % who)
    B, C, H, W = (int(s) for s in x_s.shape)
    if not (isinstance(beta, (int, float)) and math.isfinite(beta) and beta >= 0):
        raise Mi355Error('%s: beta=%r must be a finite number >= 0' % (who, beta))
    if len(mean) < C or len(std) < C:
        raise Mi355Error('%s: mean / std hold %d / %d values for C=%d channels' % (who, len(mean), len(std), C))
    b = fda_band(H, W, beta)
    need = load().mi355_fda_workspace_bytes(B, C, H, W, b)
    if need < 0:
        raise Mi355Error('%s: beta=%r gives b=%d: %s' % (who, beta, b, load().mi355_last_error().decode()))
    if out is None or ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('%s: out / the workspace would be allocated during graph capture; run one eager call first' % who)
        if out is None:
            out = torch.empty((B, C, H, W), dtype=torch.float32, device=x_s.device)
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=x_s.device)
    _dense_f32(who, 'out', out)
    if tuple(out.shape) != (B, C, H, W):
        raise Mi355Error('%s: out has shape %s, the launch writes %s' % (who, tuple(out.shape), (B, C, H, W)))
    _chk_dev(ws)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or out.device != x_s.device or ws.device != x_s.device:
        raise Mi355Error('%s: ws must be a dense uint8 tensor on the device of x_s (and out on it too)' % who)
    fl = ctypes.c_float * C
    call('mi355_fda_transfer', ptr(x_s), ptr(x_t), ptr(out), fl(*[float(v) for v in mean[:C]]), fl(*[float(v) for v in std[:C]]),
         B, C, H, W, b, ptr(ws), ws.numel(), stream_ptr())
    return out


# ---------------------------------------------------------------- geometric teacher view (csrc/warp.hip)
VIEW_REC_FLOATS = 18          # mi355_view_rec: img, hm, hm_inv, each a row-major 2 x 3 fp32 matrix
WARP_MAX_SIDE = 4096


def _size_hw(size):
    if isinstance(size, int):
        return size, size
    h, w = size
    return int(h), int(w)


def view_records(angle, scale, shift, image_size, heatmap_size):
    """The record table of a geometric view as a numpy (B, 18) fp32 array (include/mi355pose.h, mi355_view_rec).  angle: B angles
    in degrees; scale: B factors > 0; shift: (B, 2) translations (tx, ty) in image pixels; image_size, heatmap_size: (H, W) and
    (h, w), or one int for a square.  Sample b's view maps p to q = s R(a) (p - c) + c + t, c = ((W-1)/2, (H-1)/2); img = A^-1,
    hm = A in heat-map pixels, hm_inv = its inverse, each composed in float64 and rounded once.  The strides in x and y must be
    equal whole numbers; non-finite values and s <= 0 are refused."""
    import numpy as np
    who = 'view_records'
    H, W = _size_hw(image_size)
    h, w = _size_hw(heatmap_size)
    if min(H, W, h, w) < 1 or H * w != W * h or W % w != 0:
        raise Mi355Error('%s: the strides in x and y must be equal whole numbers (image %dx%d, heat-map %dx%d)' % (who, H, W, h, w))
    stride = W // w
    a = np.atleast_1d(np.asarray(angle, dtype=np.float64))
    s = np.atleast_1d(np.asarray(scale, dtype=np.float64))
    t = np.asarray(shift, dtype=np.float64).reshape(-1, 2)
    B = a.shape[0]
    if a.ndim != 1 or s.shape != (B,) or t.shape != (B, 2):
        raise Mi355Error('%s: %d angles, scales of shape %s, shifts of shape %s' % (who, B, s.shape, t.shape))
    if not (np.isfinite(a).all() and np.isfinite(s).all() and np.isfinite(t).all()):
        raise Mi355Error('%s: non-finite angle, scale or shift' % who)
    if not (s > 0).all():
        raise Mi355Error('%s: scales must be > 0, got %s' % (who, s.tolist()))
    out = np.empty((B, VIEW_REC_FLOATS), dtype=np.float32)
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    for b in range(B):
        r = np.deg2rad(a[b])
        L = s[b] * np.array([[np.cos(r), -np.sin(r)], [np.sin(r), np.cos(r)]])
        T = c + t[b] - L @ c
        Li = np.linalg.inv(L)
        mats = (np.concatenate([Li, (-Li @ T)[:, None]], axis=1), np.concatenate([L, (T / stride)[:, None]], axis=1),
                np.concatenate([Li, (-Li @ T / stride)[:, None]], axis=1))
        out[b] = np.concatenate([m.reshape(-1) for m in mats]).astype(np.float32)
    return out


def _chk_view_recs(who, recs, B, *others):
    _dense_f32(who, 'recs', recs)
    if recs.numel() != B * VIEW_REC_FLOATS:
        raise Mi355Error('%s: the record table holds %d floats, %d samples need %d' % (who, recs.numel(), B, B * VIEW_REC_FLOATS))
    if any(t.device != recs.device for t in others if t is not None):
        raise Mi355Error('%s: the operands live on different devices' % who)


def _chk_sides(who, H, W):
    if not (1 <= H <= WARP_MAX_SIDE and 1 <= W <= WARP_MAX_SIDE):
        raise Mi355Error('%s: a plane of %d x %d is outside 1..%d' % (who, H, W, WARP_MAX_SIDE))


def affine_warp_images(x, recs, out=None):
    """out[b, c] = x[b, c] resampled under the `img` matrix of recs[b] (bilinear, 0 outside; mi355_affine_warp_images).  x: dense
    fp32 (B, C, H, W); recs: a device tensor of B * 18 floats (view_records).  `out` is allocated only when not given, and never
    during graph capture."""
    who = 'affine_warp_images'
    _dense_f32(who, 'x', x)
    if x.dim() != 4 or x.numel() == 0:
        raise Mi355Error('%s: x must be a non-empty (B, C, H, W) batch, got %s' % (who, tuple(x.shape)))
    B, C, H, W = (int(s) for s in x.shape)
    _chk_sides(who, H, W)
    if out is None:
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('%s: out would be allocated during graph capture; run one eager call first' % who)
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    _dense_f32(who, 'out', out)
    if tuple(out.shape) != (B, C, H, W):
        raise Mi355Error('%s: out has shape %s, the launch writes %s' % (who, tuple(out.shape), (B, C, H, W)))
    _chk_view_recs(who, recs, B, x, out)
    call('mi355_affine_warp_images', ptr(x), ptr(recs), ptr(out), B, C, H, W, stream_ptr())
    return out


def affine_unwarp_heatmaps(y, recs, margin, w_in=None, out=None):
    """The teacher's heat-maps mapped back to the loader's frame: y_hat[b, k] = y[b, k] resampled under the `hm` matrix of recs[b]
    (mi355_affine_unwarp_heatmaps).  Returns (y_hat, valid, w_out): valid (B, K) is 1.0 where the arg-max of y[b, k] lies at
    least `margin` pixels inside the teacher's frame and its pre-image lies inside the map, else 0.0; w_out = w_in * valid with
    w_in's shape ((B, K) or (B, K, 1)), None without w_in.  `out`: the triple (y_hat, valid, w_out) -- w_out None without w_in --
    to be written in place; allocated only when not given, and never during graph capture."""
    who = 'affine_unwarp_heatmaps'
    _dense_f32(who, 'y', y)
    if y.dim() != 4 or y.numel() == 0:
        raise Mi355Error('%s: y must be a non-empty (B, K, h, w) batch of heat-maps, got %s' % (who, tuple(y.shape)))
    B, K, h, w = (int(s) for s in y.shape)
    _chk_sides(who, h, w)
    if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not math.isfinite(margin) or margin < 0:
        raise Mi355Error('%s: margin=%r must be a finite number >= 0' % (who, margin))
    if w_in is not None:
        _dense_f32(who, 'w_in', w_in)
        if w_in.numel() != B * K or w_in.shape[0] != B:
            raise Mi355Error('%s: w_in %s for %d x %d maps' % (who, tuple(w_in.shape), B, K))
    if out is None:
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('%s: the outputs would be allocated during graph capture; run one eager call first' % who)
        out = (torch.empty((B, K, h, w), dtype=torch.float32, device=y.device), torch.empty((B, K), dtype=torch.float32, device=y.device),
               None if w_in is None else torch.empty(tuple(w_in.shape), dtype=torch.float32, device=y.device))
    y_hat, valid, w_out = out
    if (w_in is None) != (w_out is None):
        raise Mi355Error('%s: w_in and w_out go together (both or neither)' % who)
    shapes = ((B, K, h, w), (B, K), None if w_in is None else tuple(w_in.shape))
    for what, t, s in (('y_hat', y_hat, shapes[0]), ('valid', valid, shapes[1]), ('w_out', w_out, shapes[2])):
        if t is None:
            continue
        _dense_f32(who, what, t)
        if tuple(t.shape) != s:
            raise Mi355Error('%s: %s has shape %s, the launch writes %s' % (who, what, tuple(t.shape), s))
    _chk_view_recs(who, recs, B, y, w_in, y_hat, valid, w_out)
    call('mi355_affine_unwarp_heatmaps', ptr(y), ptr(recs), float(margin), ptr(w_in), ptr(y_hat), ptr(valid), ptr(w_out), B, K, h, w,
         stream_ptr())
    return y_hat, valid, w_out


def mse_heatmap_w(pred, target, rec, wmap, want_grad, rows=None, grad=None):
    """mse_heatmap with a per-map weight: (rows [B,K] = w * the per-map sums of squared differences, unit_grad [B,K,H,W] * w or
    None).  wmap: B * K fp32 weights on the device; maps with w == 0 or outside the record's mask give exact zeros and are not
    read.  rec: mse_record().  rows / grad are allocated only when not given, and never during graph capture."""
    who = 'mse_heatmap_w'
    for what, t in (('pred', pred), ('target', target), ('wmap', wmap)):
        _dense_f32(who, what, t)
    if pred.dim() != 4 or pred.numel() == 0 or tuple(target.shape) != tuple(pred.shape):
        raise Mi355Error('%s: pred %s vs target %s ((B, K, H, W) of one shape)' % (who, tuple(pred.shape), tuple(target.shape)))
    B, K, H, W = (int(s) for s in pred.shape)
    if wmap.numel() != B * K:
        raise Mi355Error('%s: %d weights for %d x %d maps' % (who, wmap.numel(), B, K))
    _chk_dev(rec)
    if rec.dtype != torch.int32:
        raise Mi355Error('%s: rec must be the int32 pair of mse_record' % who)
    _chk_room('%s rec' % who, rec, 2)
    if rows is None or (want_grad and grad is None):
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('%s: rows / unit_grad would be allocated during graph capture; run one eager call first' % who)
        if rows is None:
            rows = torch.empty((B, K), dtype=torch.float32, device=pred.device)
        if want_grad and grad is None:
            grad = torch.empty_like(pred)
    _dense_f32(who, 'rows', rows)
    _chk_room('%s rows' % who, rows, B * K)
    if want_grad:
        _dense_f32(who, 'unit_grad', grad)
        _chk_room('%s unit_grad' % who, grad, B * K * H * W)
    if len({t.device for t in (pred, target, wmap, rec, rows) + ((grad,) if want_grad else ())}) != 1:
        raise Mi355Error('%s: the operands live on different devices' % who)
    call('mi355_mse_heatmap_w', ptr(pred), ptr(target), ptr(rec), ptr(wmap), ptr(rows), ptr(grad) if want_grad else 0, B, K, H * W,
         stream_ptr())
    return rows, (grad if want_grad else None)


# ---------------------------------------------------------------- adaptive occlusion, teacher confidence (csrc/occlude.hip)
OCC_MAX_BOXES, OCC_MAX_JOINTS = 8, 64


def _occ_out(who, out, specs, device):
    """The outputs of one launch: `out` as given, or fresh tensors -- never during graph capture.  specs: (name, shape, dtype) or
    None for an output the call does not have; each given tensor must be dense, of that shape and dtype, on `device`."""
    if out is None:
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('%s: the outputs would be allocated during graph capture; run one eager call first' % who)
        out = tuple(None if s is None else torch.empty(s[1], dtype=s[2], device=device) for s in specs)
    if len(out) != len(specs):
        raise Mi355Error('%s: out must hold %d tensors, got %d' % (who, len(specs), len(out)))
    for t, s in zip(out, specs):
        if (t is None) != (s is None):
            raise Mi355Error('%s: out has %s where the call %s' % (who, 'nothing' if t is None else 'a tensor',
                                                                    'writes ' + s[0] if s is not None else 'writes nothing'))
        if t is None:
            continue
        _chk_dev(t)
        if t.dtype != s[2] or tuple(t.shape) != tuple(s[1]) or not t.is_contiguous() or t.device != device:
            raise Mi355Error('%s: %s must be a dense %s tensor of shape %s on %s, got %s %s strides %s on %s'
                             % (who, s[0], s[2], tuple(s[1]), device, t.dtype, tuple(t.shape), t.stride(), t.device))
    return out


def peak_prob(hm, beta=1.0, out=None):
    """(idx int32 (B, K), xy fp32 (B, K, 2), p fp32 (B, K)) of the heat-maps hm (B, K, H, W), dense fp32: mi355_argmax2d's index and
    coordinates and the peak of softmax(beta * hm) per map (mi355_peak_prob); p is NaN for a map that holds a NaN or an inf.
    `out`: that triple, written in place; allocated only when not given, and never during graph capture."""
    who = 'peak_prob'
    _dense_f32(who, 'hm', hm)
    if hm.dim() != 4 or hm.numel() == 0:
        raise Mi355Error('%s: hm must be a non-empty (B, K, H, W) batch of heat-maps, got %s' % (who, tuple(hm.shape)))
    B, K, H, W = (int(s) for s in hm.shape)
    idx, xy, p = _occ_out(who, out, (('idx', (B, K), torch.int32), ('xy', (B, K, 2), torch.float32), ('p', (B, K), torch.float32)), hm.device)
    call('mi355_peak_prob', ptr(hm), float(beta), ptr(idx), ptr(xy), ptr(p), B * K, H, W, stream_ptr())
    return idx, xy, p


def teacher_select(p, xy=None, u=None, tau=0.0, prob=0.0, n=0, lo=1, hi=1, image_side=1, heatmap_size=(1, 1), gate_in=None, w_in=None,
                   out=None, stats=None):
    """The confidence gate and the occlusion boxes of a batch (mi355_teacher_select).  p (B, K): peak_prob's; xy (B, K, 2) in
    heat-map pixels; u (B, 1 + 2n) uniform draws on the device; gate_in (B, K) optional (the flags of a geometric view); w_in
    (B, K) or (B, K, 1) optional.  Returns (conf (B, K), w_out (w_in's shape, None without w_in), boxes int32 (B, n, 4) as
    (x0, y0, x1, y1) in image pixels, count int32 (B,)); boxes and count are None when n == 0 (the gate alone).  `stats`: an
    optional fp32 tensor of two elements, which receives the mean number of boxes per sample and the mean of conf.  `out`: the
    quadruple, written in place; allocated only when not given, and never during graph capture."""
    who = 'teacher_select'
    _dense_f32(who, 'p', p)
    if p.dim() != 2 or p.numel() == 0:
        raise Mi355Error('%s: p must be a non-empty (B, K) tensor, got %s' % (who, tuple(p.shape)))
    B, K = (int(s) for s in p.shape)
    n = int(n)
    if not 0 <= n <= OCC_MAX_BOXES:
        raise Mi355Error('%s: N=%d boxes per sample, 0..%d' % (who, n, OCC_MAX_BOXES))
    H, W = _size_hw(heatmap_size)
    others = [p]
    for what, t, shape in (('xy', xy, (B, K, 2)), ('u', u, (B, 1 + 2 * n)), ('gate_in', gate_in, (B, K))):
        if t is None:
            if n > 0 and what != 'gate_in':
                raise Mi355Error('%s: %s is needed to draw boxes (N=%d)' % (who, what, n))
            continue
        _dense_f32(who, what, t)
        if tuple(t.shape) != shape:
            raise Mi355Error('%s: %s has shape %s, the launch indexes %s' % (who, what, tuple(t.shape), shape))
        others.append(t)
    if w_in is not None:
        _dense_f32(who, 'w_in', w_in)
        if w_in.numel() != B * K or w_in.shape[0] != B:
            raise Mi355Error('%s: w_in %s for %d x %d maps' % (who, tuple(w_in.shape), B, K))
        others.append(w_in)
    if stats is not None:
        _dense_f32(who, 'stats', stats)
        _chk_room('%s stats' % who, stats, 2)
        others.append(stats)
    conf, w_out, boxes, count = _occ_out(who, out, (('conf', (B, K), torch.float32),
                                                    None if w_in is None else ('w_out', tuple(w_in.shape), torch.float32),
                                                    None if n == 0 else ('boxes', (B, n, 4), torch.int32),
                                                    None if n == 0 else ('count', (B,), torch.int32)), p.device)
    if any(t.device != p.device for t in others):
        raise Mi355Error('%s: the operands live on different devices' % who)
    call('mi355_teacher_select', ptr(p), ptr(xy) if n else 0, ptr(gate_in), ptr(w_in), ptr(u) if n else 0, float(tau), float(prob), n,
         int(lo), int(hi), int(image_side), H, W, ptr(conf), ptr(w_out), ptr(boxes), ptr(count), ptr(stats), B, K, stream_ptr())
    return conf, w_out, boxes, count


def occlude_images(x, boxes, out=None):
    """x (B, C, H, W), dense fp32, with every pixel inside any box of its sample set to +0.0 in all channels; every other word
    is copied bit for bit (mi355_occlude_images).  boxes: int32 (B, N, 4) on the device, (x0, y0, x1, y1) half-open, N <= 8.  x is
    only read.  `out` is allocated only when not given, and never during graph capture."""
    who = 'occlude_images'
    _dense_f32(who, 'x', x)
    if x.dim() != 4 or x.numel() == 0:
        raise Mi355Error('%s: x must be a non-empty (B, C, H, W) batch, got %s' % (who, tuple(x.shape)))
    B, C, H, W = (int(s) for s in x.shape)
    _chk_dev(boxes)
    if boxes.dtype != torch.int32 or boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4 or not boxes.is_contiguous():
        raise Mi355Error('%s: boxes must be a dense int32 (%d, N, 4) tensor, got %s %s strides %s' % (who, B, boxes.dtype, tuple(boxes.shape), boxes.stride()))
    N = int(boxes.shape[1])
    if N > OCC_MAX_BOXES:
        raise Mi355Error('%s: N=%d boxes per sample, 0..%d' % (who, N, OCC_MAX_BOXES))
    out, = _occ_out(who, None if out is None else (out,), (('out', (B, C, H, W), torch.float32),), x.device)
    if boxes.device != x.device:
        raise Mi355Error('%s: the operands live on different devices' % who)
    call('mi355_occlude_images', ptr(x), ptr(boxes) if N else 0, N, ptr(out), B, C, H, W, stream_ptr())
    return out


# ---------------------------------------------------------------- rendered hands (csrc/render.hip)
# include/mi355pose.h mi355_hand_rec, field for field
HAND_REC_DTYPE = _np.dtype([('jx', '<f4', 21), ('jy', '<f4', 21), ('jz', '<f4', 21), ('radius', '<f4', 20), ('skin', '<f4', 3),
                            ('light', '<f4', 3), ('ambient', '<f4'), ('bg0', '<f4', 3), ('bg1', '<f4', 3), ('grad', '<f4', 2),
                            ('grad_off', '<f4'), ('noise_amp', '<f4'), ('noise_inv_cell', '<f4'), ('noise_seed', '<u4'),
                            ('occ_a', '<f4', 2), ('occ_b', '<f4', 2), ('occ_r', '<f4'), ('occ_z', '<f4'), ('occ_col', '<f4', 3),
                            ('sensor_sigma', '<f4'), ('sensor_seed', '<u4'), ('gain', '<f4', 3), ('bias', '<f4', 3), ('reserved', '<u4')])
assert HAND_REC_DTYPE.itemsize == 480
RENDER_SIDES = tuple(range(16, 513, 16))


def render_norm(mean=None, std=None):
    """(mean3, inv_std3) as the fp32 values the kernel subtracts and multiplies by: 1 / std formed in double, rounded once."""
    mean = _np.asarray(MEAN if mean is None else mean, dtype=_np.float64)
    std = _np.asarray(STD if std is None else std, dtype=_np.float64)
    if mean.shape != (3,) or std.shape != (3,) or not (_np.isfinite(mean).all() and _np.isfinite(std).all() and (std > 0).all()):
        raise Mi355Error('render_hands: mean and std must be three finite values each, std > 0')
    return mean.astype(_np.float32), (1.0 / std).astype(_np.float32)


def render_hands(recs, image_size, out=None, out_ema=None, ids=None, mean=None, std=None):
    """The images of a batch of hand records (mi355_render_hands): recs is a dense device tensor holding B records of
    HAND_REC_DTYPE (any element type; B = its bytes / 480), image_size = S, a multiple of 16 from 16 to 512.  Returns `out`
    (B, 3, S, S) fp32, normalised with mean / std (the loaders' by default); out_ema, when given, receives the same scene with gain 1,
    bias 0 and no sensor noise, and ids (B, S, S) uint8 the front-most primitive at each pixel centre (0 background, 1 .. 20 bone
    index + 1, 21 the occluder).  `out` is allocated only when not given, and never during graph capture.  Every check raises
    before anything is launched."""
    who = 'render_hands'
    _chk_dev(recs, out, out_ema, ids)
    S = int(image_size)
    if S != image_size or S not in RENDER_SIDES:
        raise Mi355Error('%s: image_size=%r is not a multiple of 16 from 16 to 512' % (who, image_size))
    nbytes = recs.numel() * recs.element_size()
    if not recs.is_contiguous() or nbytes == 0 or nbytes % HAND_REC_DTYPE.itemsize:
        raise Mi355Error('%s: recs must be a dense tensor of whole %d-byte records, got %s %s strides %s' % (
            who, HAND_REC_DTYPE.itemsize, recs.dtype, tuple(recs.shape), recs.stride()))
    B = nbytes // HAND_REC_DTYPE.itemsize
    if out is None:
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('%s: out would be allocated during graph capture; run one eager call first' % who)
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=recs.device)
    for what, t, shape, dt, align in (('recs', recs, None, None, 16), ('out', out, (B, 3, S, S), torch.float32, 16),
                                      ('out_ema', out_ema, (B, 3, S, S), torch.float32, 16), ('ids', ids, (B, S, S), torch.uint8, 4)):
        if t is None:
            continue
        if shape is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise Mi355Error('%s: %s must be a dense %s tensor of shape %s, got %s %s strides %s' % (who, what, dt, shape, t.dtype, tuple(t.shape), t.stride()))
        if t.data_ptr() % align:
            raise Mi355Error('%s: %s must be %d-byte aligned (offset %d)' % (who, what, align, t.data_ptr() % align))
        if t.device != recs.device:
            raise Mi355Error('%s: the operands live on different devices' % who)
    spans = [(what, t.data_ptr(), t.numel() * t.element_size()) for what, t in (('recs', recs), ('out', out), ('out_ema', out_ema), ('ids', ids))
             if t is not None]
    for u in range(len(spans)):
        for v in range(u + 1, len(spans)):
            (na, pa, la), (nb, pb, lb) = spans[u], spans[v]
            if pa < pb + lb and pb < pa + la:
                raise Mi355Error('%s: %s and %s overlap' % (who, na, nb))
    m3, s3 = render_norm(mean, std)
    fl = ctypes.c_float * 3
    call('mi355_render_hands', ptr(recs), ptr(out), ptr(out_ema), ptr(ids), B, S, fl(*m3.tolist()), fl(*s3.tolist()), stream_ptr())
    return out


# ---------------------------------------------------------------- hand tracking (csrc/track.hip)
# include/mi355pose.h mi355_track_rec, field for field
TRACK_REC_DTYPE = _np.dtype([('frame', '<i4'), ('x0', '<f4'), ('y0', '<f4'), ('side', '<f4'), ('mirror', '<i4'), ('live', '<i4'),
                             ('lost', '<i4'), ('reserved', '<i4')])
assert TRACK_REC_DTYPE.itemsize == 32
TRACK_MAX_COORD, TRACK_MAX_FRAME, TRACK_MAX_JOINTS, TRACK_MAX_SIDE = 1048576.0, 4096, 64, 512      # include/mi355pose.h MI355_TRACK_*
TRACK_SIDES = tuple(range(16, TRACK_MAX_SIDE + 1, 16))
# tau, min_joints, alpha, grow, max_lost and min_side are PLACEHOLDERS: their effect has not been measured.  scale = 1.5 is the data
# sets' crop (scale_box(get_bounding_box(keypoint2d), w, h, 1.5)).
TRACK_DEFAULTS = dict(tau=0.02, min_joints=8, scale=1.5, alpha=1.0, grow=1.25, max_lost=5, min_side=16.0)


def track_records(n, frame=0, x0=0.0, y0=0.0, side=1.0, mirror=0, live=0, lost=0):
    """A numpy structured array of n records (TRACK_REC_DTYPE); every argument is a scalar or a sequence of n values."""
    rec = _np.zeros(int(n), TRACK_REC_DTYPE)
    for name, v in (('frame', frame), ('x0', x0), ('y0', y0), ('side', side), ('mirror', mirror), ('live', live), ('lost', lost)):
        rec[name] = v
    return rec


def pack_track_records(rec, device=None, out=None):
    """The (N, 8) int32 tensor that holds the records `rec` (a TRACK_REC_DTYPE array) word for word: new on `device`, or `out`
    rewritten in place (a tracker's records stay at their address)."""
    rec = _np.ascontiguousarray(rec, dtype=TRACK_REC_DTYPE).reshape(-1)
    host = torch.from_numpy(rec.view(_np.int32).reshape(-1, 8).copy())
    if out is None:
        return host.to(device)
    if out.dtype != torch.int32 or tuple(out.shape) != tuple(host.shape) or not out.is_contiguous():
        raise Mi355Error('pack_track_records: out must be a dense int32 %s tensor, got %s %s' % (tuple(host.shape), out.dtype, tuple(out.shape)))
    out.copy_(host)
    return out


def unpack_track_records(recs):
    """The records of an (N, 8) int32 tensor as a TRACK_REC_DTYPE array on the host (a device tensor is read back: synchronises)."""
    a = _np.ascontiguousarray(recs.detach().cpu().numpy()).reshape(-1, 8)
    if a.dtype != _np.int32:
        raise Mi355Error('unpack_track_records: the records are an int32 (N, 8) tensor, got %s' % (a.dtype,))
    return a.view(TRACK_REC_DTYPE).reshape(-1)


def _chk_track_recs(who, what, recs):
    _chk_dev(recs)
    if recs.dtype != torch.int32 or recs.dim() != 2 or recs.shape[1] != 8 or recs.shape[0] < 1 or not recs.is_contiguous():
        raise Mi355Error('%s: %s must be a dense int32 (N, 8) tensor of records, got %s %s strides %s' % (who, what, recs.dtype, tuple(recs.shape), recs.stride()))
    return int(recs.shape[0])


def roi_crop_normalize(frames, recs, S, out=None, mean=MEAN, std=STD):
    """out (N, 3, S, S) fp32: the square of every record of `recs` (int32 (N, 8) on the device, pack_track_records) cut out of the
    uint8 (F, Hf, Wf, 3) RGB device tensor `frames`, resized to S x S, mirrored where the record says so and normalised
    (mi355_roi_crop_normalize).  The records are read on the device only; an unusable one gives an image of zeros.  `out` is
    allocated only when not given, and never during graph capture.  Every check raises before anything is launched."""
    who = 'roi_crop_normalize'
    _chk_dev(frames, out)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0 or not frames.is_contiguous():
        raise Mi355Error('%s: frames must be a dense uint8 (F, Hf, Wf, 3) tensor, got %s %s strides %s' % (who, frames.dtype, tuple(frames.shape), frames.stride()))
    F, Hf, Wf = (int(s) for s in frames.shape[:3])
    N = _chk_track_recs(who, 'recs', recs)
    if int(S) != S or S not in TRACK_SIDES:
        raise Mi355Error('%s: S=%r is not a multiple of 16 from 16 to %d' % (who, S, TRACK_MAX_SIDE))
    S = int(S)
    out, = _occ_out(who, None if out is None else (out,), (('out', (N, 3, S, S), torch.float32),), frames.device)
    if recs.device != frames.device:
        raise Mi355Error('%s: the operands live on different devices' % who)
    norm = _np.array(list(mean) + list(std), dtype=_np.float32)
    call('mi355_roi_crop_normalize', ptr(frames), F, Hf, Wf, ptr(recs), N, S, norm.ctypes.data, ptr(out), stream_ptr())
    return out


def track_params(frame_shape, S, **kw):
    """The mi355_track_params of a frame (Hf, Wf) and crop side S; keywords override TRACK_DEFAULTS."""
    from . import TrackParams
    unknown = sorted(set(kw) - set(TRACK_DEFAULTS))
    if unknown:
        raise Mi355Error('track_update: unknown parameter(s) %s (known: %s)' % (', '.join(unknown), ', '.join(sorted(TRACK_DEFAULTS))))
    p = dict(TRACK_DEFAULTS, **kw)
    Hf, Wf = _size_hw(frame_shape)
    return TrackParams(float(p['tau']), int(p['min_joints']), float(p['scale']), float(p['alpha']), float(p['grow']), int(p['max_lost']),
                       float(p['min_side']), Wf, Hf, int(S))


def track_update(recs, xy, conf, params, out=None, rec_out=None):
    """Key points back to the frame and the next box of every hand (mi355_track_update).  recs: int32 (N, 8) records on the device;
    xy (N, K, 2) fp32 key points in crop pixels; conf (N, K) fp32; params: track_params(...).  Returns (kp (N, K, 2) in frame pixels,
    vis (N, K) 1.0 / 0.0, score (N,), rec_out); `rec_out` defaults to `recs` itself (updated in place).  `out`: the triple (kp, vis,
    score), written in place; allocated only when not given, and never during graph capture."""
    who = 'track_update'
    N = _chk_track_recs(who, 'recs', recs)
    _dense_f32(who, 'xy', xy)
    _dense_f32(who, 'conf', conf)
    if xy.dim() != 3 or xy.shape[0] != N or xy.shape[2] != 2 or xy.shape[1] < 1:
        raise Mi355Error('%s: xy must be (%d, K, 2), got %s' % (who, N, tuple(xy.shape)))
    K = int(xy.shape[1])
    if conf.numel() != N * K or conf.shape[0] != N:
        raise Mi355Error('%s: conf %s for %d x %d joints' % (who, tuple(conf.shape), N, K))
    if rec_out is None:
        rec_out = recs
    elif _chk_track_recs(who, 'rec_out', rec_out) != N:
        raise Mi355Error('%s: rec_out holds %d records, recs %d' % (who, rec_out.shape[0], N))
    kp, vis, score = _occ_out(who, out, (('kp', (N, K, 2), torch.float32), ('vis', (N, K), torch.float32), ('score', (N,), torch.float32)), recs.device)
    if any(t.device != recs.device for t in (xy, conf, rec_out)):
        raise Mi355Error('%s: the operands live on different devices' % who)
    call('mi355_track_update', ptr(recs), ptr(xy), ptr(conf), params, ptr(kp), ptr(vis), ptr(score), ptr(rec_out), N, K, stream_ptr())
    return kp, vis, score, rec_out


# ---------------------------------------------------------------- MMD alignment (csrc/mmd.hip)
MMD_MAX_ROWS, MMD_MAX_KERNELS = 256, 8
_mmd_ws = {}


def _mmd_workspace(device, B, K):
    """The (K, n, n) fp32 distance / coefficient matrices of mmd_heatmap, one buffer per shape: a captured graph that contains the
    launches keeps seeing the address it was captured with.  Allocated outside graph capture only (warm up before capturing)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), B, K)
    buf = _mmd_ws.get(key)
    if buf is None:
        if torch.cuda.is_current_stream_capturing():
            raise Mi355Error('mmd_heatmap: the workspace for B=%d K=%d would be allocated during graph capture: warm up first' % (B, K))
        nbytes = load().mi355_mmd_workspace(B, K)
        if nbytes == 0:
            raise Mi355Error('mmd_heatmap: B=%d K=%d refused (1 <= B, n = 2 B <= %d rows, 1 <= K)' % (B, K, MMD_MAX_ROWS))
        buf = _mmd_ws[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    return buf


def mmd_heatmap(source, target, want_source_grad, want_target_grad, kernel_mul=2.0, kernel_num=5, fix_sigma=None, scale=1.0,
                rows=None, grad_source=None, grad_target=None):
    """Per-joint multi-kernel MMD of source, target (B, K, H, W) or (B, K, HW), fp32 with every row (b, k) contiguous.  Returns
    (rows [K] = loss_k, grad_source or None, grad_target or None); the scalar loss is reduce_sum(rows, scale / K) and the gradients
    are d(that scalar) / d source and / d target.  A side whose gradient is not wanted is neither allocated nor written."""
    _chk_dev(source, target)
    for what, t in (('source', source), ('target', target)):
        if t.dim() not in (3, 4) or t.dtype != torch.float32 or not t.is_contiguous():
            raise Mi355Error('mmd_heatmap: %s must be a contiguous fp32 (B, K, HW) or (B, K, H, W) tensor, got %s %s strides %s'
                             % (what, t.dtype, tuple(t.shape), t.stride()))
    if tuple(source.shape) != tuple(target.shape):
        raise Mi355Error('mmd_heatmap: source %s vs target %s: the kernel matrix is sliced by one batch size' % (tuple(source.shape), tuple(target.shape)))
    B, K = source.shape[:2]
    HW = source[0, 0].numel() if B and K else 0
    work = _mmd_workspace(source.device, B, K)
    n = 2 * B
    if rows is None:
        rows = torch.empty((K,), dtype=torch.float32, device=source.device)
    if want_source_grad and grad_source is None:
        grad_source = torch.empty_like(source)
    if want_target_grad and grad_target is None:
        grad_target = torch.empty_like(target)
    _chk_dev(rows, grad_source, grad_target)
    _chk_room('mmd_heatmap source', source, B * K * HW)
    _chk_room('mmd_heatmap target', target, B * K * HW)
    _chk_room('mmd_heatmap work', work, K * n * n)
    _chk_room('mmd_heatmap rows', rows, K)
    _chk_room('mmd_heatmap grad_source', grad_source if want_source_grad else None, B * K * HW)
    _chk_room('mmd_heatmap grad_target', grad_target if want_target_grad else None, B * K * HW)
    call('mi355_mmd_heatmap', ptr(source), ptr(target), ptr(work), work.numel() * 4, ptr(rows),
         ptr(grad_source) if want_source_grad else 0, ptr(grad_target) if want_target_grad else 0, int(B), int(K), int(HW),
         float(kernel_mul), int(kernel_num), float(fix_sigma) if fix_sigma else 0.0, float(scale), stream_ptr())
    return rows, (grad_source if want_source_grad else None), (grad_target if want_target_grad else None)


# ---------------------------------------------------------------- joint feature alignment (csrc/jfa.hip)
JFA_MAX_JOINTS = 32
JFA_AXES = {'ref': 1, 'xy': 0}        # 'ref': x selects the rows (the reference's indexing), 'xy': y selects the rows


def joint_divisor(radius, scale=1.0):
    """(2 radius + 1)^2 / scale as the fp32 the kernels divide by; with scale = 1 the reference's 13 * 13."""
    if not scale > 0:
        raise Mi355Error('joint_pool: scale must be positive, got %r' % (scale,))
    return float(torch.tensor((2 * int(radius) + 1) ** 2 / float(scale), dtype=torch.float64).to(torch.float32))


def _chk_joints(who, xy, B):
    if xy.dim() != 3 or xy.shape[0] != B or xy.shape[2] != 2 or xy.dtype != torch.float32 or not xy.is_contiguous():
        raise Mi355Error('%s: key points must be a contiguous fp32 (%d, K, 2) tensor, got %s %s strides %s'
                         % (who, B, xy.dtype, tuple(xy.shape), xy.stride()))
    if not 1 <= xy.shape[1] <= JFA_MAX_JOINTS:
        raise Mi355Error('%s: K=%d joints (1 .. %d)' % (who, xy.shape[1], JFA_MAX_JOINTS))
    return xy.shape[1]


def _chk_jfa(who, C, H, W, radius, axes):
    if axes not in JFA_AXES:
        raise Mi355Error("%s: axes must be 'ref' or 'xy', got %r" % (who, axes))
    if C < 8 or C % 8:
        raise Mi355Error('%s: C=%d channels (a multiple of 8, at least 8)' % (who, C))
    if H < 1 or W < 1 or int(radius) < 1 or int(radius) != radius:
        raise Mi355Error('%s: H=%d W=%d radius=%r (each at least 1)' % (who, H, W, radius))


def _chk_desc(who, what, t, shape=None):
    if t.dim() != 3 or t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise Mi355Error('%s: %s must be a contiguous, 16-byte aligned fp32 (B, K, C) tensor%s, got %s %s strides %s offset %d'
                         % (who, what, '' if shape is None else ' of shape %s' % (tuple(shape),), t.dtype, tuple(t.shape), t.stride(), t.data_ptr() % 16))


def _pool_args(who, f, xy, radius, axes, out):
    """The checks of the pooling wrapper `who` (feature map, key points, radius and axes, 16-byte start, room) and its `out`, made
    when None: (B, K, C, H, W, out)."""
    _chk_feature(who + ' feature', f)
    B, C, H, W = f.shape
    K = _chk_joints(who, xy, B)
    _chk_jfa(who, C, H, W, radius, axes)
    if f.data_ptr() % 16:
        raise Mi355Error('%s: the feature map must start on a 16-byte boundary (offset %d)' % (who, f.data_ptr() % 16))
    if out is None:
        out = torch.empty((B, K, C), dtype=torch.float32, device=f.device)
    _chk_desc(who, 'out', out, (B, K, C))
    _chk_room(who + ' feature', f, B * C * H * W)
    _chk_room(who + ' xy', xy, B * K * 2)
    _chk_room(who + ' out', out, B * K * C)
    return B, K, C, H, W, out


def _gather_args(who, g, what, per_image, xy, out, radius, axes):
    """The checks of the gather wrapper `who`: the feature gradient `out`, key points, radius and axes, the incoming gradient `g`
    named `what` ((B, K, C) when `per_image`, else (K, C)), 16-byte start, room: (B, K, C, H, W)."""
    _chk_feature(who + ' out', out)
    B, C, H, W = out.shape
    K = _chk_joints(who, xy, B)
    _chk_jfa(who, C, H, W, radius, axes)
    if per_image:
        _chk_desc(who, what, g, (B, K, C))
    else:
        _chk_proto(who, what, g, (K, C))
    if out.data_ptr() % 16:
        raise Mi355Error('%s: the feature gradient must start on a 16-byte boundary (offset %d)' % (who, out.data_ptr() % 16))
    _chk_room('%s %s' % (who, what), g, (B if per_image else 1) * K * C)
    _chk_room(who + ' out', out, B * C * H * W)
    return B, K, C, H, W


def _kl_buffers(who, chk, a, rows, grads):
    """rows (one per row of the operand `a`) and the wanted gradients of the KL wrapper `who`, each made when None, the gradients
    checked with `chk` against `a`; `grads`: (name, tensor or None, wanted) for either side.  Returns (rows, [gradient or None,
    gradient or None])."""
    if rows is None:
        rows = torch.empty(a.shape[:-1], dtype=torch.float32, device=a.device)
    grads = [(what, torch.empty_like(a) if want and g is None else g, want) for what, g, want in grads]
    if rows.dtype != torch.float32 or not rows.is_contiguous():
        raise Mi355Error('%s: rows must be a contiguous fp32 tensor' % who)
    for what, g, want in grads:
        if want:
            chk(who, what, g, a.shape)
    _chk_room(who + ' rows', rows, a.numel() // a.shape[-1])
    return rows, [g if want else None for _, g, want in grads]


def joint_pool(f, xy, radius=6, axes='ref', divisor=None, out=None):
    """desc (B, K, C) fp32: the box sum of the window of the channels_last feature map f (B, C, H, W; bf16 / fp32) around each key
    point xy (B, K, 2) = (x, y), divided by `divisor` ((2 radius + 1)^2 when None): the reference's loss1
    (uda/model/loss.py:331-365)."""
    _chk_dev(f, xy, out)
    B, K, C, H, W, out = _pool_args('joint_pool', f, xy, radius, axes, out)
    call('mi355_jfa_pool', ptr(f), ptr(xy), ptr(out), B, K, C, H, W, int(radius), joint_divisor(radius) if divisor is None else float(divisor),
         JFA_AXES[axes], dtype_code(f.dtype), stream_ptr())
    return out


def joint_kl(a, b, want_a, want_b, scale=1.0, rows=None, grad_a=None, grad_b=None):
    """KL between the channel distributions of two sets of descriptors a, b (B, K, C) fp32 (the reference's loss3 behind its two
    loss1 calls, uda/model/loss.py:368-378): a goes through log_softmax, b is normalised to sum 1 after adding 1e-6.  Returns
    (rows (B, K), grad_a or None, grad_b or None); the scalar loss is reduce_sum(rows, scale / (B K)) and the gradients are
    d(that scalar) / d a and / d b.  A side whose gradient is not wanted is neither allocated nor written."""
    _chk_dev(a, b, rows, grad_a, grad_b)
    _chk_desc('joint_kl', 'a', a)
    _chk_desc('joint_kl', 'b', b, a.shape)
    B, K, C = a.shape
    if B < 1 or K < 1 or C < 8 or C % 8:
        raise Mi355Error('joint_kl: B=%d K=%d C=%d (C a multiple of 8, at least 8)' % (B, K, C))
    rows, (grad_a, grad_b) = _kl_buffers('joint_kl', _chk_desc, a, rows, (('grad_a', grad_a, want_a), ('grad_b', grad_b, want_b)))
    call('mi355_jfa_kl', ptr(a), ptr(b), ptr(rows), ptr(grad_a) if want_a else 0, ptr(grad_b) if want_b else 0, B * K, C,
         float(scale) / (B * K), stream_ptr())
    return rows, grad_a, grad_b


def joint_scatter(gd, xy, out, accumulate, radius=6, axes='ref', divisor=None):
    """The backward of joint_pool: `out` (B, C, H, W channels_last, bf16 / fp32) receives, at every pixel, the sum of gd[b, j, :] /
    divisor over the joints whose window holds the pixel (ascending j, fp32).  accumulate=False writes it (zeros outside every
    window); accumulate=True adds it onto what `out` holds, one rounding, and leaves uncovered pixels alone."""
    _chk_dev(gd, xy, out)
    B, K, C, H, W = _gather_args('joint_scatter', gd, 'gd', True, xy, out, radius, axes)
    call('mi355_jfa_scatter', ptr(gd), ptr(xy), ptr(out), int(bool(accumulate)), B, K, C, H, W, int(radius),
         joint_divisor(radius) if divisor is None else float(divisor), JFA_AXES[axes], dtype_code(out.dtype), stream_ptr())
    return out


# ---------------------------------------------------------------- prototype alignment with running memory (csrc/proto.hip)
PROTO_MODES = {'kl': 0, 'softkl': 1}      # lossx (uda/model/loss.py:381-466), lossx3 (:560-652)


def proto_blend(m, device=None, out=None):
    """The device record {m, 1 - m} of proto_update / proto_scatter as a 2-element fp32 tensor (new, or `out` rewritten): both
    are formed in double and rounded once, as the reference's Python floats ``m`` and ``(1 - m)`` are where they meet the tensor."""
    m = float(m)
    if not 0.0 < m <= 1.0:
        raise Mi355Error('proto_blend: m must be in (0, 1], got %r' % (m,))
    host = torch.tensor([m, 1.0 - m], dtype=torch.float64).to(torch.float32)
    if out is None:
        return host.to(device)
    if out.dtype != torch.float32 or out.numel() != 2 or not out.is_contiguous():
        raise Mi355Error('proto_blend: out must be a contiguous fp32 tensor of 2 elements')
    out.copy_(host)
    return out


def _chk_proto(who, what, t, shape=None):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise Mi355Error('%s: %s must be a contiguous, 16-byte aligned fp32 (K, C) tensor%s, got %s %s strides %s offset %d'
                         % (who, what, '' if shape is None else ' of shape %s' % (tuple(shape),), t.dtype, tuple(t.shape), t.stride(), t.data_ptr() % 16))
    if not 1 <= t.shape[0] <= JFA_MAX_JOINTS or t.shape[1] < 8 or t.shape[1] % 8:
        raise Mi355Error('%s: %s K=%d C=%d (1 .. %d joints, C a multiple of 8, at least 8)' % (who, what, t.shape[0], t.shape[1], JFA_MAX_JOINTS))


def _chk_blend(who, blend):
    if blend.dtype != torch.float32 or blend.numel() != 2 or not blend.is_contiguous():
        raise Mi355Error('%s: blend must be the 2-element fp32 record of proto_blend, got %s %s' % (who, blend.dtype, tuple(blend.shape)))


def proto_pool(f, xy, radius=6, axes='ref', out=None):
    """desc (B, K, C) fp32: the box sum of the window of the channels_last feature map f (B, C, H, W; bf16 / fp32) around each key
    point xy (B, K, 2) = (x, y), divided by the window's own s_row * s_col, s = hi - lo + 1 (the reference's lossx.loss1 up to its
    stack, uda/model/loss.py:402-433)."""
    _chk_dev(f, xy, out)
    B, K, C, H, W, out = _pool_args('proto_pool', f, xy, radius, axes, out)
    call('mi355_proto_pool', ptr(f), ptr(xy), ptr(out), B, K, C, H, W, int(radius), JFA_AXES[axes], dtype_code(f.dtype), stream_ptr())
    return out


def proto_update(desc, memory, blend, out=None):
    """P (K, C) = m * mean_b desc[b] + (1 - m) * memory, and memory <- P in place (uda/model/loss.py:436-448, :454): desc (B, K, C)
    fp32, memory (K, C) fp32 at its fixed address, blend = proto_blend(m).  Returns P (new, or `out`; never the memory itself)."""
    _chk_dev(desc, memory, blend, out)
    _chk_desc('proto_update', 'desc', desc)
    B, K, C = desc.shape
    if B < 1:
        raise Mi355Error('proto_update: B=%d' % B)
    _chk_proto('proto_update', 'memory', memory, (K, C))
    _chk_blend('proto_update', blend)
    if out is None:
        out = torch.empty((K, C), dtype=torch.float32, device=desc.device)
    _chk_proto('proto_update', 'out', out, (K, C))
    if out.data_ptr() == memory.data_ptr():
        raise Mi355Error('proto_update: out must not be the memory itself (the loss needs P after the memory is overwritten)')
    _chk_room('proto_update desc', desc, B * K * C)
    _chk_room('proto_update memory', memory, K * C)
    _chk_room('proto_update out', out, K * C)
    call('mi355_proto_update', ptr(desc), ptr(memory), ptr(blend), ptr(out), B, K, C, stream_ptr())
    return out


def proto_kl(pt, ps, want_t, want_s, mode='kl', scale=1.0, rows=None, grad_t=None, grad_s=None):
    """KL between the channel distributions of the prototypes pt, ps (K, C) fp32: pt goes through log_softmax; mode 'kl' (lossx,
    uda/model/loss.py:455-466) normalises ps to sum 1, mode 'softkl' (lossx3, :645) takes its softmax.  Returns (rows (K,), grad_t
    or None, grad_s or None); the scalar loss is reduce_sum(rows, scale / K) for 'kl' and reduce_sum(rows, scale) for 'softkl',
    and the gradients are d(that scalar) / d pt and / d ps.  A side whose gradient is not wanted is neither allocated nor written."""
    _chk_dev(pt, ps, rows, grad_t, grad_s)
    if mode not in PROTO_MODES:
        raise Mi355Error("proto_kl: mode must be 'kl' or 'softkl', got %r" % (mode,))
    _chk_proto('proto_kl', 'pt', pt)
    _chk_proto('proto_kl', 'ps', ps, pt.shape)
    K, C = pt.shape
    rows, (grad_t, grad_s) = _kl_buffers('proto_kl', _chk_proto, pt, rows, (('grad_t', grad_t, want_t), ('grad_s', grad_s, want_s)))
    call('mi355_proto_kl', ptr(pt), ptr(ps), ptr(rows), ptr(grad_t) if want_t else 0, ptr(grad_s) if want_s else 0, K, C,
         PROTO_MODES[mode], float(scale) / K if mode == 'kl' else float(scale), stream_ptr())
    return rows, grad_t, grad_s


def proto_scatter(gp, xy, blend, out, accumulate, radius=6, axes='ref'):
    """The backward of proto_pool + proto_update: `out` (B, C, H, W channels_last, bf16 / fp32) receives, at every pixel, the sum of
    (gp[j, :] * (m / B)) / (s_row s_col)(b, j) over the joints whose window holds the pixel (ascending j, fp32); gp (K, C) is the
    gradient w.r.t. the prototypes, the same for every image.  accumulate=False writes it (zeros outside every window);
    accumulate=True adds it onto what `out` holds, one rounding, and leaves uncovered pixels alone."""
    _chk_dev(gp, xy, blend, out)
    _chk_blend('proto_scatter', blend)
    B, K, C, H, W = _gather_args('proto_scatter', gp, 'gp', False, xy, out, radius, axes)
    call('mi355_proto_scatter', ptr(gp), ptr(xy), ptr(blend), ptr(out), int(bool(accumulate)), B, K, C, H, W, int(radius),
         JFA_AXES[axes], dtype_code(out.dtype), stream_ptr())
    return out


# ---------------------------------------------------------------- kernel timer (bench.py roofline)
def spin_us(us):
    call('mi355_spin_us', int(us), stream_ptr())


def prof_event_overhead_us(n=256):
    us = ctypes.c_double(0)
    call('mi355_prof_event_overhead_us', int(n), stream_ptr(), ctypes.byref(us))
    return us.value


def prof_read_split(flop_per_byte):
    out = (ctypes.c_double * 8)()
    call('mi355_prof_read_split', float(flop_per_byte), out)
    return list(out)


def prof_enable(on):
    call('mi355_prof_enable', int(on))


def prof_reset():
    call('mi355_prof_reset')


def prof_launches():
    """Every launch logged since the last reset, in launch order: dicts with family, us (event-timed), flops, bytes, label."""
    n = ctypes.c_long()
    call('mi355_prof_launch_count', ctypes.byref(n))
    out = []
    fam, us, fl, by = ctypes.c_int(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    buf = ctypes.create_string_buffer(192)
    for i in range(n.value):
        call('mi355_prof_read_launch', i, ctypes.byref(fam), ctypes.byref(us), ctypes.byref(fl), ctypes.byref(by), buf, 192)
        out.append({'family': fam.value, 'us': us.value, 'flops': fl.value, 'bytes': by.value, 'label': buf.value.decode()})
    return out


def prof_read():
    ms, n, fl, by = ctypes.c_double(), ctypes.c_long(), ctypes.c_double(), ctypes.c_double()
    call('mi355_prof_read', ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by))
    return ms.value, n.value, fl.value, by.value
