"""Two independent numpy float64 restatements of the Fourier-domain stylisation (Yang and Soatto, CVPR 2020) as
include/mi355pose.h states it for mi355_fda_transfer.  Written from that description; the reference project has no such function.

(a) full_fft: the published form on de-normalised planes -- fft2 -> fftshift -> the centre (2b+1)^2 window of the amplitude taken
    from the target -> ifftshift -> ifft2 -> real -- re-normalised at the end.
(b) partial_dft: only the window, as W_r X W_c^T with (2b+1) x H and (2b+1) x W twiddle matrices; the affine folded into the
    coefficients (times std; plus mean H W at DC); the phase factor 1 where |Fs| is exactly 0; the change to the image as the
    inverse partial DFT of the amplitude difference.

Inputs are float32 arrays (B, C, H, W); mean / std are rounded to float32 first, as the entry point takes them.  Both return
float64: the caller rounds once."""
import math

import numpy as np


def band(H, W, beta):
    return int(math.floor(min(H, W) * beta))


def _norm(mean, std, C):
    m = np.asarray(mean, np.float32)[:C].astype(np.float64)
    s = np.asarray(std, np.float32)[:C].astype(np.float64)
    assert m.shape == (C,) and s.shape == (C,)
    return m.reshape(1, C, 1, 1), s.reshape(1, C, 1, 1)


def full_fft(x_s, x_t, b, mean, std):
    B, C, H, W = x_s.shape
    m, s = _norm(mean, std, C)
    p_s, p_t = x_s.astype(np.float64) * s + m, x_t.astype(np.float64) * s + m
    f_s, f_t = np.fft.fft2(p_s, axes=(-2, -1)), np.fft.fft2(p_t, axes=(-2, -1))
    amp_s, pha_s, amp_t = np.abs(f_s), np.angle(f_s), np.abs(f_t)
    a_s, a_t = np.fft.fftshift(amp_s, axes=(-2, -1)), np.fft.fftshift(amp_t, axes=(-2, -1))
    ch, cw = H // 2, W // 2
    a_s[..., ch - b:ch + b + 1, cw - b:cw + b + 1] = a_t[..., ch - b:ch + b + 1, cw - b:cw + b + 1]
    a_s = np.fft.ifftshift(a_s, axes=(-2, -1))
    out01 = np.real(np.fft.ifft2(a_s * np.exp(1j * pha_s), axes=(-2, -1)))
    return (out01 - m) / s


def window(x, b, mean, std):
    """The de-normalised window F01[u, v], u, v in [-b, b] (index u + b, v + b), of every plane of normalised x: (B, C, 2b+1, 2b+1)."""
    B, C, H, W = x.shape
    m, s = _norm(mean, std, C)
    u = np.arange(-b, b + 1)
    w_r = np.exp(-2j * np.pi * ((u[:, None] * np.arange(H)[None, :]) % H) / H)          # (2b+1, H)
    w_c = np.exp(-2j * np.pi * ((u[:, None] * np.arange(W)[None, :]) % W) / W)          # (2b+1, W)
    f = np.einsum('uy,bcyx,vx->bcuv', w_r, x.astype(np.float64), w_c) * s
    f[:, :, b, b] += (m * H * W)[..., 0, 0]
    return f


def partial_dft(x_s, x_t, b, mean, std, want_min=False):
    B, C, H, W = x_s.shape
    m, s = _norm(mean, std, C)
    f_s, f_t = window(x_s, b, mean, std), window(x_t, b, mean, std)
    a_s, a_t = np.abs(f_s), np.abs(f_t)
    zero = a_s == 0
    phase = np.where(zero, 1.0, f_s / np.where(zero, 1.0, a_s))
    d = (a_t - a_s) * phase
    u = np.arange(-b, b + 1)
    e_r = np.exp(2j * np.pi * ((u[:, None] * np.arange(H)[None, :]) % H) / H)
    e_c = np.exp(2j * np.pi * ((u[:, None] * np.arange(W)[None, :]) % W) / W)
    delta = np.real(np.einsum('uy,bcuv,vx->bcyx', e_r, d, e_c)) / (H * W * s)
    out = x_s.astype(np.float64) + delta
    if want_min:
        return out, float((a_s / (H * W)).min())
    return out


def inputs(shape, seed, mean, std):
    """The generators of the tests: s01 uniform, t01 its square law; both normalised in float32."""
    rng = np.random.default_rng(seed)
    s01, t01 = rng.random(shape), rng.random(shape) ** 2
    C = shape[1]
    m = np.asarray(mean, np.float32)[:C].reshape(1, C, 1, 1)
    s = np.asarray(std, np.float32)[:C].reshape(1, C, 1, 1)
    return ((s01.astype(np.float32) - m) / s).astype(np.float32), ((t01.astype(np.float32) - m) / s).astype(np.float32)
