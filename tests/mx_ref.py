"""CPU restatement of the MX (block-scaled e4m3) quantisation rule of csrc/mx_fp8.hip, in torch.

Per block of 32 consecutive elements along the contracted (contiguous) axis: amax = max |x| over the finite elements,
amax = m * 2^E with m in [1, 2), e = E - 8 + (m > 1.75), clamped to [-127, 127]; scale byte = e + 127, or 0xFF when the
block holds a NaN or an Inf; element = RNE-to-e4m3fn(x * 2^-e) (Inf saturates to +-448, NaN stays NaN)."""
import torch

BLOCK = 32


def mx_exp(amax):
    """e of the rule for a float32 tensor of finite amax values >= 0 (from the bits: exact for subnormals and zero too)"""
    bits = amax.float().contiguous().view(torch.int32).long()
    e = (bits >> 23) - 127 - 8 + ((bits & 0x7fffff) > 0x600000).long()
    return e.clamp(-127, 127)


def mx_quantize_ref(x):
    """x [..., C] (bf16 / fp32, C a multiple of 32; the last axis is the blocked one) -> (q uint8 [..., C], s uint8 [..., C/32])"""
    shape = x.shape
    xf = x.float().reshape(-1, BLOCK)
    fin = torch.isfinite(xf)
    amax = torch.where(fin, xf.abs(), torch.zeros_like(xf)).amax(1)
    e = mx_exp(amax)
    inv = torch.pow(2.0, (-e).double()).float()          # 2^-e, exact in fp32 (e <= 120 for finite amax)
    v = (xf * inv[:, None]).clamp(-448.0, 448.0)         # (clamp keeps NaN)
    q = v.to(torch.float8_e4m3fn).view(torch.uint8).reshape(shape)
    s = torch.where((~fin).any(1), torch.full_like(e, 255), e + 127).to(torch.uint8)
    return q, s.reshape(*shape[:-1], shape[-1] // BLOCK)


def mx_dequantize(q, s):
    """e4m3 bytes [..., C] and E8M0 bytes [..., C/32] -> float32 values (0xFF scale -> NaN)"""
    v = q.view(torch.float8_e4m3fn).float()
    sc = s.view(torch.float8_e8m0fnu).float()
    return (v.reshape(*v.shape[:-1], -1, BLOCK) * sc[..., None]).reshape(v.shape)


def mx_pack_weights_ref(w, O, T, I):
    """fp32 master [O][T][I] -> (wf [O][T][I], sf [O][T][I/32], wt [I][T][O], st [I][T][O/32]), flat uint8, both packs
    quantised from the master"""
    w3 = w.float().reshape(O, T, I)
    wf, sf = mx_quantize_ref(w3)
    wt, st = mx_quantize_ref(w3.permute(2, 1, 0).contiguous())
    return wf.reshape(-1), sf.reshape(-1), wt.reshape(-1), st.reshape(-1)
