"""'mxfp8' compute mode without a GPU: the command line and the runtime accept it, and the reference quantiser of the MX rule
(tests/mx_ref.py, which the GPU tests hold the kernels to) gives the hand-worked results."""
import pytest
import torch

from conftest import PKG  # noqa: F401  (puts the package on sys.path)
from mx_ref import mx_dequantize, mx_exp, mx_pack_weights_ref, mx_quantize_ref


def test_train_parser_accepts_mxfp8():
    import train1
    a = train1.build_parser().parse_args(['data/none', '--dtype', 'mxfp8'])
    assert a.dtype == 'mxfp8'
    with pytest.raises(SystemExit):
        train1.build_parser().parse_args(['data/none', '--dtype', 'mx9'])


def test_set_compute_dtype_mxfp8():
    import mi355
    try:
        mi355.set_compute_dtype('mxfp8')
        assert mi355.mx_convs() and not mi355.fp8_convs() and mi355.compute_dtype() == torch.bfloat16
        mi355.set_compute_dtype('fp8')
        assert mi355.fp8_convs() and not mi355.mx_convs()
        with pytest.raises(ValueError, match='mxfp8'):
            mi355.set_compute_dtype('mxfp4')
    finally:
        mi355.set_compute_dtype('bf16')
    assert not mi355.mx_convs() and not mi355.fp8_convs()


def _block(vals):
    x = torch.zeros(32)
    x[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return x


def test_reference_quantiser_hand_worked_cases():
    cases = [  # (block values, scale byte, first element byte)
        ([448.0], 127, 0x7E),                 # amax 448 = 1.75 * 2^8: e = 0, 448 is the largest e4m3 value
        ([449.0], 128, 0x76),                 # m = 1.7539 > 1.75: e = 1, 449 / 2 = 224.5 -> 224 (0 1110 110)
        ([-1.0, 0.5], 119, 0xF8),             # amax 1: e = -8, -1 * 2^8 = -256 (1 1111 000)
        ([0.0], 0, 0x00),                     # all-zero block
        ([3.0 * 2 ** -130], 0, None),         # fp32 subnormal amax: e clamps to -127
        ([1.0, float('nan')], 255, 0x78),     # NaN in the block: 0xFF; the finite values keep the rule (1 * 2^8 = 256)
        ([float('inf'), 2.0], 255, 0x7E),     # Inf: 0xFF; e from the finite amax 2 (e = -7): Inf saturates to 448
    ]
    for vals, sbyte, q0 in cases:
        q, s = mx_quantize_ref(_block(vals))
        assert int(s[0]) == sbyte, (vals, int(s[0]))
        if vals == [-1.0, 0.5]:
            assert int(q[1]) == 0x70                                  # 0.5 * 2^8 = 128 (0 1110 000)
        if q0 is not None:
            assert int(q[0]) == q0, (vals, hex(int(q[0])))
    # the e rule itself: smallest e with amax / 2^e <= 448
    am = torch.tensor([448.0, 448.0 * 2 ** 10, 449.0, 1.0, 2 ** -126, 0.0, 3.0e38])
    assert mx_exp(am).tolist() == [0, 10, 1, -8, -127, -127, 120]


def test_reference_quantiser_dequantises_within_e4m3_rounding():
    torch.manual_seed(0)
    x = torch.randn(5, 256) * torch.exp(torch.randn(5, 256) * 4)
    q, s = mx_quantize_ref(x)
    assert q.shape == (5, 256) and s.shape == (5, 8)
    xr = mx_dequantize(q, s)
    blk = x.reshape(-1, 32).abs().amax(1, keepdim=True)
    err = (xr - x).reshape(-1, 32).abs()
    # no block saturates, and the error is within half an e4m3 step of the block's top binade (or the subnormal step)
    assert bool((err <= blk * 2.0 ** -4 + 1e-30).all())
    xb = torch.tensor([float('nan')] + [1.0] * 31)
    assert torch.isnan(mx_dequantize(*mx_quantize_ref(xb))).all()         # 0xFF scale: the whole block dequantises to NaN


def test_reference_weight_packs_are_both_from_the_master():
    torch.manual_seed(1)
    O, T, I = 64, 9, 96
    w = torch.randn(O, T, I) * torch.exp(torch.randn(O, 1, 1) * 3)
    wf, sf, wt, st = mx_pack_weights_ref(w, O, T, I)
    assert wf.numel() == wt.numel() == O * T * I and sf.numel() == O * T * I // 32 and st.numel() == O * T * I // 32
    f = mx_dequantize(wf.view(O, T, I), sf.view(O, T, I // 32))
    t = mx_dequantize(wt.view(I, T, O), st.view(I, T, O // 32)).permute(2, 1, 0)
    assert float((f - w).abs().max()) <= 2.0 ** -4 * float(w.abs().max())
    assert float((t - w).abs().max()) <= 2.0 ** -4 * float(w.abs().max())
    assert not torch.equal(f, t)            # blocks along I vs along O: different scales, so different roundings
