"""The exact-operand reference of the convolution tests (tests/conv_exact_ref.py), checked where it costs nothing: against
torch's own float64 convolutions, the range condition for every shape the GPU module runs, and the evidence that a single
missing product -- which the Gaussian tolerance tests cannot see -- breaks the exact comparison."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact_ref as R
from seeded import randn

SHAPES = [
    # N, Ci, H, W, Co, k, s, p
    (2, 8, 9, 13, 16, 3, 1, 1), (2, 8, 9, 13, 16, 3, 2, 1), (1, 16, 15, 17, 8, 4, 2, 1), (3, 8, 20, 36, 8, 7, 2, 3),
    (2, 16, 6, 5, 24, 1, 1, 0), (2, 16, 8, 8, 8, 1, 2, 0), (1, 8, 7, 9, 8, 5, 2, 2), (1, 8, 12, 10, 16, 4, 1, 2),
]


@pytest.mark.parametrize('shape', SHAPES)
def test_reference_matches_torch_in_float64(shape):
    N, Ci, H, W, Co, k, s, p = shape
    x, w = R.ints(1, N, Ci, H, W).double(), R.weights(2, Co, Ci, k, k, q=0.7).double()
    y = F.conv2d(x, w, None, stride=s, padding=p)
    assert torch.equal(R.conv_fwd(x, w, s, p), y)
    dy = R.ints(3, *y.shape).double()
    assert torch.equal(R.conv_dgrad(dy, w, s, p, (H, W)), torch.nn.grad.conv2d_input(x.shape, w, dy, stride=s, padding=p))
    assert torch.equal(R.conv_wgrad(x, dy, k, k, s, p), torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=s, padding=p))
    # fp32 arithmetic is exact on these operands too: that is what makes the kernels' fp32 accumulators order-free
    assert torch.equal(F.conv2d(x.float(), w.float(), None, stride=s, padding=p).double(), y)


def test_reference_epilogues_crop_concat_and_statistics():
    N, Ci, H, W, Co, k, s, p = 2, 8, 9, 13, 16, 4, 1, 2
    x, w = R.ints(1, N, Ci, H, W).double(), R.weights(2, Co, Ci, k, k, q=0.7).double()
    full = F.conv2d(x, w, None, stride=s, padding=p)
    crop = R.conv_fwd(x, w, s, p, out_hw=(H, W))
    assert torch.equal(crop, full[:, :, :H, :W])
    dy = R.ints(3, N, Co, H, W).double()
    wr = w.clone().requires_grad_(True)
    F.conv2d(x, wr, None, stride=s, padding=p)[:, :, :H, :W].backward(dy)
    assert torch.equal(R.conv_wgrad(x, dy, k, k, s, p), wr.grad)
    bias, res = R.ints(4, Co, lo=-8, hi=8), R.ints(5, N, Co, H, W, lo=-16, hi=16)
    assert torch.equal(R.fwd_epilogue(crop, bias, res, relu=True), F.relu(crop + bias.double().view(1, -1, 1, 1) + res.double()))
    x2, w2 = R.ints(6, N, 8, H, W), R.weights(7, Co, 8, 1, 1, q=1.0).view(Co, 8)
    x3, w3 = R.ints(1, N, Ci, H, W), R.weights(8, Co, Ci, 1, 1, q=1.0)
    cat = R.cat_fwd(x3, w3, x2, w2, 1, 0)
    assert torch.equal(cat, F.conv2d(torch.cat([x3, x2], 1).double(), torch.cat([w3, w2.view(Co, 8, 1, 1)], 1).double()))
    n, mean, m2 = R.bn_stats(crop)
    assert n == N * H * W
    assert torch.allclose(mean, crop.mean(dim=(0, 2, 3)), rtol=1e-13, atol=1e-13)
    assert torch.allclose(m2 / n, crop.var(dim=(0, 2, 3), unbiased=False), rtol=1e-12, atol=1e-12)
    # slices of the rows recombine to the same statistics (the form the kernels write them in)
    rows = crop.permute(0, 2, 3, 1).reshape(-1, Co)
    parts = []
    for sl in (rows[:100], rows[100:163], rows[163:]):
        mu = sl.mean(0)
        parts.append(torch.stack([torch.full((Co,), float(sl.shape[0]), dtype=torch.float64), mu, ((sl - mu) ** 2).sum(0)], 1))
    tot, gm, gm2 = R.fold_stats(torch.stack(parts).reshape(-1), 3, Co)
    assert torch.equal(tot, torch.full((Co,), float(n), dtype=torch.float64))
    assert torch.allclose(gm, mean, rtol=1e-13, atol=1e-13) and torch.allclose(gm2, m2, rtol=1e-12, atol=1e-9)


def test_masked_accumulate_reference_reads_the_bits_in_memory_order():
    N, C, H, W, per = 1, 16, 2, 3, 8
    mask = torch.zeros(N * H * W * C // per, dtype=torch.uint8)
    mask[3] = 0b00000101                       # NHWC elements 24 and 26: pixel (0, 1), channels 8 and 10
    bits = R.mask_bits(mask, N, C, H, W, per)
    want = torch.zeros(N, C, H, W, dtype=torch.float64)
    want[0, 8, 0, 1] = 1; want[0, 10, 0, 1] = 1
    assert torch.equal(bits, want)
    base, dx = R.ints(1, N, C, H, W, lo=-16, hi=16), R.ints(2, N, C, H, W).double()
    assert torch.equal(R.dgrad_epilogue(dx, 1.0, base, bits), dx + base.double() * want)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_range_condition_holds_for_every_gpu_case(name):
    """No case is filtered to satisfy it: a shape that broke it would need a lower weight density."""
    R.assert_case_in_range(R.build_case(name))
    R._cache.pop(name, None)                    # (the full-size case holds several hundred MB of float64)


@pytest.mark.parametrize('name', sorted(R.CAT_CASES))
def test_range_condition_holds_for_every_concat_case(name):
    c = R.build_cat_case(name)
    for dt, widths in R.CAT_C2.items():
        for n2 in widths:
            R.assert_exact_in(dt, c.y[n2], c.y_b[n2])


@pytest.mark.parametrize('name', sorted(R.PGEMM_CASES))
def test_range_condition_holds_for_every_pgemm_case(name):
    R.assert_exact_in(torch.bfloat16, *R.build_pgemm_case(name).values)


@pytest.mark.parametrize('name', sorted(R.HM_CASES))
def test_range_condition_holds_for_every_heatmap_case(name):
    R.assert_exact_in(torch.float32, R.build_hm_case(name).ref)


@pytest.mark.parametrize('form', sorted(R.GROUPED_CASES))
def test_range_condition_holds_for_every_grouped_weight_gradient(form):
    items, refs = R.build_grouped_case(form)
    assert any(r is None for r in refs) and any(it[3] is not None for it in items)      # a shared and an accumulating item
    R.assert_exact_in(torch.float32, *[r for r in refs if r is not None])


@pytest.mark.parametrize('shape', sorted(set(c for v in R.ROUNDING_CASES.values() for c in v), key=str))
def test_rounding_shapes_hold_bf16_operands_and_sums_that_round(shape):
    N, H, W, Co, _ = shape
    x, w, sums = R.rounding_case(N, H, W, Co)
    assert torch.equal(x.to(torch.bfloat16).float(), x) and torch.equal(w.to(torch.bfloat16).float(), w)
    ref = R.conv_fwd(x, w, 1, 0)
    assert set(int(v) for v in ref.unique()) == set(sums)
    R.assert_exact_in(torch.float32, ref)                                                # exact before the one rounding under test
    assert not torch.equal(R.to_dtype(ref, torch.bfloat16).double(), ref)


@pytest.mark.parametrize('name', sorted(R.FP8_CASES))
def test_range_condition_holds_for_every_fp8_case(name):
    c = R.build_fp8_case(name)
    R.assert_exact_in(torch.bfloat16, c.y, c.y_b, c.dx, c.dx_q, c.dx_acc)
    R.assert_exact_in(torch.float32, c.dw, c.dw_acc)
    # the operands themselves: integers e4m3 (activations, weights) and e5m2 (gradients) hold, so quantising cannot move them
    for t, f8 in ((c.x, torch.float8_e4m3fn), (c.w, torch.float8_e4m3fn), (c.dy, torch.float8_e5m2)):
        assert torch.equal(t.to(f8).float(), t)


def test_rounding_case_expectations_are_round_to_nearest_even():
    x, w, sums = R.rounding_case()
    y = R.conv_fwd(x, w, 1, 0)
    assert sorted(set(int(v) for v in y.reshape(-1))) == sorted(set(sums))
    got = {int(v): float(R.to_dtype(torch.tensor([float(v)], dtype=torch.float64), torch.bfloat16)) for v in sums}
    # bf16 spacing is 2 in [256, 512): odd sums are ties and go to the even multiple of 2, i.e. a multiple of 4
    assert got[257] == 256.0 and got[258] == 258.0 and got[259] == 260.0 and got[261] == 260.0 and got[383] == 384.0
    assert got[-257] == -256.0 and got[-259] == -260.0 and got[381] == 380.0


@pytest.mark.parametrize('Ci', [64, 256, 1024])
def test_one_missing_product_breaks_the_exact_comparison_and_not_the_tolerance_rule(Ci):
    """K = 576, 2304, 9216: remove one product -- the SAME tap and channel of the same output element on both sides.  Exact
    operands: the removed product is non-zero, so the bits change.  Gaussian operands under the rule of
    test_conv_fwd_dgrad_wgrad (bf16-rounded N(0, 1) activations, N(0, 1/K) weights, 1.2e-2 of max |ref|): the same mutation
    stays below the tolerance.  The index is the one whose Gaussian product has the median magnitude among the indices where the
    exact product is non-zero: a typical term, chosen without looking at either comparison."""
    N, H, W, Co, k, s, p = 1, 8, 8, 8, 3, 1, 1
    site = (0, 3, 4, 5)
    x, w = R.ints(41, N, Ci, H, W), R.weights(42, Co, Ci, k, k, q=R.density(Ci * k * k))
    xg = randn(1, N, Ci, H, W).to(torch.bfloat16).float()
    wg = randn(2, Co, Ci, k, k, scale=1.0 / np.sqrt(Ci * k * k)).to(torch.bfloat16).float()
    pe, pg = R.window_products(x, w, s, p, *site), R.window_products(xg, wg, s, p, *site)
    live = (pe != 0).nonzero().reshape(-1)
    kidx = int(live[pg[live].abs().argsort()[live.numel() // 2]])

    y = R.conv_fwd(x, w, s, p)
    mutated, removed = R.drop_one_product(y, x, w, s, p, *site, kidx)
    assert removed != 0.0
    assert R.same_bits(R.to_dtype(y, torch.bfloat16), y, torch.bfloat16)
    assert not R.same_bits(R.to_dtype(mutated, torch.bfloat16), y, torch.bfloat16)
    assert not R.same_bits(R.to_dtype(mutated, torch.float32), y, torch.float32)

    ref = F.conv2d(xg, wg, None, stride=s, padding=p)
    mut_g, removed_g = R.drop_one_product(ref.double(), xg, wg, s, p, *site, kidx)
    tol = 1.2e-2 * float(ref.abs().max())
    assert removed_g != 0.0
    assert float((mut_g.float() - ref).abs().max()) <= tol, (removed_g, tol)
    assert abs(removed_g) < 0.5 * tol
