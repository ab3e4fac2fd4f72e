"""CPU checks of tests/mt_ref.py, the numpy restatement the GPU tests of the mean-teacher kernels compare against: its fold
equals torch's `_fold_scale_shift` expressions and the multiply bit for bit, its mt_loss equals the reference's live function
(tests/golden/g12_mt.npz, written by tests/golden/make_golden_mt.py)."""
import numpy as np
import pytest
import torch

from conftest import golden
import mt_ref


def _torch_fold(w, gamma, beta, mean, var, cbias, eps, axis, exact_sqrt=False):
    """The expressions of mi355/nn.py (_fold_scale_shift, then `wm * scale.view(...)`), on CPU tensors.  exact_sqrt: the square
    root through float64 (correctly rounded to fp32, as the double has more than 2 * 24 + 2 bits) instead of torch.sqrt."""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float32))
    w, gamma, beta, mean, var, cbias = (t(a) for a in (w, gamma, beta, mean, var, cbias))
    x = var.float() + eps
    root = torch.sqrt(x.double()).float() if exact_sqrt else torch.sqrt(x)
    scale = gamma.float() / root
    shift = beta.float() - mean.float() * scale
    if cbias is not None:
        shift = shift + cbias.float() * scale
    out = w * (scale.view(-1, 1, 1) if axis == 0 else scale.view(1, 1, -1))
    return out.numpy(), shift.numpy(), (torch.sqrt(x) != torch.sqrt(x.double()).float()).numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('axis', [0, 1])
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('shape', [(1, 1, 1), (5, 9, 3), (4, 16, 7), (64, 1, 64), (33, 31, 1)])
def test_fold_restatement_equals_torch_bit_for_bit(shape, bias, axis):
    O, T, I = shape
    C = O if axis == 0 else I
    rng = np.random.default_rng(O * 100 + T * 10 + I + axis)
    w = rng.standard_normal(shape).astype(np.float32)
    gamma = rng.standard_normal(C).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    mean = rng.standard_normal(C).astype(np.float32)
    var = (rng.random(C) * 2).astype(np.float32)
    var[0] = 0.0                                   # var = 0: the scale is gamma / sqrt(eps)
    gamma[C // 2] = 0.0                            # gamma = 0 (C = 1: this replaces nothing the var = 0 case needs)
    if C > 2:
        gamma[1] = -abs(gamma[1]) - 0.5            # negative gamma
    cb = rng.standard_normal(C).astype(np.float32) if bias else None
    for eps in (1e-5, 1e-3):
        got = mt_ref.fold(w, gamma, beta, mean, var, cb, eps, axis)
        # every operation of the torch expressions is one correctly rounded fp32 operation -- except that the CPU torch.sqrt of
        # some builds is off by an ulp on about one input in 200 (the kernel's, like numpy's, is correctly rounded).  So: bit for
        # bit against the expressions with the root taken through float64, and bit for bit against the expressions as they
        # stand on every channel whose torch.sqrt is the correctly rounded one.
        want = _torch_fold(w, gamma, beta, mean, var, cb, eps, axis, exact_sqrt=True)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
        live = _torch_fold(w, gamma, beta, mean, var, cb, eps, axis)
        ok = ~live[2]
        print('channels whose torch.sqrt is not correctly rounded: %d of %d' % (int(live[2].sum()), C))
        sel = (lambda a: a[ok]) if axis == 0 else (lambda a: a[:, :, ok])
        assert _same(sel(got[0]), sel(live[0])) and _same(got[1][ok], live[1][ok])


def test_fold_is_not_an_fma():
    """The restatement rounds the products on their own: a fused beta - mean * scale differs somewhere on 4096 random channels."""
    rng = np.random.default_rng(7)
    C = 4096
    gamma, beta, mean = (rng.standard_normal(C).astype(np.float32) for _ in range(3))
    var = (rng.random(C) + 0.1).astype(np.float32)
    _, shift = mt_ref.fold(np.ones((C, 1, 1), np.float32), gamma, beta, mean, var, None, 1e-5, 0)
    scale = gamma / np.sqrt(var + np.float32(1e-5))
    fused = (beta.astype(np.float64) - mean.astype(np.float64) * scale.astype(np.float64)).astype(np.float32)
    assert (fused != shift).any()


@pytest.mark.parametrize('case', ['a', 'b'])
@pytest.mark.parametrize('k', mt_ref.GOLDEN_KS)
def test_mt_loss_restatement_equals_the_reference(case, k):
    g = golden('g12_mt')
    pre, label = g[case + '/pre'], g[case + '/label']
    assert pre.shape[:2] == (2, 21) and pre.shape[2:] in ((8, 8), (5, 7))
    want = float(g['%s/loss_%d' % (case, k)])
    want_g, joints = mt_ref.golden_grad(g, case, k)
    assert joints == mt_ref.subset(k)                  # the channels the reference's gradient touches: the restated curriculum
    # torch's fp32 MSELoss is within a few ulp of the float64 value at these sizes (at most 2688 terms of like magnitude)
    assert abs(mt_ref.mt_loss64(pre, label, k) - want) <= 8 * np.spacing(np.float32(want))
    g64 = mt_ref.mt_grad64(pre, label, k)
    assert np.all(np.abs(g64 - want_g) <= 2 * np.spacing(np.abs(want_g).astype(np.float32)))
    off = [j for j in range(21) if j not in mt_ref.subset(k)]
    assert not want_g[:, off].any() and (not off or want_g[:, list(mt_ref.subset(k))].any())
    # the kernel's fp32 gradient expression: within 1 ulp of torch's (which rounds 2 / n and the product in another order)
    ug = mt_ref.unit_grad(pre, label, mt_ref.mask(k), mt_ref.grad_scale(1.0, pre.shape, k))
    assert np.all(np.abs(ug.astype(np.float64) - want_g) <= np.spacing(np.abs(want_g).astype(np.float32)))
    assert not ug[:, off].any()


def test_subset_classes():
    assert [len(mt_ref.subset(k)) for k in mt_ref.GOLDEN_KS] == [1, 1, 6, 6, 11, 11, 16, 16, 21, 21]
    assert mt_ref.mask(400) == (1 << 21) - 1 and mt_ref.mask(0) == 1
