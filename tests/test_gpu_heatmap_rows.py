"""Every form of the heat-map row kernels of csrc/heatmap.hip (hard arg-max, soft-arg-max, KL loss + gradient, pseudo-label
builders) and the small kernels beside them, each against the float64 references of tests/heatmap_ref.py.

Forms.  `row_form()` picks, per call, the register-resident kernel of the map size (1: 4096 pixels, block per map; 2: 1024,
wave per map; 3: 256, wave per map) or the loop kernel (0: any other size, any inspected pointer off a 16-byte boundary,
MI355_ROW_REG=0).  Every row test runs the same values (a) from 16-byte-aligned buffers and (b) with one inspected pointer
one float past such a boundary (`buf[1:1 + n]`), which takes the loop kernel at every size; the addresses are asserted.
Outputs sit inside larger buffers filled with a sentinel; the words in front of and behind them must survive.  Every call
is made twice on the same buffers and must give the same bits.  `test_module_under_row_reg_0` re-runs the module in a child
process with MI355_ROW_REG=0, where (a) is the loop kernel as well.

Comparisons.  arg-max idx / xy / maxval and pseudo-label gt: bit-identical to numpy / the reference (maxval: to the element
at numpy's arg-max, which np.amax equals as a value; the sign np.amax gives a zero maximum of mixed -0.0 / 0.0 depends on its
SIMD fold order -- see test_argmax_bits).  gf: bit-identical
between (a) and (b), within 2e-7 (no extra, no normalisation) or rtol 1e-5 / atol 1e-6 of the reference (the tolerances of
test_pseudo_labels_bit_exact / test_ground_false_builders_vs_oracle).  soft-arg-max and KL: per case, the bound is
16 x the error of the float32 CPU oracle against the float64 reference on that very input (test_heatmap_ref_cpu.py computes
it; nothing is typed in), at least 16 float32 ulps of the quantity's scale (2^-20 x out_scale * max(H, W); 2^-20 x
max|reference| for loss rows and gradient), at most the tolerance test_gpu_kernels.py already asks (soft-arg-max rtol 1e-4 /
atol 1e-3; loss 1e-4 and gradient 1e-3 of their maxima).  (a) against (b): the same bound.

NaN.  The float64 reference is NaN, and the assertion is on the NaN pattern instead of a distance, in: KL rows whose target
map is all zero with eps = 0 (0 / 0) and rows whose target holds a +inf pixel (loss and the whole gradient map: the softmax
term of every pixel is scaled by the sum of the normalised target) -- 14 707 of the 47 376 KL rows of the matrix, summed
over its 532 (size, rows, configuration) cases; ground-false maps that normalise = 1 divides by a zero maximum (an `extra`
of -3 over a whole image; K = 1 with kind 2, where clip(gt) - 10 gt is empty by construction).  Soft-arg-max (364 cases),
arg-max, labels without normalise = 1, bilinear, PCK and the sums have no such case.  Nothing else is excluded.

Worst kernel error per kernel, form and map size, over all row counts, configurations and both alignments, as the ratio
error / bound of the worst case, with that case's error, its float32-oracle yardstick and its bound.  Units: soft-arg-max
in output coordinates; KL loss rows and gradient as absolute values (the gradient carries the 1 / rows of the mean).
Measured on an MI355X with the library of commit 1bdd45e (this module changes no kernel), default switches.

form size     | soft-arg-max: err/bound  err      yardstick bound    | KL loss rows: err/bound  err      yardstick bound    | KL gradient: err/bound  err      yardstick bound
1    64x64    | 0.070  2.19e-05 1.96e-05 3.13e-04 | 0.284  3.42e-07 7.52e-08 1.20e-06 | 0.064  3.33e-09 3.25e-09 5.21e-08
1    32x128   | 0.063  1.80e-03 1.80e-03 2.88e-02 | 0.888  5.72e-07 2.44e-08 6.44e-07 | 0.137  1.63e-08 1.39e-09 1.19e-07
1    128x32   | 0.175  9.50e-05 3.39e-05 5.43e-04 | 0.352  2.25e-07 1.38e-08 6.38e-07 | 0.069  7.78e-10 7.04e-10 1.13e-08
2    32x32    | 0.121  1.59e-05 8.23e-06 1.32e-04 | 0.344  3.53e-07 6.41e-08 1.02e-06 | 0.101  1.93e-08 1.06e-08 1.91e-07
2    16x64    | 0.171  4.39e-05 1.60e-05 2.56e-04 | 0.418  6.31e-07 9.44e-08 1.51e-06 | 0.120  1.21e-08 6.31e-09 1.01e-07
3    16x16    | 0.089  5.44e-06 2.27e-06 6.10e-05 | 0.388  2.50e-07 1.12e-08 6.43e-07 | 0.077  3.68e-08 2.28e-08 4.77e-07
3    8x32     | 0.124  3.80e-06 1.92e-06 3.07e-05 | 0.531  3.81e-07 2.35e-08 7.18e-07 | 0.182  2.64e-09 9.03e-10 1.45e-08
0    64x64    | 0.061  3.29e-05 3.39e-05 5.42e-04 | 0.383  4.61e-07 7.52e-08 1.20e-06 | 0.151  5.08e-08 2.10e-08 3.36e-07
0    32x32    | 0.121  1.59e-05 8.23e-06 1.32e-04 | 0.810  8.30e-07 6.41e-08 1.02e-06 | 0.187  3.56e-08 1.06e-08 1.91e-07
0    16x16    | 0.091  1.23e-05 8.45e-06 1.35e-04 | 0.388  2.50e-07 1.12e-08 6.43e-07 | 0.079  4.30e-09 3.39e-09 5.42e-08
0    32x128   | 0.063  1.80e-03 1.80e-03 2.88e-02 | 0.795  5.12e-07 2.44e-08 6.44e-07 | 0.137  1.63e-08 1.39e-09 1.19e-07
0    128x32   | 0.073  5.71e-05 4.89e-05 7.82e-04 | 0.725  4.63e-07 1.38e-08 6.38e-07 | 0.114  1.64e-08 8.98e-09 1.44e-07
0    16x64    | 0.068  1.04e-05 3.17e-06 1.53e-04 | 0.339  5.12e-07 9.44e-08 1.51e-06 | 0.064  1.76e-10 1.72e-10 2.75e-09
0    8x32     | 0.074  9.01e-06 3.38e-06 1.22e-04 | 0.607  4.36e-07 1.84e-08 7.18e-07 | 0.182  2.64e-09 9.03e-10 1.45e-08
0    128x128  | 0.141  7.33e-03 7.33e-03 5.18e-02 | 0.330  4.41e-07 8.36e-08 1.34e-06 | 0.104  9.17e-10 5.49e-10 8.79e-09
0    8x8      | 0.108  9.24e-07 5.33e-07 8.52e-06 | 0.126  7.87e-06 2.50e-06 6.23e-05 | 0.108  4.42e-09 2.55e-09 4.09e-08
0    5x7      | 0.116  1.93e-06 9.75e-07 1.67e-05 | 0.143  9.18e-08 3.22e-08 6.40e-07 | 0.177  3.10e-08 1.10e-08 1.75e-07
0    10x12    | 0.152  4.34e-06 9.54e-07 2.86e-05 | 0.777  3.89e-07 3.13e-08 5.01e-07 | 0.145  9.16e-09 3.96e-09 6.34e-08
0    1x1      | 0.000  0.00e+00 0.00e+00 3.81e-06 | 0.000  0.00e+00 0.00e+00 0.00e+00 | 0.000  0.00e+00 0.00e+00 0.00e+00
0    1x3      | 0.135  9.63e-07 3.93e-07 7.15e-06 | 0.100  7.62e-07 1.92e-07 7.65e-06 | 0.184  9.32e-08 2.60e-08 5.06e-07
0    63x65    | 0.064  9.27e-04 9.12e-04 1.46e-02 | 0.360  6.10e-07 1.06e-07 1.69e-06 | 0.130  3.15e-09 1.51e-09 2.42e-08

No case exceeds its bound; the largest error / bound is 0.888 (KL loss rows, form 1, 32 x 128, rows = 1: a dense target on
N(0, 1) logits).  Soft-arg-max stays within 4.6 x and the KL gradient within 12 x the yardstick of their worst cases.  KL
loss rows go beyond 16 x the yardstick (up to 34 x in that same case: 5.7e-7 against 2.4e-8) and are held by the 16-ulp
floor, as specified, not by a wider factor.  The arithmetic: the row is sum(t log t) - sum(t logp), two sums of about 8 in
magnitude (log 4096 = 8.3) that cancel to a loss of 0.68; the kernel's 5.7e-7 is 0.6 ulp of those sums (ulp(8) = 9.5e-7) and
14 ulps of the loss, the float32 oracle (blocked, vectorised ATen sums) happens to land within 0.6 ulp of the loss itself.

The gradient's factor `tn_sum` (the sum of the normalised target) is 1 to rounding on every finite row, so leaving it out
moves a finite gradient by less than an ulp of its scale; what holds it in place is the +inf-target row, whose whole gradient
map must be NaN as in the oracle.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import heatmap_ref as R
from test_heatmap_ref_cpu import kl_yardstick, softargmax_yardstick

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = 'MI355_TEST_HEATMAP_ROWS_CHILD'

SENT = 0x7FA5A5A5            # a NaN as float32: an output word the kernel skipped is seen by the comparison as well
PAD = 64                     # sentinel words in front of and behind every output


def _mi():
    import mi355
    from mi355 import ops
    mi355.load()
    return mi355, ops


def form_of(HW):
    """row_form() of csrc/heatmap.hip for 16-byte-aligned pointers."""
    if os.environ.get('MI355_ROW_REG', '1').strip() in ('0', ''):
        return 0
    return {4096: 1, 1024: 2, 256: 3}.get(HW, 0)


def _place(t, dev, off=0):
    """Device copy of the CPU tensor `t` (4-byte elements) that starts `off` elements past a 16-byte boundary, inside its
    own larger allocation."""
    n = t.numel()
    buf = torch.zeros(n + 8, dtype=t.dtype, device=dev)
    v = buf[off:off + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


class Slot:
    """n output elements (int32 / float32) inside a buffer of sentinel words, `off` elements past a 16-byte boundary."""

    def __init__(self, n, dev, dtype=torch.float32, off=0):
        self.n, self.off = n, off
        self.buf = torch.full((PAD + off + n + PAD,), SENT, dtype=torch.int32, device=dev)
        self.out = self.buf[PAD + off:PAD + off + n].view(dtype)
        assert self.out.data_ptr() % 16 == 4 * off

    def bits(self):
        return self.buf[PAD + self.off:PAD + self.off + self.n].cpu().numpy().copy()

    def intact(self):
        lo, hi = self.buf[:PAD + self.off], self.buf[PAD + self.off + self.n:]
        return bool((lo == SENT).all()) and bool((hi == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def _twice(fn, slots):
    """Run `fn` twice on the same buffers: same bits both times, sentinels intact.  Returns the bits of every slot."""
    fn()
    torch.cuda.synchronize()
    first = [s.bits() for s in slots]
    fn()
    torch.cuda.synchronize()
    for s, a in zip(slots, first):
        assert np.array_equal(s.bits(), a), 'not the same bits run to run'
        assert s.intact(), 'wrote outside its output'
    return first


def _f(bits):
    return bits.view(np.float32)


def _measure(kernel, form, H, W, rows, cfg, err, yard, bnd):
    print('MEASURE %s form=%d size=%dx%d rows=%d cfg=%s err=%.4g yard=%.4g bound=%.4g' % (kernel, form, H, W, rows, cfg, err, yard, bnd))


# ------------------------------------------------------------------------------------------------------------------ arg-max
def geometry(HW, form):
    """(wave, lane, slot) of every element index of a map, by RowGeom / row_index() of the register forms and the
    `i = threadIdx.x + 256 * n` walk of the loop kernel."""
    i = np.arange(HW)
    if form == 0:
        tid = i % 256
        return tid // 64, tid % 64, i // 256
    vec, e = i // 4, i % 4
    threads = 256 if form == 1 else 64
    tid, j = vec % threads, vec // threads
    return tid // 64, tid % 64, 4 * j + e


TIE_KINDS = ['waves_lo', 'waves_hi', 'lanes_lo', 'lanes_hi', 'slots']


@functools.lru_cache(maxsize=None)
def tie_pairs(HW, form):
    """{kind: (a, b)}, a < b, two positions of one map that hold the same maximum: in two different waves (the smaller index
    in the lower / the higher wave), in two lanes of one wave (lower / higher lane), in two register slots (or two walks of
    the loop) of one thread.  Worked out from the geometry of `form`; a kind the geometry cannot have is absent."""
    wave, lane, slot = geometry(HW, form)
    rng = np.random.default_rng([17, HW, form])
    out = {}
    if HW < 2:
        return out
    for _ in range(20000):
        a, b = sorted(rng.integers(0, HW, 2).tolist())
        if a == b:
            continue
        if wave[a] != wave[b]:
            kind = 'waves_lo' if wave[a] < wave[b] else 'waves_hi'
        elif lane[a] != lane[b]:
            kind = 'lanes_lo' if lane[a] < lane[b] else 'lanes_hi'
        else:
            kind = 'slots'
        out.setdefault(kind, (a, b))
        if len(out) == len(TIE_KINDS):
            break
    return out


def test_tie_positions_cover_each_geometry():
    """Needs no device, but belongs to the arg-max matrix below: the tie positions really are where their names say, and
    every register geometry has the kinds it can have (the 64 x 64 tie of test_argmax_bit_exact_and_accuracy has both
    positions in one wave)."""
    assert set(tie_pairs(4096, 1)) == set(TIE_KINDS)
    assert set(tie_pairs(1024, 2)) == {'lanes_lo', 'lanes_hi', 'slots'}        # one wave per map
    assert set(tie_pairs(256, 3)) == {'lanes_lo', 'slots'}                      # lane = i / 4 grows with i
    assert set(tie_pairs(16384, 0)) == set(TIE_KINDS) and set(tie_pairs(64, 0)) == {'lanes_lo'}
    wave, lane, slot = geometry(4096, 1)
    a, b = 10 * 64 + 7, 40 * 64 + 3
    assert wave[a] == wave[b] == 2
    for HW, form in ((4096, 1), (1024, 2), (256, 3), (4095, 0)):
        wave, lane, slot = geometry(HW, form)
        assert len(set(zip(wave.tolist(), lane.tolist(), slot.tolist()))) == HW


def argmax_maps(H, W, rows):
    """numpy float32 [rows, 1, H, W] and the pattern name of every row."""
    HW = H * W
    rng = np.random.default_rng([19, H, W, rows])
    hm = rng.standard_normal((rows, HW)).astype(np.float32)
    pats = ['random', 'constant', 'first', 'last', 'negative', 'zero', 'zero_peak', 'negzero_peak', 'negzero_zero', 'zero_negzero', 'nan', 'nan_inf', 'inf_nan', 'neginf']
    ties = []
    for form in sorted({form_of(HW), 0}):
        for kind, ab in sorted(tie_pairs(HW, form).items()):
            ties.append(('f%d_%s' % (form, kind), ab))
    pats += ['tie_' + n for n, _ in ties] + ['nan2_' + n for n, _ in ties]
    tie = dict(ties)
    names = []
    mid = HW // 2
    for r in range(rows):
        p = pats[(r + rows) % len(pats)]
        names.append(p)
        m = hm[r]
        if p == 'constant':
            m[:] = 0.5
        elif p == 'first':
            m[0] = 9.0
        elif p == 'last':
            m[HW - 1] = 9.0
        elif p == 'negative':
            m[:] = -np.abs(m) - 0.125
        elif p == 'zero':
            m[:] = 0.0
        elif p in ('zero_peak', 'negzero_peak'):         # the maximum is a zero away from pixel 0: coordinates masked to (0, 0)
            m[:] = -np.abs(m) - 0.125
            m[mid] = 0.0 if p == 'zero_peak' else -0.0
        elif p == 'negzero_zero':
            m[:] = -0.0
            m[mid] = 0.0
        elif p == 'zero_negzero':
            m[:] = 0.0
            m[0] = -0.0
        elif p == 'nan':
            m[int(rng.integers(0, HW))] = np.nan
        elif p == 'nan_inf':
            m[mid // 2] = np.nan
            m[mid] = np.inf
        elif p == 'inf_nan':
            m[mid // 2] = np.inf
            m[mid] = np.nan
        elif p == 'neginf':
            m[:] = -np.inf
        elif p.startswith('tie_'):
            a, b = tie[p[4:]]
            m[a] = m[b] = 9.0
        elif p.startswith('nan2_'):
            a, b = tie[p[5:]]
            m[a] = m[b] = np.nan
    return hm.reshape(rows, 1, H, W), names


def _argmax(mi, d, rows, H, W, dev):
    idx, xy, mv = Slot(rows, dev, torch.int32), Slot(2 * rows, dev), Slot(rows, dev)
    got = _twice(lambda: mi.call('mi355_argmax2d', mi.ptr(d), mi.ptr(idx.out), mi.ptr(xy.out), mi.ptr(mv.out), rows, H, W, mi.stream_ptr()),
                 (idx, xy, mv))
    return got


@pytest.mark.parametrize('rows', R.ROWS)
@pytest.mark.parametrize('hw', R.SIZES, ids=R.size_id)
def test_argmax_bits(gpu, hw, rows):
    mi, ops = _mi()
    H, W = hw
    hm, names = argmax_maps(H, W, rows)
    r_idx, r_xy, r_mv = R.argmax(hm)
    # maxval, bit for bit: the element numpy's arg-max points at.  np.amax returns the same VALUE (asserted), but between a
    # -0.0 and a 0.0 its sign follows the fold order of numpy's SIMD reduction, not a rule: on [-0.0, 0.0, 0.0, ...] it gave
    # 0.0 at every size here while [-0.0, ..., 0.0, ..., -0.0] gave -0.0; the first-maximum rule gives -0.0 in both.
    at_idx = np.take_along_axis(hm.reshape(rows, -1), r_idx.reshape(rows, 1).astype(np.int64), 1).reshape(-1)
    assert np.array_equal(at_idx, r_mv.reshape(-1), equal_nan=True)
    want = (r_idx.reshape(-1), r_xy.reshape(-1).view(np.int32), at_idx.view(np.int32))
    for off in (0, 1):
        got = _argmax(mi, _place(torch.from_numpy(hm), gpu, off), rows, H, W, gpu)
        for what, g, w, per in (('idx', got[0], want[0], 1), ('xy', got[1], want[1], 2), ('maxval', got[2], want[2], 1)):
            bad = np.nonzero(g != w)[0]
            assert bad.size == 0, '%s, %s: %d wrong, first in row %d (%s): got %r, numpy %r' % (
                what, 'aligned' if off == 0 else 'loop form by alignment', bad.size, bad[0] // per, names[bad[0] // per],
                _f(g)[bad[0]] if what != 'idx' else g[bad[0]], _f(w)[bad[0]] if what != 'idx' else w[bad[0]])


def test_argmax_outputs_are_optional(gpu):
    mi, ops = _mi()
    for (H, W) in ((64, 64), (32, 32), (16, 16), (10, 12)):
        rows = 7
        hm, _ = argmax_maps(H, W, rows)
        d = _place(torch.from_numpy(hm), gpu)
        full = _argmax(mi, d, rows, H, W, gpu)
        for keep in range(3):
            s = [Slot(rows, gpu, torch.int32), Slot(2 * rows, gpu), Slot(rows, gpu)]
            p = [mi.ptr(x.out) if i == keep else 0 for i, x in enumerate(s)]
            mi.call('mi355_argmax2d', mi.ptr(d), p[0], p[1], p[2], rows, H, W, mi.stream_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(s[keep].bits(), full[keep]) and s[keep].intact()
            assert all(x.untouched() for i, x in enumerate(s) if i != keep)
        i2, xy2, mv2 = ops.argmax2d(d)
        assert np.array_equal(i2.cpu().numpy().reshape(-1), full[0]) and np.array_equal(xy2.cpu().numpy().reshape(-1), _f(full[1]))


# ------------------------------------------------------------------------------------------------------------- soft-arg-max
@pytest.mark.parametrize('rows', R.ROWS)
@pytest.mark.parametrize('hw', R.SIZES, ids=R.size_id)
def test_softargmax_every_form(gpu, hw, rows):
    mi, ops = _mi()
    H, W = hw
    for beta, out_scale in R.configs_for(R.SOFT_CONFIGS, rows):
        y = softargmax_yardstick(H, W, rows, beta, out_scale)
        ref, bnd = y['ref'].view(rows, 2), y['bound'].view(rows, 2)
        got = {}
        for off in (0, 1):
            d = _place(y['hm'], gpu, off)
            uv = Slot(2 * rows, gpu)
            bits, = _twice(lambda: mi.call('mi355_softargmax', mi.ptr(d), mi.ptr(uv.out), rows, H, W, beta, out_scale, mi.stream_ptr()), (uv,))
            got[off] = torch.from_numpy(_f(bits).astype(np.float64)).view(rows, 2)
            err = (got[off] - ref).abs()
            _measure('softargmax', form_of(H * W) if off == 0 else 0, H, W, rows, 'beta=%g,scale=%g' % (beta, out_scale),
                     float(err.max()), y['yard'], float(bnd.max()))
            assert torch.isfinite(got[off]).all()
            bad = (err > bnd).nonzero()
            assert bad.numel() == 0, 'off=%d beta=%g scale=%g: row %d (pattern %d) is %s, float64 %s, bound %g, float32 oracle off by %g' % (
                off, beta, out_scale, int(bad[0, 0]), (int(bad[0, 0]) + rows) % R.SOFT_PATTERNS, got[off][bad[0, 0]].tolist(),
                ref[bad[0, 0]].tolist(), float(bnd[bad[0, 0], bad[0, 1]]), y['yard'])
        assert bool(((got[0] - got[1]).abs() <= bnd).all())
        if (beta, out_scale) == (100.0, 4.0):
            u = ops.softargmax(y['hm'].to(gpu))                    # the wrapper: same call, same bits as (a)
            assert torch.equal(u.cpu().view(rows, 2).double(), got[0])


# ------------------------------------------------------------------------------------------------------------------------ KL
def _kl_check(tag, got_rows, got_grad, y, rows, H, W, form, cfg):
    ref_rows, ref_grad, nan = y['ref_rows'], y['ref_grad'].view(rows, -1), y['nan_rows']
    assert torch.equal(torch.isnan(got_rows), nan), '%s: NaN loss rows %s, the oracle has %s' % (
        tag, torch.isnan(got_rows).nonzero().view(-1).tolist()[:8], nan.nonzero().view(-1).tolist()[:8])
    gn = torch.isnan(got_grad)
    assert torch.equal(gn.all(1), nan) and torch.equal(gn.any(1), nan), tag + ': NaN pattern of the gradient'
    ok = ~nan
    assert torch.isfinite(got_rows[ok]).all() and torch.isfinite(got_grad[ok]).all()
    if not bool(ok.any()):
        return
    e_rows = float((got_rows[ok] - ref_rows[ok]).abs().max())
    e_grad = float((got_grad[ok] - ref_grad[ok]).abs().max())
    _measure('kl_loss', form, H, W, rows, cfg, e_rows, y['yard_rows'], y['bound_rows'])
    _measure('kl_grad', form, H, W, rows, cfg, e_grad, y['yard_grad'], y['bound_grad'])
    assert e_rows <= y['bound_rows'], '%s: loss rows off by %g (scale %g), bound %g, float32 oracle off by %g' % (
        tag, e_rows, y['scale_rows'], y['bound_rows'], y['yard_rows'])
    assert e_grad <= y['bound_grad'], '%s: gradient off by %g (scale %g), bound %g, float32 oracle off by %g' % (
        tag, e_grad, y['scale_grad'], y['bound_grad'], y['yard_grad'])
    # the reduced loss the training step logs: mean of the rows, 1e-4 relative as test_kl_heatmap_vs_oracle
    if not bool(nan.any()):
        assert abs(float(got_rows.mean()) - float(ref_rows.mean())) <= 1e-4 * abs(float(ref_rows.mean()))


@pytest.mark.parametrize('rows', R.ROWS)
@pytest.mark.parametrize('hw', R.SIZES, ids=R.size_id)
def test_kl_every_form(gpu, hw, rows):
    mi, ops = _mi()
    H, W = hw
    HW = H * W
    for eps, wmode, coeff in R.configs_for(R.KL_CONFIGS, rows):
        y = kl_yardstick(H, W, rows, eps, wmode, coeff)
        cfg = 'eps=%g,w=%s,coeff=%g' % (eps, wmode, coeff)
        w = None if y['weight'] is None else y['weight'].view(rows).to(gpu)
        got = {}
        # each pointer row_form() inspects is in turn the only one off a 16-byte boundary
        for mis in ('none', 'pred', 'target', 'unit_grad'):
            p = _place(y['pred'], gpu, int(mis == 'pred'))
            t = _place(y['target'], gpu, int(mis == 'target'))
            lr, g = Slot(rows, gpu), Slot(rows * HW, gpu, off=int(mis == 'unit_grad'))
            b_rows, b_grad = _twice(lambda: mi.call('mi355_kl_heatmap', mi.ptr(p), mi.ptr(t), mi.ptr(w), eps, mi.ptr(lr.out), mi.ptr(g.out),
                                                    rows, HW, coeff / rows, mi.stream_ptr()), (lr, g))
            got[mis] = (torch.from_numpy(_f(b_rows).astype(np.float64)), torch.from_numpy(_f(b_grad)).double().view(rows, HW))
            _kl_check('%s, misaligned: %s' % (cfg, mis), got[mis][0], got[mis][1], y, rows, H, W, form_of(HW) if mis == 'none' else 0, cfg)
            if mis in ('none', 'pred'):
                # want_grad False: no gradient pointer, the same loss bits
                lr2 = Slot(rows, gpu)
                mi.call('mi355_kl_heatmap', mi.ptr(p), mi.ptr(t), mi.ptr(w), eps, mi.ptr(lr2.out), 0, rows, HW, coeff / rows, mi.stream_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(lr2.bits(), b_rows) and lr2.intact()
        ok = ~y['nan_rows']
        for mis in ('pred', 'target', 'unit_grad'):
            if bool(ok.any()):
                assert float((got[mis][0][ok] - got['none'][0][ok]).abs().max()) <= y['bound_rows']
                assert float((got[mis][1][ok] - got['none'][1][ok]).abs().max()) <= y['bound_grad']
        # the three loop-form runs are one kernel on the same values
        assert torch.equal(got['pred'][0][ok], got['target'][0][ok]) and torch.equal(got['pred'][1][ok], got['unit_grad'][1][ok])
        if rows <= 63:
            r2, g2 = ops.kl_heatmap(y['pred'].to(gpu), y['target'].to(gpu), None if w is None else w.view(rows, 1), eps, True, coeff)
            r3, g3 = ops.kl_heatmap(y['pred'].to(gpu), y['target'].to(gpu), None if w is None else w.view(rows, 1), eps, False, coeff)
            assert g3 is None and torch.equal(r2.view(torch.int32), r3.view(torch.int32))
            assert torch.equal(r2.cpu().view(-1).double()[ok], got['none'][0][ok]) and torch.equal(g2.cpu().view(rows, HW).double()[ok], got['none'][1][ok])


# -------------------------------------------------------------------------------------------------------------- pseudo labels
# (S, tmp_size, div, kind): what build_training makes at heat-map sizes 128 / 64 / 32 (PseudoLabelGenerator kind 0 and
# RegressionDisparityx6 kind 2 at S, x5 at S / 2, x1 at S / 4), the supervised targets of utils/labels.py (kind 1, gt only,
# at S), and radius 0 / 6 at sizes where the model has another
LABEL_CASES = [(128, 6, 1, 0), (128, 6, 1, 2), (128, 6, 1, 1), (64, 6, 1, 0), (64, 6, 1, 2), (64, 6, 1, 1), (64, 4, 2, 1),
               (32, 6, 1, 0), (32, 6, 1, 2), (32, 4, 2, 1), (32, 3.0, 4, 1), (16, 4, 2, 1), (16, 3.0, 4, 1), (8, 3.0, 4, 1),
               (64, 0, 1, 2), (32, 0, 2, 1), (16, 0, 1, 0), (16, 6, 1, 2), (8, 6, 2, 0)]
LABEL_BK = [(3, 1), (2, 21), (1, 64)]


def label_centres(B, K, S, div):
    """float32 [B, K, 2] integer arg-max coordinates in [0, S * div): every corner and border, three key points on one
    pixel, the rest random."""
    rng = np.random.default_rng([23, B, K, S, div])
    top = S * div - 1
    mid = top // 2
    special = [(0, 0), (top, top), (top, 0), (0, top), (mid, 0), (0, mid), (top, mid), (mid, top), (mid, mid), (mid, mid), (mid, mid)]
    xy = rng.integers(0, top + 1, (B, K, 2)).astype(np.float32)
    for b in range(B):
        for k in range(min(K, len(special))):
            xy[b, k] = special[(k + 3 * b) % len(special)]
    return xy


@pytest.mark.parametrize('bk', LABEL_BK, ids=lambda bk: 'B%dK%d' % bk)
@pytest.mark.parametrize('case', LABEL_CASES, ids=lambda c: 'S%d_r%d_div%d_kind%d' % (c[0], int(c[1]), c[2], c[3]))
def test_pseudo_labels_every_form(gpu, case, bk):
    mi, ops = _mi()
    S, tmp, div, kind = case
    B, K = bk
    n = B * K * S * S
    xy = label_centres(B, K, S, div)
    xy_d = torch.from_numpy(xy).to(gpu)
    patch_d = torch.from_numpy(R.patch(tmp, 2).reshape(-1)).to(gpu)
    rng = np.random.default_rng([29, S, K])
    rand = (rng.standard_normal((B, K, S, S)) * 0.3).astype(np.float32)
    empty = rand.copy()
    empty[0] = -3.0                                        # empties every ground-false map of image 0
    # (extra, normalise, want_gt, want_gf)
    combos = [(None, 0, True, True), (rand, 0, True, True), (rand, 0, True, False), (empty, 2, False, True)]
    if kind != 0:                                          # (the model normalises kinds 1 and 2 only)
        combos += [(None, 1, False, True), (rand, 1, True, True), (empty, 1, False, True), (None, 2, True, True)]
    for extra, norm, want_gt, want_gf in combos:
        r_gt, r_gf = R.labels(xy, tmp, 2, div, S, kind, extra, norm)
        tag = 'extra=%s normalise=%d gt=%d gf=%d' % ('none' if extra is None else 'rand' if extra is rand else 'empty', norm, want_gt, want_gf)
        if norm != 1:
            assert np.isfinite(r_gf).all()
        if extra is empty:
            assert (np.isnan(r_gf[0]).all() if norm == 1 else (r_gf[0] == 0).all()), tag
        first = None
        for mis in ['none'] + (['extra'] if extra is not None and want_gf else []) + (['gt'] if want_gt else []) + (['gf'] if want_gf else []):
            ex = None if extra is None else _place(torch.from_numpy(extra), gpu, int(mis == 'extra'))
            gt, gf = Slot(n, gpu, off=int(mis == 'gt')), Slot(n, gpu, off=int(mis == 'gf'))
            b_gt, b_gf = _twice(lambda: mi.call('mi355_pseudo_label', mi.ptr(xy_d), mi.ptr(patch_d), int(tmp), div, S, kind, mi.ptr(ex), norm,
                                                mi.ptr(gt.out) if want_gt else 0, mi.ptr(gf.out) if want_gf else 0, B, K, mi.stream_ptr()), (gt, gf))
            if want_gt:
                assert np.array_equal(b_gt, r_gt.reshape(-1).view(np.int32)), '%s, misaligned %s: gt is not the reference bit for bit' % (tag, mis)
            else:
                assert gt.untouched()
            if want_gf:
                g = _f(b_gf).reshape(r_gf.shape).astype(np.float64)
                assert np.array_equal(np.isnan(g), np.isnan(r_gf)), '%s, misaligned %s: NaN maps' % (tag, mis)
                tol = dict(rtol=0, atol=2e-7) if (extra is None and norm == 0) else dict(rtol=1e-5, atol=1e-6)
                np.testing.assert_allclose(g, r_gf, err_msg='%s, misaligned %s' % (tag, mis), **tol)
                if first is None:
                    first = b_gf
                assert np.array_equal(b_gf, first), '%s: gf differs between the aligned call and the one with %s misaligned' % (tag, mis)
            else:
                assert gf.untouched()
    # the wrapper allocates its own outputs: the same bits as the aligned call
    gt_w, gf_w = ops.pseudo_label(xy_d, patch_d, int(tmp), div, S, kind)
    r_gt, r_gf = R.labels(xy, tmp, 2, div, S, kind)
    assert np.array_equal(gt_w.cpu().numpy(), r_gt)
    np.testing.assert_allclose(gf_w.cpu().numpy().astype(np.float64), r_gf, rtol=0, atol=2e-7)


# ------------------------------------------------------------------------------------------------------------ smaller kernels
def _ulps(a, b):
    """distance in float32 ulps between two arrays of non-negative finite float32 values"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize('rows', [1, 255, 256, 257, 64 * 21])
@pytest.mark.parametrize('norm', [(6.4, 6.4), (6.4, 3.2), (1.6, 12.8)], ids=lambda n: 'n%gx%g' % n)
def test_pck_dists(gpu, rows, norm):
    mi, ops = _mi()
    nx, ny = norm
    rng = np.random.default_rng([31, rows])
    pred = rng.integers(0, 64, (rows, 1, 2)).astype(np.float32)
    tgt = rng.integers(2, 64, (rows, 1, 2)).astype(np.float32)
    one, above, below = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)), np.nextafter(np.float32(1.0), np.float32(0.0))
    edge = [(one, one), (above, above), (below, below), (above, one), (one, above), (5.0, below), (above, 7.0), (0.0, 0.0), (5.0, 1.0), (1.0, 5.0)]
    for r in range(rows):
        if (r + rows) % 3 == 0:
            tgt[r, 0] = edge[((r + rows) // 3) % len(edge)]
    ref = R.pck(pred, tgt, nx, ny)
    assert ref.shape == (rows, 1)
    ref32 = ref.astype(np.float32).reshape(-1)
    d = Slot(rows, gpu)
    _p, _t = torch.from_numpy(pred).to(gpu), torch.from_numpy(tgt).to(gpu)
    bits, = _twice(lambda: mi.call('mi355_pck_dists', mi.ptr(_p), mi.ptr(_t), mi.ptr(d.out), rows, nx, ny, mi.stream_ptr()), (d,))
    got = _f(bits)
    off = ref32 == -1
    assert np.array_equal(got == -1, off), 'which rows are -1 (target not above 1 in both coordinates)'
    if rows >= 255:
        assert off.any() and (~off).any()
    assert (_ulps(got[~off], ref32[~off]) <= 1).all()
    w = ops.pck_dists(_p, _t, nx, ny)
    assert w.shape == (rows, 1) and np.array_equal(w.cpu().numpy().reshape(-1).view(np.int32), bits)


BILINEAR = [(16, 64), (32, 64), (16, 32), (8, 32), (32, 128), (64, 128), (64, 64), (10, 64), (64, 32)]


@pytest.mark.parametrize('hs', BILINEAR, ids=lambda p: '%dto%d' % p)
def test_bilinear_up(gpu, hs):
    mi, ops = _mi()
    h, size = hs
    B, K = 2, 5
    rng = np.random.default_rng([37, h, size])
    x = torch.from_numpy(rng.standard_normal((B, K, h, h)).astype(np.float32))
    acc = torch.from_numpy(rng.standard_normal((B, K, size, size)).astype(np.float32))
    tol = dict(rtol=1e-5, atol=1e-5)
    for alpha in (1.0, 0.5, -1.75):
        y = ops.bilinear_up(x.to(gpu), size, alpha)
        assert torch.allclose(y.cpu().double(), R.bilinear(x, size, alpha), **tol)
        out = acc.clone().to(gpu)
        y2 = ops.bilinear_up(x.to(gpu), size, alpha, out=out)
        assert y2.data_ptr() == out.data_ptr()
        assert torch.allclose(out.cpu().double(), R.bilinear(x, size, alpha, out=acc), **tol)
    # the C ABI takes h, w, H, W on their own: a non-square map into a guarded buffer, plain and accumulated
    h2, w2, H2, W2, rows = h, max(1, h // 2 + 1), size, size // 2 + 3, 3
    x2 = torch.from_numpy(rng.standard_normal((rows, 1, h2, w2)).astype(np.float32))
    o = Slot(rows * H2 * W2, gpu)
    xd = x2.to(gpu)
    bits, = _twice(lambda: mi.call('mi355_bilinear_up', mi.ptr(xd), mi.ptr(o.out), rows, h2, w2, H2, W2, 1.0, 0, mi.stream_ptr()), (o,))
    assert torch.allclose(torch.from_numpy(_f(bits)).double().view(rows, 1, H2, W2), R.bilinear(x2, (H2, W2)), **tol)
    mi.call('mi355_bilinear_up', mi.ptr(xd), mi.ptr(o.out), rows, h2, w2, H2, W2, 0.5, 1, mi.stream_ptr())
    torch.cuda.synchronize()
    assert o.intact()
    assert torch.allclose(torch.from_numpy(_f(o.bits())).double().view(rows, 1, H2, W2), 1.5 * R.bilinear(x2, (H2, W2)), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('n', [1, 63, 256, 257, 64 * 21])
def test_reduce_sum_and_scale_by_dev(gpu, n):
    mi, ops = _mi()
    rng = np.random.default_rng([41, n])
    v = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    for scale in (1.0, 1.0 / 1344):
        s = ops.reduce_sum(v.to(gpu), scale)
        ref = float(v.double().sum()) * R.f32(scale)
        # 16 float32 ulps of the sum of magnitudes: any fold order of n float32 addends stays far inside
        assert abs(float(s) - ref) <= 2.0 ** -20 * float(v.double().abs().sum()) * scale
    o = Slot(1, gpu)
    vd = v.to(gpu)
    bits, = _twice(lambda: mi.call('mi355_reduce_sum', mi.ptr(vd), mi.ptr(o.out), n, 1.0, mi.stream_ptr()), (o,))
    assert _f(bits)[0] == float(ops.reduce_sum(vd))
    k = torch.tensor(-3.3, device=gpu)
    out = ops.scale_by_dev(vd, k)
    assert torch.equal(out.cpu(), v * k.cpu())                    # one float32 product per element: exact
    o = Slot(n, gpu)
    bits, = _twice(lambda: mi.call('mi355_scale_by_dev', mi.ptr(vd), mi.ptr(k), mi.ptr(o.out), n, mi.stream_ptr()), (o,))
    assert np.array_equal(_f(bits), (v * k.cpu()).numpy())


@pytest.mark.parametrize('layout', ['contiguous', 'channels_last'])
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_scale_feature(gpu, dt, layout):
    mi, ops = _mi()
    dtype = torch.float32 if dt == 'f32' else torch.bfloat16
    per = 4 if dt == 'f32' else 8
    rng = np.random.default_rng([43, per])
    k = torch.tensor(0.37, device=gpu)
    for shape in [(1, per, 1, 1), (2, 24, 5, 3), (3, 64, 16, 16), (64, 256, 8, 8)]:
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dtype)
        if layout == 'channels_last':
            x = x.contiguous(memory_format=torch.channels_last)
        y = ops.scale_feature(x.to(gpu), k)
        assert y.dtype == dtype and y.stride() == x.stride()
        ref = (x.float() * k.cpu()).to(dtype)                     # float32 product, one rounding to the storage type
        assert torch.equal(y.cpu(), ref), shape
    # element counts that do not fill 16-byte chunks are refused, by the wrapper and by the library
    x = torch.zeros(per + 1, dtype=dtype, device=gpu)
    with pytest.raises(mi.Mi355Error):
        ops.scale_feature(x, k)
    o = Slot(8, gpu)
    for n in (per + 1, per - 1, 2 * per + per // 2):
        with pytest.raises(mi.Mi355Error):
            mi.call('mi355_scale_feature', mi.ptr(x), mi.ptr(k), mi.ptr(o.out), n, mi.dtype_code(dtype), mi.stream_ptr())
    with pytest.raises(mi.Mi355Error):
        mi.call('mi355_scale_feature', mi.ptr(x), mi.ptr(k), mi.ptr(o.out), per, 7, mi.stream_ptr())
    torch.cuda.synchronize()
    assert o.untouched()


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (2, 21, 64, 64), (3, 5, 5, 7), (64, 21, 16, 16), (2, 64, 63, 65)])
def test_hm_rowsum(gpu, shape):
    mi, ops = _mi()
    N, K, H, W = shape
    rng = np.random.default_rng([47, N, K, H])
    y = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    start = torch.from_numpy(rng.standard_normal(K).astype(np.float32))
    ref = y.double().sum((0, 2, 3))
    mag = y.double().abs().sum((0, 2, 3))
    o = Slot(K, gpu)
    yd = y.to(gpu)
    ops.hm_rowsum(yd, o.out, False)
    torch.cuda.synchronize()
    a = torch.from_numpy(_f(o.bits())).double()
    assert o.intact() and bool(((a - ref).abs() <= 2.0 ** -20 * mag).all())
    o.out.copy_(start)
    ops.hm_rowsum(yd, o.out, True)
    torch.cuda.synchronize()
    b = torch.from_numpy(_f(o.bits())).double()
    assert o.intact() and bool(((b - (ref + start.double())).abs() <= 2.0 ** -20 * (mag + start.double().abs())).all())


# ----------------------------------------------------------------------------------------------------------------- the switch
def test_module_under_row_reg_0(gpu):
    """MI355_ROW_REG is read once per process: this whole module again in a child with the register forms switched off."""
    if os.environ.get(CHILD):
        pytest.skip('this is the child')
    e = dict(os.environ, MI355_ROW_REG='0')
    e[CHILD] = '1'
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-m', 'gpu', '-k', 'not test_module_under_row_reg_0'],
                       capture_output=True, text=True, env=e, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout and 'skipped' not in r.stdout, r.stdout[-2000:]
