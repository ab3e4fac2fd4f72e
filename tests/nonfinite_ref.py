"""NaN, +Inf and -Inf through the gradient-path kernels: comparison rules, the seeding helper and the float64 references.

The exact-operand suites (conv_exact_ref.py, bn_exact_ref.py, small_exact_ref.py) stay on small integers.  Here a few elements
of one operand at a time become NaN, +Inf or -Inf while every other operand keeps those integers, and the question is where the
special value comes out.  The step guard of the training loop (GradClipper, mi355_grad_clip_coef) skips an update only when a
non-finite value that arises in an image, a label, a BatchNorm statistic or a store reaches the flat gradient buffers AS a
non-finite value; the guard buffers of tests/guarded.py (0xFF fill = NaN) rely on the same propagation; and a kernel that
discards a loaded value by arithmetic (v * 0) instead of a select shows it here and nowhere else.

The class of a value is FINITE, POS_INF, NEG_INF or NAN.  Two rules:

  pointwise  (conv forward / input-gradient / weight-gradient results, BatchNorm apply outputs, dx / dres, layout and masked
             outputs): the class equals the reference's at EVERY element, and every finite element has the reference's bits
             (conv_exact_ref.same_bits' rule, zero tolerance: the finite operands are the exact integers of the parent suites,
             so a finite sum is exact in any order).
  reduced    (BatchNorm statistics partials, saved mean / invstd, running statistics, dgamma / dbeta, column sums, bias
             gradients, loss scalars, the clip record): the value is finite exactly where the float64 reference is finite, and
             the finite values meet the tolerance the exact test of that output already uses.  Where the reference is
             non-finite ANY non-finite value is accepted: the kernels sum shifted values (v - ref: Welford deviations, the
             centred second moment, Chan's merge of two slices), and Inf - Inf is NaN.  A reference +Inf that comes back as NaN
             is therefore legitimate, and so is the reverse order of two infinities of opposite sign in a tree reduction.

Why float64 tap loops are a reference for classes: IEEE arithmetic propagates the specials whatever the summation order as long
as no finite partial sum overflows -- NaN is absorbing, a sum that holds +Inf and -Inf is NaN, a sum that holds infinities of
one sign is that infinity, Inf * 0 is NaN.  No finite operand here exceeds 16 in magnitude, so no partial sum of any order comes
near the fp32 range.  test_nonfinite_cpu.py holds the loops against torch (conv2d, torch.nn.grad, batch_norm, relu,
threshold_backward) in float64 and against an indicator rule that never multiplies by a special (conv_class_rule).

The condition of every case (case_condition, asserted on the REFERENCE before a kernel result is read): at least a quarter of
the reference's elements are finite -- a kernel that floods its output with NaN must not pass -- and every class the case names
occurs.  The classes a case names are the seeded ones where the operation keeps them (convolutions without ReLU; a ReLU turns
-Inf into 0, so its outputs name NaN and +Inf), and NaN alone for BatchNorm outputs normalised by batch statistics (the mean
of a channel that holds an Inf is Inf, x - mean is NaN there and the variance with it).

Deliberate differences from torch, each tested as documented (DIVERGENCES):
  * accumulate mask and ReLU backward are selects in the kernels and in ATen's threshold_backward; the references of
    conv_exact_ref.py / bn_exact_ref.py multiply by the 0/1 mask, which is the same on integers and keeps a masked NaN.  The
    `where` variants below are the references here.
  * mi355_pseudo_label followed the reference only for a finite `extra` (fminf / fmaxf return the other operand for a NaN).
    It now clips and takes its maximum with selects, like torch.clip / torch.max: FIXED, see test_gpu_nonfinite.py.
  * the ReLU mask of a BatchNorm backward (from the stored y, recomputed from x, or the bits the forward wrote; the same in the
    conv epilogue that forms the backward's sums) was `y > 0`, which is false for a NaN output: the gradient was dropped and
    dbeta stayed finite where torch's is NaN (ATen's threshold_backward is `y <= 0 ? 0 : g`, a NaN passes).  Found by the
    block test (test_gpu_blocks.test_non_finite_values_reach_the_gradients_as_in_float64); FIXED: every source is `!(y <= 0)`.
  * mi355_pw_wgrad takes whole 64-pixel groups only, so its case runs at H x W = 192 where the other 21-channel kernels run at 120.
"""
import numpy as np
import torch

import conv_exact_ref as C

NAN, INF = float('nan'), float('inf')
SPECIAL = {'nan': NAN, '+inf': INF, '-inf': -INF}
KINDS = ('nan', '+inf', '-inf')
FINITE, POS_INF, NEG_INF, IS_NAN = 0, 1, 2, 3
CLASS_OF = {'nan': IS_NAN, '+inf': POS_INF, '-inf': NEG_INF}
CLASS_NAME = {FINITE: 'finite', POS_INF: '+inf', NEG_INF: '-inf', IS_NAN: 'nan'}

DIVERGENCES = {
    'masked accumulate / ReLU backward': 'select (kernels, ATen threshold_backward) against multiply-by-mask (the integer references): '
                                         'a masked NaN is dropped; the references here select (dgrad_epilogue_where, relu_bwd_select)',
    'pseudo_label extra': 'fixed: clip and per-map maximum are selects that keep NaN, as torch.clip / torch.max in the reference',
    'BatchNorm backward mask from a NaN y': 'fixed: the mask is !(y <= 0) in every source, as ATen threshold_backward; y > 0 dropped the gradient '
                                            'of a NaN output and left dbeta finite',
}


# ---------------------------------------------------------------------------------------------- classes and the two rules
def classes(t):
    """int8 tensor of the class of every element (any float dtype, any device)."""
    t = t.detach()
    c = torch.zeros(t.shape, dtype=torch.int8, device=t.device)
    c[t == INF] = POS_INF
    c[t == -INF] = NEG_INF
    c[t != t] = IS_NAN
    return c


def class_counts(t):
    c = classes(t)
    return {k: int((c == k).sum()) for k in (FINITE, POS_INF, NEG_INF, IS_NAN)}


def case_condition(ref, kinds, what=''):
    """The cap on a case, on its float64 reference: a quarter of the elements finite, every named class present."""
    n = class_counts(ref)
    assert 4 * n[FINITE] >= ref.numel(), '%s: only %d of %d reference elements are finite' % (what, n[FINITE], ref.numel())
    for k in kinds:
        assert n[CLASS_OF[k]] > 0, '%s: the reference holds no %s (%r)' % (what, k, n)
    return n


def pointwise_mismatch(got, ref, dtype):
    """None, or what is wrong: `got` (any device / layout, logical shape of ref) against the float64 reference under the
    pointwise rule.  The expectation is ref -> fp32 -> dtype (exact for the finite integers, Inf and NaN keep their class)."""
    g = got.detach().cpu().contiguous()
    e = C.to_dtype(ref.detach().cpu(), dtype).contiguous()
    if g.dtype != dtype or g.shape != e.shape:
        return 'dtype / shape %s %s, expected %s %s' % (g.dtype, tuple(g.shape), dtype, tuple(e.shape))
    cg, ce = classes(g), classes(e)
    bad = (cg != ce).nonzero()
    if bad.numel():
        i = tuple(int(v) for v in bad[0])
        return '%d of %d elements have another class; first at %s: got %r, expected %s' % (bad.shape[0], e.numel(), i, float(g[i]), CLASS_NAME[int(ce[i])])
    iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
    fin = ce == FINITE
    bad = ((g.view(iv) != e.view(iv)) & fin).nonzero()
    if bad.numel():
        i = tuple(int(v) for v in bad[0])
        return '%d finite elements differ; first at %s: got %r, expected %r' % (bad.shape[0], i, float(g[i]), float(e[i]))
    return None


def reduced_mismatch(got, ref, rtol=0.0, atol=0.0):
    """None, or what is wrong under the reduced rule: finite exactly where the float64 reference is, the finite values within
    |got - ref| <= atol + rtol |ref| (zero: equal)."""
    g, e = got.detach().double().cpu(), ref.detach().double().cpu()
    if g.shape != e.shape:
        return 'shape %s, expected %s' % (tuple(g.shape), tuple(e.shape))
    fg, fe = torch.isfinite(g), torch.isfinite(e)
    bad = (fg != fe).nonzero()
    if bad.numel():
        i = tuple(int(v) for v in bad[0])
        return '%d of %d values are finite where the reference is not or the reverse; first at %s: got %r, reference %r' % (
            bad.shape[0], e.numel(), i, float(g[i]), float(e[i]))
    err = (g[fe] - e[fe]).abs()
    over = err > atol + rtol * e[fe].abs()
    if bool(over.any()):
        return '%d finite values off by up to %g (rtol %g, atol %g)' % (int(over.sum()), float(err.max()), rtol, atol)
    return None


# ---------------------------------------------------------------------------------------------- seeding
def seed_specials(t, positions):
    """A copy of `t` with SPECIAL[kind] at every (index tuple, kind) of `positions`."""
    out = t.clone()
    for idx, kind in positions:
        out[tuple(idx)] = SPECIAL[kind]
    return out


def cycle_kinds(indices, kinds=KINDS):
    return [(idx, kinds[i % len(kinds)]) for i, idx in enumerate(indices)]


def tile_rows(M, bms):
    """Rows of a GEMM's M space to poison, for every row-tile height of `bms`: the first and the last row of a full row tile and
    a row in the middle of the ragged last one; the first and the last row of all where that leaves fewer than three (one of
    each kind)."""
    rows = set()
    for bm in sorted(set(bms)):
        full = M // bm
        if full:
            rows.update((0, bm - 1))
        if M % bm:
            rows.add(full * bm + (M % bm) // 2)
    if len(rows) < 3:
        rows.update((0, M - 1))
    return sorted(rows)


def build_bm(label):
    """Row-tile height of a launch-log build ('g64x128 dma kg2', 'pgemm bm64 bn128 ns6', 'cat g64x64 f32')."""
    import re
    m = re.search(r'\bg(\d+)x(\d+)', label) or re.search(r'\bbm(\d+) bn(\d+)', label)
    assert m, label
    return int(m.group(1))


def wgrad_slab_rows(M, kstep, S):
    """wgrad_split (csrc/conv_plan.h) for the split count a launch label names: rows per slab, a whole number of K steps."""
    rps = -(-M // S)
    return -(-rps // kstep) * kstep


def slab_rows(M, plans):
    """One row in the middle of every slab of every (kstep, S) plan."""
    rows = set()
    for kstep, S in plans:
        rps = wgrad_slab_rows(M, kstep, S)
        assert (S - 1) * rps < M <= S * rps, (M, kstep, S, rps)
        for i in range(S):
            lo, hi = i * rps, min(M, (i + 1) * rps)
            rows.add((lo + hi) // 2)
    return sorted(rows)


def k_groups_hit(K, ktile, k_indices):
    """Which of the two K groups of a split-K build (igemm.hip, KG = 2: K tiles [0, ceil(nk / 2)) and the rest) the contracted
    indices fall into."""
    nk = -(-K // ktile)
    split = ((nk + 1) // 2) * ktile
    return set(int(k >= split) for k in k_indices)


def _pixel(row, H, W):
    return row // (H * W), (row // W) % H, row % W


# ---------------------------------------------------------------------------------------------- where-variants
def relu_keep_nan(y):
    """max(y, 0) that keeps NaN (ATen relu, the kernels' `v < 0 ? 0 : v`)."""
    return torch.where(y < 0, torch.zeros_like(y), y)


def relu_bwd_select(g, keep):
    """ATen threshold_backward: the gradient where `keep`, else an exact zero -- whatever the dropped value was."""
    return torch.where(keep, g, torch.zeros_like(g))


def dgrad_epilogue_where(dx, scale=1.0, base=None, bits=None):
    """dx * scale (+ base, or + base where the mask bit is set: a select, a base under a cleared bit contributes exactly 0)."""
    out = dx * scale
    if base is not None:
        b = base.double()
        out = out + (b if bits is None else torch.where(bits > 0, b, torch.zeros_like(b)))
    return out


def fwd_epilogue(y, bias=None, residual=None, relu=False):
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.double()
    return relu_keep_nan(y) if relu else y


# ---------------------------------------------------------------------------------------------- the indicator rule
def conv_class_rule(x, w, stride, pad, out_hw=None):
    """Classes of conv(x, w) without ever multiplying by a special: four convolutions of finite 0/1 indicator tensors.  An
    output is NaN iff its window holds a NaN under any weight, or an Inf under a zero weight, or infinities of both resulting
    signs; otherwise +-Inf iff it holds an infinity of that resulting sign."""
    x, w = x.double(), w.double()
    ind = lambda m: m.double()
    wp, wn, wz = ind(w > 0), ind(w < 0), ind(w == 0)
    one = torch.ones_like(w)
    isn, ip, im = ind(x != x), ind(x == INF), ind(x == -INF)
    cv = lambda a, b: C.conv_fwd(a, b, stride, pad, out_hw)
    nan = cv(isn, one) + cv(ip + im, wz)
    pos = cv(ip, wp) + cv(im, wn)
    neg = cv(ip, wn) + cv(im, wp)
    c = torch.zeros(nan.shape, dtype=torch.int8)
    c[(pos > 0)] = POS_INF
    c[(neg > 0)] = NEG_INF
    c[(nan > 0) | ((pos > 0) & (neg > 0))] = IS_NAN
    return c


# ---------------------------------------------------------------------------------------------- conv cases
# (mode, case name, operand).  mode: 'fwd' (+ bias + residual, without and with ReLU), 'dgrad' (plain, scaled, accumulating),
# 'macc' (masked accumulate), 'wgrad' (overwriting and accumulating).  One operand at a time carries the specials, so that a
# failure names its source.
CONV_SPECIALS = [
    ('fwd', 't64_co72', 'x'), ('fwd', 't64_co72', 'bias'), ('fwd', 't64_co72', 'res'), ('fwd', 't64_co72', 'w'),
    ('dgrad', 't64_s2', 'dy'), ('dgrad', 't64_s2', 'base'), ('macc', 't64_s2', 'base'),
    ('dgrad', 's2_3x3_odd', 'dy'), ('dgrad', 's2_3x3_odd', 'base'), ('macc', 's2_3x3_odd', 'base'),
    ('fwd', 'small7', 'x'), ('dgrad', 'small7', 'dy'), ('fwd', 'small_dgrad', 'x'), ('dgrad', 'small_dgrad', 'dy'),
    ('fwd', 'kg2_64', 'x'), ('fwd', 'kg2_64', 'w'), ('dgrad', 'kg2_64', 'dy'),
    ('wgrad', 'wkw_w8', 'x'), ('wgrad', 'wkw_w8', 'dy'), ('wgrad', 'wkw2_wo8', 'x'), ('wgrad', 'wkw2_wo8', 'dy'),
    ('wgrad', 'wgen_direct', 'x'), ('wgrad', 'wgen_direct', 'dy'), ('wgrad', 'wgen_direct', 'dw0'),
    ('fwd', 'dma_co136', 'x'), ('fwd', 'kw3_w8', 'x'), ('dgrad', 'kw3_w8', 'dy'),
    ('fwd', 't256d_m300', 'x'), ('dgrad', 't256d_m300', 'dy'),
]


def special_id(s):
    return '-'.join(s)


def _bms(name, column):
    return [build_bm(C.EXPECT[name][i][column]) for i in (0, 1)]


def _in_pixel_of_out_row(row, c):
    """The input pixel under the centre tap (the tap at (pad, pad)) of output row `row` of case c."""
    N, Ci, H, W, Co, k, s, p = c.shape
    n, oy, ox = _pixel(row, c.Ho, c.Wo)
    return n, min(oy * s, H - 1), min(ox * s, W - 1)


def _out_pixel_reaching(n, iy, ix, c):
    """A dy pixel whose scatter reaches the dx pixel (n, iy, ix)."""
    N, Ci, H, W, Co, k, s, p = c.shape
    def axis(i, size):
        for t in range(k):
            if (i + p - t) % s == 0 and 0 <= (i + p - t) // s < size:
                return (i + p - t) // s
        raise AssertionError('no output reaches input coordinate %d' % i)
    return n, axis(iy, c.Ho), axis(ix, c.Wo)


def _dgrad_rows(c, bms):
    """dx pixels to poison: tile rows of the unit-stride GEMM, or of phase (0, 0) of a strided one (pixels (n, 2a, 2b))."""
    N, Ci, H, W, Co, k, s, p = c.shape
    Hp, Wp = -(-H // s), -(-W // s)
    return [(n, a * s, b * s) for n, a, b in (_pixel(r, Hp, Wp) for r in tile_rows(N * Hp * Wp, bms))]


def _channels(n, count):
    """`count` different channels out of n, the last one first (the last live column of a column tail; a contracted channel
    >= 64 wherever there are more than 64)."""
    return [(n - 1 - 5 * i) % n for i in range(count)]


def _wgrad_plans(name):
    out = []
    for i, kstep in ((0, 64), (1, 32)):
        S = int(C.EXPECT[name][i][4].split(' S')[1])
        out.append((kstep, S))
    return out


def conv_special(mode, name, operand):
    """{operands, positions, kinds, refs} of one entry of CONV_SPECIALS; refs: {what: float64 reference}."""
    c = C.build_case(name)
    N, Ci, H, W, Co, k, s, p = c.shape
    ops = dict(x=c.x, w=c.w, bias=c.bias, res=c.res, dy=c.dy, base=c.base, dw0=c.dw0)
    M = N * c.Ho * c.Wo
    if mode == 'fwd':
        rows = tile_rows(M, _bms(name, 0))
        if operand == 'x':
            idx = [(n, ch, iy, ix) for (n, iy, ix), ch in zip((_in_pixel_of_out_row(r, c) for r in rows), _channels(Ci, len(rows)))]
        elif operand == 'res':
            idx = [(n, ch, oy, ox) for (n, oy, ox), ch in zip((_pixel(r, c.Ho, c.Wo) for r in rows), _channels(Co, len(rows)))]
        elif operand == 'bias':
            idx = [(ch,) for ch in _channels(Co, 3)]
        else:       # weights: the last output channel and two more, in the first and the last tap, contracted channels at both ends
            idx = [(ch, ci, t, t) for ch, ci, t in zip(_channels(Co, 3), (Ci - 1, 0, Ci // 2), (k - 1, 0, k // 2))]
    elif mode in ('dgrad', 'macc'):
        pix = _dgrad_rows(c, _bms(name, 1) + _bms(name, 2))
        if operand == 'dy':
            idx = [_out_pixel_reaching(n, iy, ix, c) for n, iy, ix in pix]
            idx = [(n, ch, oy, ox) for (n, oy, ox), ch in zip(idx, _channels(Co, len(idx)))]
        else:
            idx = [(n, ch, iy, ix) for (n, iy, ix), ch in zip(pix, _channels(Ci, len(pix)))]
    else:
        rows = slab_rows(M, _wgrad_plans(name))
        if operand == 'dy':          # one output channel per kind: its rows of dw take the kind's classes, the others stay exact
            chs = dict(zip(KINDS, _channels(Co, 3)))
            idx = [_pixel(r, c.Ho, c.Wo) for r in rows]
            pos = [((n, chs[kd], oy, ox), kd) for (n, oy, ox), kd in zip(idx, (KINDS[i % 3] for i in range(len(idx))))]
        elif operand == 'x':
            chs = dict(zip(KINDS, _channels(Ci, 3)))
            idx = [_in_pixel_of_out_row(r, c) for r in rows]
            pos = [((n, chs[kd], iy, ix), kd) for (n, iy, ix), kd in zip(idx, (KINDS[i % 3] for i in range(len(idx))))]
        else:       # the accumulate base of the weight gradient, [Co][kh][kw][Ci]
            pos = cycle_kinds([(Co - 1, k - 1, k - 1, Ci - 1), (0, 0, 0, 0), (Co // 2, k // 2, k // 2, Ci // 2)])
    kinds = KINDS
    if mode == 'macc':
        # NaN alone, under cleared and under set bits: the channel of each position moves until its bit is what its turn asks for
        per_bits = {per: C.mask_bits(c.mask[per], N, Ci, H, W, per) for per in (4, 8)}
        pos = []
        for i, (n, ch, iy, ix) in enumerate(idx):
            want = float(i % 2)          # cleared, set, cleared, ... in BOTH mask layouts
            ch = next(q for q in ([ch] + list(range(Ci))) if all(float(b[n, q, iy, ix]) == want for b in per_bits.values()))
            pos.append(((n, ch, iy, ix), 'nan'))
        kinds = ('nan',)
    elif mode != 'wgrad':
        pos = cycle_kinds(idx)
    ops[operand] = seed_specials(ops[operand], pos)
    out = dict(case=c, mode=mode, name=name, operand=operand, positions=pos, kinds=kinds, ops=ops, refs={}, expect={})
    if mode == 'fwd':
        y = C.conv_fwd(ops['x'], ops['w'], s, p, c.out_hw)
        out['refs'] = {'fwd+bias+res': fwd_epilogue(y, ops['bias'], ops['res']), 'fwd+bias+res+relu': fwd_epilogue(y, ops['bias'], ops['res'], relu=True)}
        out['expect'] = {'fwd+bias+res': kinds, 'fwd+bias+res+relu': tuple(kd for kd in kinds if kd != '-inf')}
    elif mode == 'dgrad':
        dx = C.conv_dgrad(ops['dy'], ops['w'], s, p, (H, W))
        if operand == 'dy':
            out['refs'] = {'dgrad': dx, 'dgrad*scale': dgrad_epilogue_where(dx, 0.25)}
        out['refs']['dgrad*scale+acc'] = dgrad_epilogue_where(dx, 0.25, ops['base'])
        out['expect'] = {what: kinds for what in out['refs']}
    elif mode == 'macc':
        dx = C.conv_dgrad(ops['dy'], ops['w'], s, p, (H, W))
        out['refs'] = {'dgrad+macc/%d' % per: dgrad_epilogue_where(dx, 1.0, ops['base'], per_bits[per]) for per in (4, 8)}
        out['expect'] = {what: kinds for what in out['refs']}
        out['clean'] = {'dgrad+macc/%d' % per: c.dx_macc[per] for per in (4, 8)}
    else:
        dw = C.conv_wgrad(ops['x'], ops['dy'], k, k, s, p).permute(0, 2, 3, 1).contiguous()
        if operand != 'dw0':
            out['refs']['wgrad'] = dw
        out['refs']['wgrad+acc'] = dw + ops['dw0'].double()
        out['expect'] = {what: kinds for what in out['refs']}
    return out


# concat-K, heat-map conv and persistent GEMM: the specials in x (the SECOND operand of the concat), positions by the same rules
def cat_special(name, n2, dt_index):
    c = C.build_cat_case(name)
    N, Ci, H, W, Co, k, s, p = c.shape
    rows = tile_rows(N * c.Ho * c.Wo, [build_bm(C.CAT_EXPECT[name][dt_index])])
    pos = cycle_kinds([(n, ch, oy, ox) for (n, oy, ox), ch in zip((_pixel(r, c.Ho, c.Wo) for r in rows), _channels(n2, len(rows)))])
    x2 = seed_specials(c.x2[n2], pos)
    y = C.conv_fwd(c.x, c.w, s, p) + C.conv_fwd(x2, c.w2[n2].view(Co, n2, 1, 1), 1, 0)
    return dict(case=c, x2=x2, positions=pos, kinds=KINDS, refs={'cat': y, 'cat+bias': fwd_epilogue(y, c.b1 + c.b2)})


def hm_special(name='hm_120'):
    N, Cc, K, H, W = C.HM_CASES[name]
    c = C.build_hm_case(name)
    rows = tile_rows(N * H * W, [128])
    pos = cycle_kinds([(n, ch, iy, ix) for (n, iy, ix), ch in zip((_pixel(r, H, W) for r in rows), _channels(Cc, len(rows)))])
    x = seed_specials(c.x, pos)
    return dict(case=c, x=x, positions=pos, kinds=KINDS, refs={'hm': fwd_epilogue(C.conv_fwd(x, c.w, 1, 0), c.b)})


PGEMM_SPECIALS = [('pg_k128', 'x'), ('pg_k128', 'res'), ('pg_co72', 'x'), ('pg_co72', 'res')]


def pgemm_special(name, operand):
    c = C.build_pgemm_case(name)
    N, Ci, H, W, Co = c.shape
    rows = tile_rows(N * H * W, [build_bm(C.PGEMM_EXPECT[name][0][0])])
    nch = Ci if operand == 'x' else Co
    pos = cycle_kinds([(n, ch, iy, ix) for (n, iy, ix), ch in zip((_pixel(r, H, W) for r in rows), _channels(nch, len(rows)))])
    ops = dict(x=c.x, res=c.res)
    ops[operand] = seed_specials(ops[operand], pos)
    y = C.conv_fwd(ops['x'], c.w, 1, 0)
    refs = {'fwd': y, 'fwd+relu': fwd_epilogue(y, relu=True), 'fwd+bias+res': fwd_epilogue(y, c.bias, ops['res']),
            'fwd+bias+res+relu': fwd_epilogue(y, c.bias, ops['res'], relu=True)}
    if operand == 'res':
        refs = {what: r for what, r in refs.items() if 'res' in what}
    expect = {what: tuple(kd for kd in KINDS if not (kd == '-inf' and 'relu' in what)) for what in refs}
    return dict(case=c, ops=ops, positions=pos, kinds=KINDS, refs=refs, expect=expect)


# bf16 store overflow: a 1x1 conv with zero weights whose bias carries values around the ends of the bf16 range.  The expected
# store is one round to nearest even of the fp32 value: +-3.4e38 -> +-Inf, BF16_MAX stays, 2^-133 stays a subnormal (not 0).
# The subnormal meets the fp32 epilogue only; no MFMA operand is subnormal.
def store_overflow_case():
    from small_exact_ref import BF16_MAX
    N, Ci, H, W, Co, _ = C.PGEMM_CASES['pg_co72']
    vals = [3.4e38, -3.4e38, BF16_MAX, -BF16_MAX, 2.0 ** -133, -(2.0 ** -133), 1.0, 0.0]
    bias = torch.tensor([vals[i % len(vals)] for i in range(Co)], dtype=torch.float32)
    x = C.ints(C.seed_of('store_overflow'), N, Ci, H, W)
    w = torch.zeros(Co, Ci, 1, 1)
    ref = bias.double().view(1, Co, 1, 1).expand(N, Co, H, W).contiguous()
    e = C.to_dtype(ref, torch.bfloat16)
    assert float(e[0, 0, 0, 0]) == INF and float(e[0, 1, 0, 0]) == -INF and float(e[0, 2, 0, 0]) == BF16_MAX
    assert float(e[0, 4, 0, 0]) == 2.0 ** -133 and float(e[0, 5, 0, 0]) == -(2.0 ** -133)
    return dict(shape=(N, Ci, H, W, Co), x=x, w=w, bias=bias, ref=ref)


# ---------------------------------------------------------------------------------------------- BatchNorm
def bn_bwd_select(c, keep=None, prior_dgamma=None, prior_dbeta=None):
    """bn_exact_ref.bn_bwd with the ReLU backward as a select: a masked dy contributes an exact zero, whatever it held."""
    g = c['dy'] if keep is None else relu_bwd_select(c['dy'], keep)
    xhat = (c['x'] - c['mean']) * c['invstd']
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    k0, k1, k2 = c['gamma'] * c['invstd'], s1 / c['rows'], s2 / c['rows']
    return dict(dx=k0 * (g - k1 - xhat * k2), dres=g, dbeta=s1 + (0 if prior_dbeta is None else prior_dbeta),
                dgamma=s2 + (0 if prior_dgamma is None else prior_dgamma), g=g, xhat=xhat, s1=s1, s2=s2, k0=k0, k1=k1, k2=k2)


def bn_positions(rows, C_, keep, live):
    """(row, channel) of one element per channel group where `keep` (bool [rows][C], or None: everything is live) is `live`:
    the last row of the case first, then the first, in channels C - 1 and 0."""
    out = []
    for r, ch in ((rows - 1, C_ - 1), (0, 0)):
        if keep is None:
            assert live
            out.append((r, ch))
            continue
        cand = (keep[:, ch] == live).nonzero().view(-1)
        assert cand.numel(), 'channel %d has no %s element' % (ch, 'live' if live else 'masked')
        # the candidate nearest to the wanted row
        out.append((int(cand[(cand - r).abs().argmin()]), ch))
    return out


# ---------------------------------------------------------------------------------------------- 21-channel 1x1 kernels
# B = 2, C = 64, K = 21, H x W = 10 x 12: two 64-pixel tiles per image, the second ragged (56 pixels)
PW_SHAPE = dict(N=2, C=64, K=21, HW=120)
# pixels of the three specials: the first and the last of a full 64-pixel tile (image 0), the middle of the ragged one (image 1)
PW_PIXELS = ((0, 0), (0, 63), (1, 92))
PW_OPERANDS = {'c2k': ('x', 'wkc', 'bias_k'), 'k2c': ('y', 'wck', 'bias_c', 'res'), 'wgrad': ('x', 'y', 'prior_w'), 'rowsum': ('y', 'bias_k')}


PW_WGRAD_HW = 192          # mi355_pw_wgrad takes whole 64-pixel groups only (it refuses H x W = 120): 12 x 16, three groups per image


def pw_special(dt, operand, HW=None):
    """small_exact_ref.pw_case(dt, 2, 64, 21, 120) with NaN, +Inf and -Inf in `operand`: a feature map or heat map at PW_PIXELS
    (channels: the last, the first, one in the middle), a weight matrix or a vector at its last, first and a middle element."""
    import small_exact_ref as S
    c = S.pw_case(dt, PW_SHAPE['N'], PW_SHAPE['C'], PW_SHAPE['K'], HW or PW_SHAPE['HW'])
    t = c[operand]
    W = c['W']
    if t.dim() == 4:
        chs = _channels(t.shape[1], 3)
        pos = cycle_kinds([(n, ch, px // W, px % W) for (n, px), ch in zip(PW_PIXELS, chs)])
    elif t.dim() == 2:
        pos = cycle_kinds([(t.shape[0] - 1, t.shape[1] - 1), (0, 0), (t.shape[0] // 2, t.shape[1] // 2)])
    else:
        pos = cycle_kinds([(t.shape[0] - 1,), (0,), (t.shape[0] // 2,)])
    c = dict(c)
    c[operand] = seed_specials(t, pos)
    c['positions'] = pos
    return c


# ---------------------------------------------------------------------------------------------- heat-map kernels
HM_SHAPE = (2, 21, 16, 16)
# one map per special: (image, joint, row, column, kind); every other map is clean
HM_SPECIALS = ((0, 3, 5, 7, 'nan'), (0, 20, 15, 15, '+inf'), (1, 5, 0, 0, '-inf'))


def hm_poisoned_maps():
    return [(b, k) for b, k, _, _, _ in HM_SPECIALS]


def hm_seed(t):
    return seed_specials(t, [((b, k, i, j), kd) for b, k, i, j, kd in HM_SPECIALS])


def hm_inputs(tag, scale=1.0, positive=False):
    """float32 [2, 21, 16, 16] of N(0, scale) (or uniform (0, 1) * scale) values, clean."""
    rng = np.random.default_rng([53, C.seed_of(tag)])
    v = rng.random(HM_SHAPE) if positive else rng.standard_normal(HM_SHAPE)
    return torch.from_numpy((v * scale).astype(np.float32))


# ---------------------------------------------------------------------------------------------- grouped weight gradients
def grouped_special(form='wgrad_group'):
    """conv_exact_ref.build_grouped_case(form) with NaN, +Inf and -Inf in the dy of item 0 (one output channel each: the last, the
    first, one in the middle; first, last and a middle reduction row) and in the x of item 2 (input channels, likewise).  Item 3
    of 'wgrad_group' accumulates onto item 0's gradient: a finite addend onto rows that are already special.
    -> [(shape, x, dy, dw0)], refs as build_grouped_case's."""
    items, _ = C.build_grouped_case(form)
    out, refs = [], []
    for i, (shape, x, dy, dw0) in enumerate(items):
        N, H, W, Ci, Co, k, s, p, acc, share = shape
        Ho, Wo = C.out_size(H, W, k, k, s, p)
        if i == 0:
            dy = seed_specials(dy, [((0, Co - 1, 0, 0), 'nan'), ((N - 1, 0, Ho - 1, Wo - 1), '+inf'), ((N // 2, Co // 2, Ho // 2, Wo // 2), '-inf')])
        if i == 2:
            x = seed_specials(x, [((0, Ci - 1, 0, 0), 'nan'), ((N - 1, 0, (Ho - 1) * s, (Wo - 1) * s), '+inf'), ((N // 2, Ci // 2, (Ho // 2) * s, (Wo // 2) * s), '-inf')])
        ref = C.conv_wgrad(x, dy, k, k, s, p).permute(0, 2, 3, 1).contiguous()
        if share is not None:
            refs[share] = refs[share] + ref
            ref = None
        elif acc:
            ref = ref + dw0.double()
        out.append((shape, x, dy, dw0))
        refs.append(ref)
    return out, refs
