"""Every conv GEMM build against the float64 reference BIT FOR BIT, on exact integer operands (tests/conv_exact_ref.py).

The operands are small integers for which every product and partial sum is exact in fp32 and every result exact in bf16
(the range condition, asserted on the reference before a kernel result is looked at), so a correct kernel returns the
reference's bits whatever its tile, staging, split-K or slab reduction: the tolerance is zero.  Each launch is also held to
the kernel build named in its launch-log label ("[g128x128 dma kg2 epi1]", csrc/common.h) through the expected-build tables
of conv_exact_ref.py, so a case that silently moves to another kernel when a dispatch threshold changes fails instead of
testing something else.  The tables are read from choose_conv / choose_pgemm / choose_fp8 / plan_wgrad (csrc/conv_plan.h) at
this commit, and test_conv_dispatch_cpu.py holds them against those functions without a GPU;
profiles/conv_exact_labels.txt holds the full labels of one run for diffing.

Every call runs in hostile memory (tests/guarded.py): the operands a test builds -- feature maps, packed weights, biases, masks,
accumulate bases, weight gradients, the items of a grouped call -- are copies inside 0xFF-filled guard buffers, and while a wrapper
runs, every tensor it allocates (outputs, statistics partials, fp8 / MX copies and their scale arrays) and the workspace it asks
for -- of exactly the size the library's own *_workspace function returned -- are such buffers too.  0xFF.. is a NaN in every
element type here, so a store outside a result changes a flank (checked after every call), a launch or a split that writes
nothing leaves NaN where the comparison looks (an output must have no unwritten element before it is compared: with plain
torch.empty the block of the previous, identical call would come back with the right bits in it), and a read past an operand
through a plain pointer poisons the sum it enters.  test_conv_dispatch_cpu.py holds, from the plans, that the cases include ragged
last splits, single slabs with accumulate, grouped launches with several slab-reduced items and statistics buffers with slack.

NaN, +Inf and -Inf (tests/nonfinite_ref.py, the section at the end): the guard buffers' claim that a NaN read "poisons the sum it
enters" holds only for kernels that propagate one, and the step guard of the training loop needs the same.  A few elements of one
operand at a time (x, dy, bias, residual, accumulate base, weights, the weight gradient's base) are special on the smallest case of
every build; the class of every output element must be the float64 reference's and every finite element must keep its bits.  A NaN
base under a cleared accumulate-mask bit contributes an exact zero (a select, never base * bit), the statistics and
BatchNorm-backward epilogues keep a special inside its channel, and a bf16 store rounds an fp32 value beyond the range to Inf and
keeps a subnormal.

Builds behind switches that are read once per process (MI355_DMA, MI355_KW3, MI355_PHASES, MI355_T256D_*, MI355_FP8_TILE)
run in child processes, one per entry of GROUPS, strictly one after another, each with its own timeout and no retry.

Instantiations no case reaches, and why:
  * gather 256x256 register-staged (MI355_T256 experiment switch) and the MI355_TILE-forced tiles: not dispatched by default,
    the forced tiles are the same instantiations the shapes here reach;
  * concat-K tiles behind MI355_CAT_TILE: the same instantiations are reached by shape (64x64, 64x128, 128x128) or through
    MI355_DMA=2 (LDS-DMA ring) and the forced 256x256 group;
  * pgemm at K = 1024 (named by the issue): pg_bn refuses it -- a 64-wide weight slice of more than 512 channels exceeds the 64 KB
    the kernel keeps for it -- so under mi355_set_pgemm(2) such a launch stays on the gather kernel; K = 512 is the longest K run;
  * a second full-size case for a partial column tile on the 256x128 shared-A-tile build (4096 tiles of 128x128 cost 40 GFLOP
    in the float64 reference at any channel count): its column tail is the code the 128x128 shared-A-tile build runs at Co = 136;
  * pgemm bm128 (MI355_PG_BM=128) and the ring depths only MI355_PG_RING selects (128-wide columns with a ring of 5 and no
    addend ring, 64-wide columns with a ring of 4): experiment switches, never dispatched by default;
  * the EPI = 2 (BatchNorm-backward) epilogue on the 256-row, shared-A-tile, split-K and concat-K builds: it does not exist
    (dispatch falls to a regular tile, which the 'bnb' column asserts)."""
import os
import re
import subprocess
import sys

import pytest
import torch

import conv_exact_ref as R
import guarded as G
import nonfinite_ref as NF
from mx_ref import mx_dequantize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUPS, EXPECT, CAT_EXPECT, FP8_EXPECT, ROUNDING_EXPECT, PGEMM = R.GROUPS, R.EXPECT, R.CAT_EXPECT, R.FP8_EXPECT, R.ROUNDING_EXPECT, R.PGEMM_EXPECT
GROUP = os.environ.get('MI355_CONV_EXACT_GROUP', 'default')      # set by the parent for its child processes
DT = {'bf16': torch.bfloat16, 'f32': torch.float32}


def _names(table):
    return [n for n in table if table[n][0] == GROUP]


def _ops():
    import mi355
    from mi355 import ops
    mi355.load()
    return ops


@pytest.fixture(scope='module', autouse=True)
def launch_log(gpu):
    ops = _ops()
    ops.prof_enable(1)
    yield
    ops.prof_enable(0)


@pytest.fixture(autouse=True)
def guards():
    """Every test starts and ends without guard buffers of another test (tests/guarded.py)."""
    G.reset()
    yield
    G.reset()


def _run(ops, fn):
    """fn() with the labels of the conv-family launches it made.  The call runs inside a guard window (tests/guarded.py): every
    tensor the wrapper allocates and the workspace it asks for are 0xFF-filled buffers between 0xFF flanks, and after the launch
    no flank byte -- theirs, or of any operand a test placed -- may have changed."""
    ops.prof_reset()
    with G.window(ops, 'conv call'):
        out = fn()
    torch.cuda.synchronize()
    labels = [l['label'] for l in ops.prof_launches() if l['family'] == 0]
    G.check(' | '.join(labels))
    return out, labels


def _guarded(ops, what, fn):
    """fn() in a guard window of its own: operand producers (quantisers, weight packs) and the BatchNorm launches of this module."""
    with G.window(ops, what):
        out = fn()
    torch.cuda.synchronize()
    G.check(what)
    return out


def _pitch(dtype, *channels):
    """The widest row of the case, for the flanks of its flat operands (packed weights, vectors, workspace)."""
    G.row_pitch(max(channels) * (2 if dtype == torch.bfloat16 else 4))


def _whole(what, t):
    """The launch wrote all of `t`: no element is still the guard fill (a NaN, which no reference of this module holds)."""
    assert t.data_ptr() % G.BOUNDARY == G.START, '%s: not in a guard buffer' % what          # (the allocator's own blocks start on the boundary)
    assert G.unwritten(t) == 0, '%s: %d bytes of the output were never written' % (what, G.unwritten(t))


def _build(label):
    m = re.search(r'\[([^\]]*)\]$', label)
    assert m, 'launch label without a build: %r' % label
    return m.group(1)


def _check_builds(what, labels, expect):
    """Every launch of one call ran the expected build; returns the epilogue index the launches carry (0, 1 or 2)."""
    n = 1
    if ' *' in expect:
        expect, n = expect.split(' *')[0], int(expect.split(' *')[1])
    print('\nLABEL %s %s' % (what, ' | '.join(labels)))
    assert all(l.split(' [')[0].strip() for l in labels), '%s: a launch without its layer label: %r' % (what, labels)
    builds = [_build(l) for l in labels]
    bare = [re.sub(r' epi\d$', '', b) for b in builds]
    assert bare == [expect] * n, '%s: launched %r, expected %d x [%s]' % (what, labels, n, expect)
    epis = set(int(b[-1]) if re.search(r' epi\d$', b) else 0 for b in builds)
    assert len(epis) == 1
    return epis.pop()


def _same(what, got, ref, dtype):
    _whole(what, got)
    assert R.same_bits(got, ref, dtype), '%s: %s' % (what, R.first_mismatch(got, ref, dtype))


def _dev(t, dtype, gpu):
    return G.place(_ops().to_nhwc(t.to(gpu), dtype), 'feature map')


def _vec(t, gpu, what='vector'):
    """A bias, a mask, a scale, a per-channel vector or a gradient buffer: onto the device, into a guard buffer."""
    return G.place(t.to(gpu).contiguous(), what)


def _packs(ops, *args):
    """ops.pack_weights(*args) with both packs in guard buffers."""
    return tuple(t if t is None else G.place(t, 'packed weights') for t in _guarded(ops, 'pack_weights', lambda: ops.pack_weights(*args)))


def _check_stats(what, part, C, ref, rows):
    """(n, mean, M2) slices of a statistics epilogue, folded in float64, against float64 statistics of the exact output: n exact,
    mean and 1 / sqrt(var + eps) within the tolerances of test_conv_epilogue_bn_statistics (1e-5 / 2e-5 relative, 1e-6 absolute)."""
    assert part is not None and part[1] >= 1, what
    # the slices the launch reports are written, and nothing behind them is (the buffer holds more than any launch fills)
    used = part[1] * C * 3
    assert used < part[0].numel(), what
    assert G.unwritten(part[0][:used]) == 0 and G.unwritten(part[0][used:]) == (part[0].numel() - used) * 4, what
    tot, mean, m2 = R.fold_stats(part[0], part[1], C)
    n, rmean, rm2 = R.bn_stats(ref)
    assert n == rows and torch.equal(tot, torch.full((C,), float(rows), dtype=torch.float64)), what
    inv, rinv = 1.0 / torch.sqrt(m2 / tot + 1e-5), 1.0 / torch.sqrt(rm2 / n + 1e-5)
    print('\nSTATS %s: max |mean err| %.3e (max |mean| %.3e), max rel invstd err %.3e' % (
        what, float((mean - rmean).abs().max()), float(rmean.abs().max()), float(((inv - rinv) / rinv).abs().max())))
    assert torch.allclose(mean, rmean, rtol=1e-5, atol=1e-6), what
    assert torch.allclose(inv, rinv, rtol=2e-5, atol=1e-6), what


# ---------------------------------------------------------------------------------------------- forward / dgrad / wgrad
_CONV = [(n, dt) for n in _names(R.CASES) for dt in ('bf16', 'f32')]
if _CONV:
    @pytest.mark.parametrize('name,dt', _CONV, ids=['%s-%s' % p for p in _CONV])
    def test_conv_builds_return_the_reference_bits(gpu, name, dt):
        ops = _ops()
        c = R.build_case(name)
        dtype, per = DT[dt], (8 if dt == 'bf16' else 4)
        R.assert_exact_in(dtype, *c.fwd_values)
        R.assert_exact_in(dtype, *c.dgrad_values)
        R.assert_exact_in(torch.float32, c.dw, c.dw_acc)
        e_fwd, e_dgrad, e_acc, e_bnb, e_wgrad = EXPECT[name][0 if dt == 'bf16' else 1]
        N, Ci, H, W, Co, k, s, p = c.shape
        desc = ops.make_desc(N, H, W, Ci, Co, k, k, s, p, dtype, out_hw=c.out_hw)
        _pitch(dtype, Ci, Co)
        xd, dyd = _dev(c.x, dtype, gpu), _dev(c.dy, dtype, gpu)
        wf, wt = _packs(ops, _vec(c.w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, k * k, Ci, Ci, dtype)
        bias, res = _vec(c.bias, gpu, 'bias'), _dev(c.res, dtype, gpu)
        tag = '%s/%s ' % (name, dt)

        for what, fn, ref in (('fwd', lambda: ops.conv_fwd(desc, xd, wf), c.y),
                              ('fwd+bias', lambda: ops.conv_fwd(desc, xd, wf, bias), c.y_b),
                              ('fwd+bias+res', lambda: ops.conv_fwd(desc, xd, wf, bias, res), c.y_br),
                              ('fwd+bias+res+relu', lambda: ops.conv_fwd(desc, xd, wf, bias, res, relu=True), c.y_brr)):
            y, labels = _run(ops, fn)
            assert _check_builds(tag + what, labels, e_fwd) == 0
            _same(tag + what, y, ref, dtype)
        (y, part), labels = _run(ops, lambda: ops.conv_fwd_stats(desc, xd, wf, bias))
        assert _check_builds(tag + 'fwd+stats', labels, e_fwd) == 1
        _same(tag + 'fwd+stats', y, c.y_b, dtype)
        _check_stats(tag + 'fwd+stats', part, Co, c.y_b, N * c.Ho * c.Wo)

        if c.has_dgrad:
            sc = _vec(torch.full((1,), 0.25), gpu, 'scale')
            base, mask, bias_i = _dev(c.base, dtype, gpu), _vec(c.mask[per], gpu, 'mask'), _vec(c.bias_i, gpu, 'bias')
            for what, fn, ref, exp in (
                    ('dgrad', lambda: ops.conv_dgrad(desc, dyd, wt), c.dx, e_dgrad),
                    ('dgrad*scale', lambda: ops.conv_dgrad(desc, dyd, wt, scale_dev=sc), c.dx_q, e_dgrad),
                    ('dgrad*scale+acc', lambda: ops.conv_dgrad(desc, dyd, wt, scale_dev=sc, out=G.place(base, 'base'), accumulate=True), c.dx_acc, e_acc),
                    ('dgrad+macc', lambda: ops.conv_dgrad_masked_acc(desc, dyd, wt, G.place(base, 'base'), mask), c.dx_macc[per], e_acc),
                    ('deconv+bias', lambda: ops.deconv_fwd_act(desc, dyd, wt, bias_i), c.dx_b, e_dgrad),
                    ('deconv+bias+relu', lambda: ops.deconv_fwd_act(desc, dyd, wt, bias_i, relu=True), c.dx_br, e_dgrad)):
                dx, labels = _run(ops, fn)
                assert _check_builds(tag + what, labels, exp) == 0
                _same(tag + what, dx, ref, dtype)
            (dx, part), labels = _run(ops, lambda: ops.conv_dgrad_stats(desc, dyd, wt))
            epi = _check_builds(tag + 'dgrad+stats', labels, e_dgrad)
            _same(tag + 'dgrad+stats', dx, c.dx, dtype)
            assert (epi == 1) == (part is not None)          # the statistics are fused, or refused (uneven phases), never half done
            if s == 1:
                assert epi == 1
            if part is not None:
                _check_stats(tag + 'dgrad+stats', part, Ci, c.dx, N * H * W)
            # the input gradient as the dy of a BatchNorm: exact dx, that BatchNorm's reduction partials against its own passes
            xb = _dev(c.base, dtype, gpu)
            gamma, beta = _vec(1 + c.bias_i / 64, gpu, 'gamma'), _vec(c.bias_i / 32, gpu, 'beta')
            rm, rv, nbt = _vec(torch.zeros(Ci), gpu, 'running_mean'), _vec(torch.ones(Ci), gpu, 'running_var'), _vec(torch.zeros((), dtype=torch.int64), gpu, 'num_batches_tracked')
            _, mean, invstd = _guarded(ops, 'bn_train_fwd', lambda: ops.bn_train_fwd(xb, None, gamma, beta, rm, rv, nbt, 1e-5, 0.1, False))
            _whole('mean', mean), _whole('invstd', invstd)
            bn = (xb, None, gamma, beta, mean, invstd, False)
            (dx, part), labels = _run(ops, lambda: ops.conv_dgrad_bnbwd(desc, dyd, wt, bn))
            epi = _check_builds(tag + 'dgrad+bnb', labels, e_bnb)
            _same(tag + 'dgrad+bnb', dx, c.dx, dtype)
            assert (epi == 2) == (part is not None)
            if s == 1:
                assert epi == 2
            if part is not None:
                used = part[1] * Ci * 2          # [slice][C][2] sums: the reported slices written, nothing behind them
                assert used < part[0].numel()
                assert G.unwritten(part[0][:used]) == 0 and G.unwritten(part[0][used:]) == (part[0].numel() - used) * 4
                sums = []
                for pp in (None, part):
                    dg, db = G.empty((Ci,), torch.float32, gpu, 'dgamma'), G.empty((Ci,), torch.float32, gpu, 'dbeta')
                    _guarded(ops, 'bn_bwd', lambda: ops.bn_bwd(dx, xb, None, gamma, mean, invstd, dg, db, False, False, False, beta=beta, partial=pp))
                    _whole('dgamma', dg), _whole('dbeta', db)
                    sums.append((dg, db))
                (dga, dba), (dgb, dbb) = sums
                tol = 2e-5 * (float(dga.abs().max()) + float(dba.abs().max()) + 1.0)     # as test_gemm_epilogue_bn_backward_reduction
                assert float((dga - dgb).abs().max()) <= tol and float((dba - dbb).abs().max()) <= tol

        kind, slabs = e_wgrad.split(' ')
        dw = G.empty((Co, k, k, Ci), torch.float32, gpu, 'dw')          # nothing but the guard fill: the launch must overwrite it
        _, labels = _run(ops, lambda: ops.conv_wgrad(desc, xd, dyd, dw, accumulate=False))
        print('\nLABEL %swgrad %s' % (tag, ' | '.join(labels)))
        assert len(labels) == 1 and labels[0].split(' ')[0] == kind and labels[0].split(' ')[-1] == slabs, (labels, e_wgrad)
        _same(tag + 'wgrad', dw, c.dw, torch.float32)
        dw = _vec(c.dw0, gpu, 'dw')
        _, labels = _run(ops, lambda: ops.conv_wgrad(desc, xd, dyd, dw, accumulate=True))
        assert len(labels) == 1 and labels[0].split(' ')[0] == kind and labels[0].split(' ')[-1] == slabs, (labels, e_wgrad)
        _same(tag + 'wgrad+acc', dw, c.dw_acc, torch.float32)
        if dt == 'f32':
            R._cache.pop(name, None)          # both formats done: drop the float64 references of this case


# ---------------------------------------------------------------------------------------------- concat-K forward
_CAT = [(n, dt) for n in _names(R.CAT_CASES) for dt in ('bf16', 'f32')]
if _CAT:
    @pytest.mark.parametrize('name,dt', _CAT, ids=['%s-%s' % p for p in _CAT])
    def test_concat_k_builds_return_the_reference_bits(gpu, name, dt):
        ops = _ops()
        c = R.build_cat_case(name)
        dtype = DT[dt]
        expect = CAT_EXPECT[name][0 if dt == 'bf16' else 1]
        N, Ci, H, W, Co, k, s, p = c.shape
        desc = ops.make_desc(N, H, W, Ci, Co, k, k, s, p, dtype)
        _pitch(dtype, Ci, Co)
        xd = _dev(c.x, dtype, gpu)
        wf, _ = _packs(ops, _vec(c.w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, k * k, Ci, Ci, dtype)
        b1, b2 = _vec(c.b1, gpu, 'bias'), _vec(c.b2, gpu, 'bias2')
        for n2 in R.CAT_C2[dtype]:          # one 16-byte chunk of second-operand channels, and three
            R.assert_exact_in(dtype, c.y[n2], c.y_b[n2])
            x2d, w2 = _dev(c.x2[n2], dtype, gpu), _vec(c.w2[n2].to(dtype), gpu, 'w2')
            tag = '%s/%s c2=%d ' % (name, dt, n2)
            y, labels = _run(ops, lambda: ops.conv_fwd_cat(desc, xd, wf, None, x2d, w2, None))
            assert _check_builds(tag + 'cat', labels, expect) == 0
            _same(tag + 'cat', y, c.y[n2], dtype)
            y, labels = _run(ops, lambda: ops.conv_fwd_cat(desc, xd, wf, b1, x2d, w2, b2))
            assert _check_builds(tag + 'cat+bias', labels, expect) == 0
            _same(tag + 'cat+bias', y, c.y_b[n2], dtype)
            (y, part), labels = _run(ops, lambda: ops.conv_fwd_cat(desc, xd, wf, b1, x2d, w2, b2, want_stats=True))
            assert _check_builds(tag + 'cat+stats', labels, expect) == 1
            _same(tag + 'cat+stats', y, c.y_b[n2], dtype)
            _check_stats(tag + 'cat+stats', part, Co, c.y_b[n2], N * c.Ho * c.Wo)


# ---------------------------------------------------------------------------------------------- rounding of the store path
ROUNDING = {g: [c + (e,) for c, e in zip(R.ROUNDING_CASES[g], ROUNDING_EXPECT[g])] for g in R.ROUNDING_CASES}
if GROUP in ROUNDING:
    @pytest.mark.parametrize('case', ROUNDING[GROUP], ids=lambda c: '%s-%dx%dx%dx%d' % ((c[5].replace(' ', '_'),) + c[:4]))
    def test_bf16_store_rounds_to_nearest_even(gpu, case):
        """The exact tests never round; this one pins the one rounding they do not see.  Sums of 256 .. 384 in magnitude, where
        bf16 is spaced by 2: odd sums are ties.  Expected: float64 -> fp32 -> bf16, i.e. round to nearest even."""
        import mi355
        ops = _ops()
        lib = mi355.load()
        N, H, W, Co, pg, expect = case
        x, w, sums = R.rounding_case(N, H, W, Co)
        ref = R.conv_fwd(x, w, 1, 0)
        assert set(int(v) for v in ref.unique()) == set(sums)
        assert not torch.equal(R.to_dtype(ref, torch.bfloat16).double(), ref)         # the case does round
        desc = ops.make_desc(N, H, W, 64, Co, 1, 1, 1, 0, torch.bfloat16)
        _pitch(torch.bfloat16, 64, Co)
        wf, _ = _packs(ops, _vec(w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, 1, 64, 64, torch.bfloat16)
        xd = _dev(x, torch.bfloat16, gpu)
        prev = lib.mi355_set_pgemm(pg) if pg is not None else None
        try:
            y, labels = _run(ops, lambda: ops.conv_fwd(desc, xd, wf))
        finally:
            if pg is not None:
                lib.mi355_set_pgemm(prev)
        assert _check_builds('rounding %s' % (case,), labels, expect) == 0
        _same('rounding', y, ref, torch.bfloat16)


if GROUP == 'default':
    # ------------------------------------------------------------------------------------------ persistent GEMM
    @pytest.mark.parametrize('name', sorted(PGEMM))
    def test_pgemm_builds_return_the_reference_bits(gpu, name):
        """mi355_set_pgemm(2): the persistent GEMM wherever the launch fits it -- 351 rows (the last of six row tiles holds 31),
        K = 64 .. 512 (the longest K whose weight slice fits LDS; every ring depth the defaults choose), 64- and 128-wide column tiles,
        72 live columns, every epilogue."""
        import mi355
        ops = _ops()
        lib = mi355.load()
        c = R.build_pgemm_case(name)
        N, Ci, H, W, Co = c.shape
        has_dgrad, (e_fwd, e_dgrad) = c.has_dgrad, PGEMM[name]
        dtype = torch.bfloat16
        R.assert_exact_in(dtype, *c.values)
        x, w, bias, res, y, y_b, y_brr = c.x, c.w, c.bias, c.res, c.y, c.y_b, c.y_brr
        desc = ops.make_desc(N, H, W, Ci, Co, 1, 1, 1, 0, dtype)
        _pitch(dtype, Ci, Co)
        wf, wt = _packs(ops, _vec(w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, 1, Ci, Ci, dtype)
        xd, resd, biasd = _dev(x, dtype, gpu), _dev(res, dtype, gpu), _vec(bias, gpu, 'bias')
        prev = lib.mi355_set_pgemm(2)
        try:
            for what, fn, ref, exp in (('fwd', lambda: ops.conv_fwd(desc, xd, wf), y, e_fwd[0]),
                                       ('fwd+bias', lambda: ops.conv_fwd(desc, xd, wf, biasd), y_b, e_fwd[0]),
                                       ('fwd+bias+res+relu', lambda: ops.conv_fwd(desc, xd, wf, biasd, resd, relu=True), y_brr, e_fwd[1])):
                got, labels = _run(ops, fn)
                assert _check_builds('%s %s' % (name, what), labels, exp) == 0
                _same('%s %s' % (name, what), got, ref, dtype)
            (got, part), labels = _run(ops, lambda: ops.conv_fwd_stats(desc, xd, wf, biasd))
            assert _check_builds(name + ' fwd+stats', labels, e_fwd[0]) == 1
            _same(name + ' fwd+stats', got, y_b, dtype)
            _check_stats(name + ' fwd+stats', part, Co, y_b, N * H * W)
            if has_dgrad:
                dy, base, mask, dx, dx_acc, dx_macc = c.dy, c.base, c.mask, c.dx, c.dx_acc, c.dx_macc
                dyd, based, sc, maskd = _dev(dy, dtype, gpu), _dev(base, dtype, gpu), _vec(torch.full((1,), 0.25), gpu, 'scale'), _vec(mask, gpu, 'mask')
                for what, fn, ref, exp in (
                        ('dgrad', lambda: ops.conv_dgrad(desc, dyd, wt), dx, e_dgrad[0]),
                        ('dgrad*scale+acc', lambda: ops.conv_dgrad(desc, dyd, wt, scale_dev=sc, out=G.place(based, 'base'), accumulate=True), dx_acc, e_dgrad[1]),
                        ('dgrad+macc', lambda: ops.conv_dgrad_masked_acc(desc, dyd, wt, G.place(based, 'base'), maskd), dx_macc, e_dgrad[1])):
                    got, labels = _run(ops, fn)
                    assert _check_builds('%s %s' % (name, what), labels, exp) == 0
                    _same('%s %s' % (name, what), got, ref, dtype)
        finally:
            lib.mi355_set_pgemm(prev)

    # ------------------------------------------------------------------------------------------ 21-channel heat-map conv
    @pytest.mark.parametrize('dt', ['bf16', 'f32'])
    @pytest.mark.parametrize('name', sorted(R.HM_CASES))
    def test_heatmap_conv_returns_the_reference_bits(gpu, dt, name):
        """conv1x1_heatmap (128 x 32 tile, NCHW fp32 output): HW = 120 (row tiles that straddle images and a partial last one) and
        4096, K = 21."""
        ops = _ops()
        dtype = DT[dt]
        N, C, K, H, W = R.HM_CASES[name]
        c = R.build_hm_case(name)
        R.assert_exact_in(torch.float32, c.ref)
        _pitch(dtype, C)
        xd, wd, bd = _dev(c.x, dtype, gpu), _vec(c.w.view(K, C).to(dtype), gpu, 'weights'), _vec(c.b, gpu, 'bias')
        y, labels = _run(ops, lambda: ops.conv1x1_heatmap(xd, wd, bd, K))
        assert _check_builds('%s/%s' % (name, dt), labels, 'g128x32 hm' if dt == 'bf16' else 'g128x32 f32 hm') == 0
        assert y.is_contiguous()
        _same(name, y, c.ref, torch.float32)

    # ------------------------------------------------------------------------------------------ grouped weight gradients
    GROUPED = {     # form: the launches R.GROUPED_CASES[form] must make (kernel and items per launch), in order
        'wgrad_group':    ['wgrad_group x3', 'wgrad_group x1'],
        'wgrad_group256': ['wgrad_group256 x2', 'wgrad_group256 x1'],
        'wgrad_kw_group': ['wgrad_kw_group x1', 'wgrad_kw_group x2', 'wgrad_kw_group x1'],
    }
    _GROUPED = [(f, dt) for f in sorted(GROUPED) for dt in R.GROUPED_CASES[f][0]]

    @pytest.mark.parametrize('form,dt', _GROUPED, ids=['%s-%s' % p for p in _GROUPED])
    def test_grouped_weight_gradients_return_the_reference_bits(gpu, form, dt):
        """The three grouped weight-gradient kernels on mixed items: overwriting and accumulating ones, a strided 1x1, a 3x3 the
        specialised kernels do not take, and an item that accumulates onto the gradient an earlier item of the call wrote."""
        ops = _ops()
        dtype = DT[dt]
        heads = GROUPED[form]
        cases, refs = R.build_grouped_case(form)
        items = []
        _pitch(dtype, *[ch for shape, _, _, _ in cases for ch in shape[3:5]])
        for (N, H, W, Ci, Co, k, s, p, acc, share), x, dy, dw0 in cases:
            if share is not None:
                dw = items[share][3]
            elif acc:
                dw = _vec(dw0, gpu, 'dw')
            else:
                dw = G.empty((Co, k, k, Ci), torch.float32, gpu, 'dw')
            items.append((ops.make_desc(N, H, W, Ci, Co, k, k, s, p, dtype), _dev(x, dtype, gpu), _dev(dy, dtype, gpu), dw, acc))
        R.assert_exact_in(torch.float32, *[r for r in refs if r is not None])
        _, labels = _run(ops, lambda: ops.conv_wgrad_grouped(items))
        print('\nLABEL %s/%s %s' % (form, dt, ' | '.join(labels)))
        assert [' '.join(l.split(' ')[:2]) for l in labels] == heads, labels
        for i, ref in enumerate(refs):
            if ref is not None:
                _same('%s item %d' % (form, i), items[i][3], ref, torch.float32)


# ---------------------------------------------------------------------------------------------- fp8 and MX operands
_FP8 = _names(R.FP8_CASES)
if _FP8:
    @pytest.mark.parametrize('name', _FP8)
    def test_fp8_and_mx_builds_return_the_reference_bits(gpu, name):
        """The same integers through the fp8 quantisers (just-in-time power-of-two scales) and the MX quantiser (E8M0 block
        scales): quantise -> dequantise must return them unchanged -- a test of the quantisers and the precondition for exactness
        -- and then every fp8 / MX convolution must return the reference's bits."""
        import mi355
        ops = _ops()
        lib = mi355.load()
        c = R.build_fp8_case(name)
        bf16 = torch.bfloat16
        R.assert_exact_in(bf16, c.y, c.y_b, c.dx, c.dx_q, c.dx_acc)
        R.assert_exact_in(torch.float32, c.dw, c.dw_acc)
        N, Ci, H, W, Co, k, s, p = c.shape
        e_plain, e_kw3 = FP8_EXPECT[name]
        e_fwd, e_dgrad = e_plain if isinstance(e_plain, tuple) else (e_plain, e_plain)
        desc = ops.make_desc_fp8(N, H, W, Ci, Co, k, k, s, p)
        _pitch(bf16, Ci, Co)
        xd, dyd, based = _dev(c.x, bf16, gpu), _dev(c.dy, bf16, gpu), _dev(c.base, bf16, gpu)
        w_conv = _vec(c.w.permute(0, 2, 3, 1), gpu, 'master weights')
        bias, sc = _vec(c.bias, gpu, 'bias'), _vec(torch.full((1,), 0.25), gpu, 'scale')
        sx, sw, sd = [_vec(ops.fp8_state(gpu), gpu, 'fp8 state') for _ in range(3)]
        # the fp8 copies are made inside a guard window: the GEMMs below read them with 0xFF on either side
        x8 = _guarded(ops, 'fp8_quantize x', lambda: ops.fp8_quantize(xd, sx, ops.E4M3, jit=True))
        dy8 = _guarded(ops, 'fp8_quantize dy', lambda: ops.fp8_quantize(dyd, sd, ops.E5M2, jit=True))
        wf8, wt8 = _guarded(ops, 'pack_weights_fp8', lambda: ops.pack_weights_fp8(w_conv, Co, k * k, Ci, sw))
        for what, t in (('x8', x8), ('dy8', dy8), ('wf8', wf8), ('wt8', wt8)):
            _whole(what, t)
        assert torch.equal((x8.view(torch.float8_e4m3fn).float() * sx[1]).cpu(), c.x)
        assert torch.equal((dy8.view(torch.float8_e5m2).float() * sd[1]).cpu(), c.dy)
        assert torch.equal((wf8.view(torch.float8_e4m3fn).float() * sw[1]).view(Co, k, k, Ci).cpu(), c.w.permute(0, 2, 3, 1))
        assert torch.equal((wt8.view(torch.float8_e4m3fn).float() * sw[1]).view(Ci, k, k, Co).cpu(), c.w.permute(1, 2, 3, 0))
        prev = lib.mi355_set_fp8_kw3(0)
        try:
            for mode, ef, ed in ((0, e_fwd, e_dgrad), (1, e_kw3, e_kw3)):
                if ef is None:
                    continue
                lib.mi355_set_fp8_kw3(mode)
                tag = '%s kw3=%d ' % (name, mode)
                (y, part), labels = _run(ops, lambda: ops.conv_fwd_fp8(desc, x8, sx, wf8, sw, bias, want_stats=True))
                assert _check_builds(tag + 'fwd8', labels, 'f8 ' + ef) == 1
                _same(tag + 'fwd8', y, c.y_b, bf16)
                _check_stats(tag + 'fwd8', part, Co, c.y_b, N * c.Ho * c.Wo)
                y, labels = _run(ops, lambda: ops.conv_fwd_fp8(desc, x8, sx, wf8, sw))
                assert _check_builds(tag + 'fwd8 plain', labels, 'f8 ' + ef) == 0
                _same(tag + 'fwd8 plain', y, c.y, bf16)
                dx, labels = _run(ops, lambda: ops.conv_dgrad_fp8(desc, dy8, sd, wt8, sw))
                assert _check_builds(tag + 'dgrad8', labels, 'f8 ' + ed + ' bf8') == 0
                _same(tag + 'dgrad8', dx, c.dx, bf16)
                (dx, part), labels = _run(ops, lambda: ops.conv_dgrad_fp8(desc, dy8, sd, wt8, sw, want_stats=True))
                epi = _check_builds(tag + 'dgrad8+stats', labels, 'f8 ' + ed + ' bf8')
                _same(tag + 'dgrad8+stats', dx, c.dx, bf16)
                assert (epi == 1) == (part is not None) and (epi == 1 or s != 1)
                if part is not None:
                    _check_stats(tag + 'dgrad8+stats', part, Ci, c.dx, N * H * W)
                dx, labels = _run(ops, lambda: ops.conv_dgrad_fp8(desc, dy8, sd, wt8, sw, scale_dev=sc, out=G.place(based, 'base'), accumulate=True))
                assert _check_builds(tag + 'dgrad8*scale+acc', labels, 'f8 ' + ed + ' bf8') == 0
                _same(tag + 'dgrad8*scale+acc', dx, c.dx_acc, bf16)
        finally:
            lib.mi355_set_fp8_kw3(prev)
        dw = G.empty((Co, k, k, Ci), torch.float32, gpu, 'dw')
        _, labels = _run(ops, lambda: ops.conv_wgrad_fp8(desc, x8, sx, dy8, sd, dw, False))
        print('\nLABEL %s wgrad8 %s' % (name, ' | '.join(labels)))
        assert len(labels) == 1 and labels[0].startswith('wgrad8 '), labels
        _same(name + ' wgrad8', dw, c.dw, torch.float32)
        dw = _vec(c.dw0, gpu, 'dw')
        _run(ops, lambda: ops.conv_wgrad_fp8(desc, x8, sx, dy8, sd, dw, True))
        _same(name + ' wgrad8+acc', dw, c.dw_acc, torch.float32)

        # MX: e4m3 elements, one E8M0 scale per 32 contracted channels
        # ... and so are the MX copies with their E8M0 scale arrays: a scale load one block off reads 0xFF, the NaN code
        xq, xs = _guarded(ops, 'mx_quantize x', lambda: ops.mx_quantize(xd))
        dyq, dys = _guarded(ops, 'mx_quantize dy', lambda: ops.mx_quantize(dyd))
        wf, sf, wt, st = _guarded(ops, 'pack_weights_mx', lambda: ops.pack_weights_mx(w_conv, Co, k * k, Ci))
        for what, t in (('xq', xq), ('xs', xs), ('dyq', dyq), ('dys', dys), ('wf', wf), ('sf', sf), ('wt', wt), ('st', st)):
            _whole(what, t)
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().cpu()
        assert torch.equal(mx_dequantize(nhwc(xq), xs.view(N, H, W, Ci // 32).cpu()), c.x.permute(0, 2, 3, 1))
        assert torch.equal(mx_dequantize(nhwc(dyq), dys.view(N, c.Ho, c.Wo, Co // 32).cpu()), c.dy.permute(0, 2, 3, 1))
        assert torch.equal(mx_dequantize(wf.view(Co, k, k, Ci).cpu(), sf.view(Co, k, k, Ci // 32).cpu()), c.w.permute(0, 2, 3, 1))
        assert torch.equal(mx_dequantize(wt.view(Ci, k, k, Co).cpu(), st.view(Ci, k, k, Co // 32).cpu()), c.w.permute(1, 2, 3, 0))
        (y, part), labels = _run(ops, lambda: ops.conv_fwd_mx(desc, xq, xs, wf, sf, bias, want_stats=True))
        assert _check_builds(name + ' fwdmx', labels, 'mx ' + e_fwd) == 1
        _same(name + ' fwdmx', y, c.y_b, bf16)
        _check_stats(name + ' fwdmx', part, Co, c.y_b, N * c.Ho * c.Wo)
        dx, labels = _run(ops, lambda: ops.conv_dgrad_mx(desc, dyq, dys, wt, st))
        assert _check_builds(name + ' dgradmx', labels, 'mx ' + e_dgrad) == 0
        _same(name + ' dgradmx', dx, c.dx, bf16)
        (dx, part), labels = _run(ops, lambda: ops.conv_dgrad_mx(desc, dyq, dys, wt, st, want_stats=True))
        epi = _check_builds(name + ' dgradmx+stats', labels, 'mx ' + e_dgrad)
        _same(name + ' dgradmx+stats', dx, c.dx, bf16)
        assert (epi == 1) == (part is not None) and (epi == 1 or s != 1)
        if part is not None:
            _check_stats(name + ' dgradmx+stats', part, Ci, c.dx, N * H * W)
        y, labels = _run(ops, lambda: ops.conv_fwd_mx(desc, xq, xs, wf, sf))
        assert _check_builds(name + ' fwdmx plain', labels, 'mx ' + e_fwd) == 0
        _same(name + ' fwdmx plain', y, c.y, bf16)
        dx, labels = _run(ops, lambda: ops.conv_dgrad_mx(desc, dyq, dys, wt, st, scale_dev=sc, out=G.place(based, 'base'), accumulate=True))
        assert _check_builds(name + ' dgradmx*scale+acc', labels, 'mx ' + e_dgrad) == 0
        _same(name + ' dgradmx*scale+acc', dx, c.dx_acc, bf16)


# ---------------------------------------------------------------------------------------------- NaN, +Inf and -Inf operands
# tests/nonfinite_ref.py: a few elements of ONE operand are NaN / +Inf / -Inf, every other value stays an exact integer.  The
# pointwise rule: the class of every output element is the float64 reference's and every finite element has its bits.  The
# cases, their positions and the condition on the reference are held without a GPU by test_nonfinite_cpu.py.
def _pointwise(what, got, ref, dtype):
    _whole(what, got)          # (a NaN a kernel computed or passed through is not the all-ones fill)
    bad = NF.pointwise_mismatch(got, ref, dtype)
    assert bad is None, '%s: %s' % (what, bad)


_SPECIALS = [(s, dt) for s in NF.CONV_SPECIALS if R.CASES[s[1]][0] == GROUP for dt in ('bf16', 'f32')]
if _SPECIALS:
    @pytest.mark.parametrize('spec,dt', _SPECIALS, ids=['%s-%s' % (NF.special_id(s), dt) for s, dt in _SPECIALS])
    def test_specials_come_out_where_the_reference_has_them(gpu, spec, dt):
        ops = _ops()
        mode, name, operand = spec
        sp = NF.conv_special(mode, name, operand)
        for what, ref in sp['refs'].items():          # the cap on the case, before any kernel result is read
            NF.case_condition(ref, sp['expect'][what], '%s %s' % (NF.special_id(spec), what))
        c, o, refs = sp['case'], sp['ops'], sp['refs']
        dtype, per = DT[dt], (8 if dt == 'bf16' else 4)
        e_fwd, e_dgrad, e_acc, e_bnb, e_wgrad = EXPECT[name][0 if dt == 'bf16' else 1]
        N, Ci, H, W, Co, k, s, p = c.shape
        desc = ops.make_desc(N, H, W, Ci, Co, k, k, s, p, dtype, out_hw=c.out_hw)
        _pitch(dtype, Ci, Co)
        wf, wt = _packs(ops, _vec(o['w'].permute(0, 2, 3, 1), gpu, 'master weights'), Co, k * k, Ci, Ci, dtype)
        tag = '%s/%s ' % (NF.special_id(spec), dt)
        if mode == 'fwd':
            xd, bias, res = _dev(o['x'], dtype, gpu), _vec(o['bias'], gpu, 'bias'), _dev(o['res'], dtype, gpu)
            for what, relu in (('fwd+bias+res', False), ('fwd+bias+res+relu', True)):
                y, labels = _run(ops, lambda: ops.conv_fwd(desc, xd, wf, bias, res, relu=relu))
                assert _check_builds(tag + what, labels, e_fwd) == 0
                _pointwise(tag + what, y, refs[what], dtype)
        elif mode == 'dgrad':
            dyd, base, sc = _dev(o['dy'], dtype, gpu), _dev(o['base'], dtype, gpu), _vec(torch.full((1,), 0.25), gpu, 'scale')
            for what, fn, exp in (('dgrad', lambda: ops.conv_dgrad(desc, dyd, wt), e_dgrad),
                                  ('dgrad*scale', lambda: ops.conv_dgrad(desc, dyd, wt, scale_dev=sc), e_dgrad),
                                  ('dgrad*scale+acc', lambda: ops.conv_dgrad(desc, dyd, wt, scale_dev=sc, out=G.place(base, 'base'), accumulate=True), e_acc)):
                if what in refs:
                    dx, labels = _run(ops, fn)
                    assert _check_builds(tag + what, labels, exp) == 0
                    _pointwise(tag + what, dx, refs[what], dtype)
        elif mode == 'macc':
            # a NaN base under a cleared bit contributes an exact zero (a select, as ATen's threshold_backward), under a set bit it stays
            dyd, base, mask = _dev(o['dy'], dtype, gpu), _dev(o['base'], dtype, gpu), _vec(c.mask[per], gpu, 'mask')
            what = 'dgrad+macc/%d' % per
            dx, labels = _run(ops, lambda: ops.conv_dgrad_masked_acc(desc, dyd, wt, G.place(base, 'base'), mask))
            assert _check_builds(tag + what, labels, e_acc) == 0
            _pointwise(tag + what, dx, refs[what], dtype)
        else:
            xd, dyd = _dev(o['x'], dtype, gpu), _dev(o['dy'], dtype, gpu)
            kind, slabs = e_wgrad.split(' ')
            for what, acc in (('wgrad', False), ('wgrad+acc', True)):
                if what in refs:
                    dw = _vec(o['dw0'], gpu, 'dw') if acc else G.empty((Co, k, k, Ci), torch.float32, gpu, 'dw')
                    _, labels = _run(ops, lambda: ops.conv_wgrad(desc, xd, dyd, dw, accumulate=acc))
                    assert len(labels) == 1 and labels[0].split(' ')[0] == kind and labels[0].split(' ')[-1] == slabs, (labels, e_wgrad)
                    _pointwise(tag + what, dw, refs[what], torch.float32)


def _fold_or_raw(part, C, width):
    """The written slices of an epilogue's partials [slice][C][width] as float64 on the host."""
    return part[0][:part[1] * C * width].detach().cpu().double().view(part[1], C, width)


if GROUP == 'default':
    @pytest.mark.parametrize('dt', ['bf16', 'f32'])
    def test_statistics_epilogue_keeps_an_inf_in_its_channel(gpu, dt):
        """conv_fwd_stats with +Inf in one bias element and conv_dgrad_stats with +Inf in one weight of one input channel: that
        channel's partials are non-finite in every slice that holds one of its non-finite outputs, every other channel's partials
        are the bits of the clean run, and the outputs follow the pointwise rule."""
        ops = _ops()
        dtype = DT[dt]
        for name, side in (('t64_co72', 'fwd'), ('small_dgrad', 'dgrad')):
            c = R.build_case(name)
            N, Ci, H, W, Co, k, s, p = c.shape
            e_fwd, e_dgrad = EXPECT[name][0 if dt == 'bf16' else 1][:2]
            desc = ops.make_desc(N, H, W, Ci, Co, k, k, s, p, dtype)
            _pitch(dtype, Ci, Co)
            xd, dyd = _dev(c.x, dtype, gpu), _dev(c.dy, dtype, gpu)
            runs = {}
            for poisoned in (False, True):
                if side == 'fwd':
                    C_, ch, rows = Co, Co - 1, N * c.Ho * c.Wo
                    bias = NF.seed_specials(c.bias, [((ch,), '+inf')]) if poisoned else c.bias
                    wf, _ = _packs(ops, _vec(c.w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, k * k, Ci, Ci, dtype)
                    bd = _vec(bias, gpu, 'bias')
                    (y, part), labels = _run(ops, lambda: ops.conv_fwd_stats(desc, xd, wf, bd))
                    assert _check_builds('%s fwd+stats' % name, labels, e_fwd) == 1
                    ref = NF.fwd_epilogue(c.y, bias)
                else:
                    C_, ch, rows = Ci, Ci - 1, N * H * W
                    w = NF.seed_specials(c.w, [((Co - 1, ch, k // 2, k // 2), '+inf')]) if poisoned else c.w
                    _, wt = _packs(ops, _vec(w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, k * k, Ci, Ci, dtype)
                    (y, part), labels = _run(ops, lambda: ops.conv_dgrad_stats(desc, dyd, wt))
                    assert _check_builds('%s dgrad+stats' % name, labels, e_dgrad) == 1
                    ref = R.conv_dgrad(c.dy, w, s, p, (H, W))
                if poisoned:
                    n = NF.class_counts(ref)
                    assert 4 * n[NF.FINITE] >= ref.numel() and n[NF.FINITE] < ref.numel()
                    assert bool(torch.isfinite(ref[:, [q for q in range(C_) if q != ch]]).all()) and not bool(torch.isfinite(ref[:, ch]).all())
                _pointwise('%s %s+stats' % (name, side), y, ref, dtype)
                assert part is not None
                runs[poisoned] = (_fold_or_raw(part, C_, 3), R.fold_stats(part[0], part[1], C_), ref)
            (pc, _, _), (pp, (tot, mean, m2), ref) = runs[False], runs[True]
            others = [q for q in range(C_) if q != ch]
            assert torch.equal(pc[:, others], pp[:, others]), '%s: an Inf in channel %d changed the partials of another channel' % (name, ch)
            assert torch.equal(pc[:, :, 0], pp[:, :, 0])                    # the counts are counts
            nr, rmean, rm2 = R.bn_stats(ref)
            assert NF.reduced_mismatch(tot, torch.full((C_,), float(rows), dtype=torch.float64)) is None
            inv, rinv = 1.0 / torch.sqrt(m2 / tot + 1e-5), 1.0 / torch.sqrt(rm2 / nr + 1e-5)
            for what, got, want, tol in (('mean', mean, rmean, dict(rtol=1e-5, atol=1e-6)), ('invstd', inv, rinv, dict(rtol=2e-5, atol=1e-6))):
                bad = NF.reduced_mismatch(got, want, **tol)          # (the tolerances of _check_stats)
                assert bad is None, '%s %s: %s' % (name, what, bad)
            assert not bool(torch.isfinite(mean[ch])) and not bool(torch.isfinite(m2[ch]))

    @pytest.mark.parametrize('relu', ['none', 'from_y', 'from_x'])
    @pytest.mark.parametrize('dt', ['bf16', 'f32'])
    def test_bn_backward_epilogue_drops_a_masked_nan_and_keeps_a_live_one(gpu, dt, relu):
        """conv_dgrad_bnbwd (accumulating, the NaN in ONE element of the base, so in one element of the BatchNorm's dy) and
        conv_fwd_bnbwd (the NaN in x: a window of the BatchNorm's dy in every channel).  A NaN where the ReLU mask clears the
        gradient changes no partial at all (the bits of the clean run); one where the mask keeps it makes that channel's sums
        non-finite and no other's.  The stored gradient follows the pointwise rule either way."""
        ops = _ops()
        dtype = DT[dt]
        for name, side in (('small_dgrad', 'dgrad'), ('t64_s2', 'fwd')):
            c = R.build_case(name)
            N, Ci, H, W, Co, k, s, p = c.shape
            e = EXPECT[name][0 if dt == 'bf16' else 1]
            desc = ops.make_desc(N, H, W, Ci, Co, k, k, s, p, dtype)
            _pitch(dtype, Ci, Co)
            wf, wt = _packs(ops, _vec(c.w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, k * k, Ci, Ci, dtype)
            C_, bshape, bias_c = (Ci, (N, Ci, H, W), c.bias_i) if side == 'dgrad' else (Co, (N, Co, c.Ho, c.Wo), c.bias)
            xb64 = R.ints(R.seed_of(name + '/bn x'), *bshape, lo=-16, hi=16)
            xb = _dev(xb64, dtype, gpu)
            gamma, beta = _vec(1 + bias_c / 64, gpu, 'gamma'), _vec(bias_c / 32, gpu, 'beta')
            rm, rv, nbt = _vec(torch.zeros(C_), gpu, 'running_mean'), _vec(torch.ones(C_), gpu, 'running_var'), _vec(torch.zeros((), dtype=torch.int64), gpu, 'num_batches_tracked')
            yb, mean, invstd = _guarded(ops, 'bn_train_fwd', lambda: ops.bn_train_fwd(xb, None, gamma, beta, rm, rv, nbt, 1e-5, 0.1, relu != 'none'))
            bn = (xb, yb if relu == 'from_y' else None, gamma, beta, mean, invstd, relu != 'none')
            # where the mask keeps and where it clears, away from the threshold: the stored y for the kept side, the float64
            # pre-activation (from the kernel's own statistics) for the cleared one
            pre = (xb64.double() - mean.double().cpu().view(1, -1, 1, 1)) * (gamma.double() * invstd.double()).cpu().view(1, -1, 1, 1) + beta.double().cpu().view(1, -1, 1, 1)
            kept = (yb.float().cpu() > 0.1) if relu != 'none' else torch.ones(bshape, dtype=torch.bool)
            cleared = (pre < -0.1) & (yb.float().cpu() == 0) if relu != 'none' else torch.zeros(bshape, dtype=torch.bool)
            sure = kept | cleared
            assert relu == 'none' or (bool(kept.any()) and bool(cleared.any()))

            def run(ops_in):
                if side == 'dgrad':
                    dyd, base = _dev(c.dy, dtype, gpu), _dev(ops_in, dtype, gpu)
                    (g, part), labels = _run(ops, lambda: ops.conv_dgrad_bnbwd(desc, dyd, wt, bn, out=G.place(base, 'base'), accumulate=True))
                    assert _check_builds('%s dgrad+bnb' % name, labels, e[3]) == 2
                    return g, part, R.dgrad_epilogue(c.dx, 1.0, ops_in)
                xd = _dev(ops_in, dtype, gpu)
                (g, part), labels = _run(ops, lambda: ops.conv_fwd_bnbwd(desc, xd, wf, bn))
                assert _check_builds('%s fwd+bnb' % name, labels, e[0]) == 2
                return g, part, R.conv_fwd(ops_in, c.w, s, p)

            clean_in = c.base if side == 'dgrad' else c.x
            g, part, ref = run(clean_in)
            _same('%s clean' % name, g, ref, dtype)
            assert part is not None
            clean = _fold_or_raw(part, C_, 2)
            for want_live in ((False, True) if relu != 'none' else (True,)):
                if side == 'fwd' and not want_live:
                    continue                 # (the window below holds kept and cleared elements at once)
                if side == 'dgrad':          # one element of the BatchNorm's dy
                    where = (kept if want_live else cleared).nonzero()
                    idx = tuple(int(v) for v in where[where.shape[0] // 2])
                else:                        # an x pixel: the 3x3 window of outputs around it, every channel
                    idx = (N - 1, Ci - 1, H // 2, W // 2)
                g, part, ref = run(NF.seed_specials(clean_in, [(idx, 'nan')]))
                nan = ref != ref
                assert bool(nan.any()) and 4 * int((~nan).sum()) >= ref.numel()
                _pointwise('%s %s nan' % (name, side), g, ref, dtype)
                assert part is not None
                got = _fold_or_raw(part, C_, 2)
                per_channel = lambda m: m.permute(1, 0, 2, 3).reshape(C_, -1).any(1)
                live, doubt = per_channel(nan & kept), per_channel(nan & ~sure)          # (doubt: a NaN where y sits at the threshold)
                if side == 'dgrad':
                    assert bool(live.any()) == want_live
                for ch in range(C_):
                    if bool(doubt[ch]):
                        continue
                    if bool(live[ch]):
                        assert not bool(torch.isfinite(got[:, ch].sum(0)).any()), '%s: the live NaN of channel %d left a finite sum' % (name, ch)
                    else:
                        assert torch.equal(got[:, ch], clean[:, ch]), '%s: a masked NaN (or one of another channel) changed the sums of channel %d' % (name, ch)

    @pytest.mark.parametrize('dt', ['bf16', 'f32'])
    def test_concat_k_and_heatmap_conv_with_specials(gpu, dt):
        ops = _ops()
        dtype, i = DT[dt], (0 if dt == 'bf16' else 1)
        name = 'cat_64x64'
        c = R.build_cat_case(name)
        N, Ci, H, W, Co, k, s, p = c.shape
        desc = ops.make_desc(N, H, W, Ci, Co, k, k, s, p, dtype)
        _pitch(dtype, Ci, Co)
        xd = _dev(c.x, dtype, gpu)
        wf, _ = _packs(ops, _vec(c.w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, k * k, Ci, Ci, dtype)
        b1, b2 = _vec(c.b1, gpu, 'bias'), _vec(c.b2, gpu, 'bias2')
        for n2 in R.CAT_C2[dtype]:
            sp = NF.cat_special(name, n2, i)
            for what, ref in sp['refs'].items():
                NF.case_condition(ref, sp['kinds'], what)
            x2d, w2 = _dev(sp['x2'], dtype, gpu), _vec(c.w2[n2].to(dtype), gpu, 'w2')
            y, labels = _run(ops, lambda: ops.conv_fwd_cat(desc, xd, wf, None, x2d, w2, None))
            assert _check_builds('%s c2=%d cat' % (name, n2), labels, CAT_EXPECT[name][i]) == 0
            _pointwise('cat c2=%d' % n2, y, sp['refs']['cat'], dtype)
            y, labels = _run(ops, lambda: ops.conv_fwd_cat(desc, xd, wf, b1, x2d, w2, b2))
            assert _check_builds('%s c2=%d cat+bias' % (name, n2), labels, CAT_EXPECT[name][i]) == 0
            _pointwise('cat+bias c2=%d' % n2, y, sp['refs']['cat+bias'], dtype)
        sp = NF.hm_special('hm_120')
        NF.case_condition(sp['refs']['hm'], sp['kinds'], 'hm_120')
        Nh, Ch, K, Hh, Wh = R.HM_CASES['hm_120']
        hc = sp['case']
        _pitch(dtype, Ch)
        xh, wd, bd = _dev(sp['x'], dtype, gpu), _vec(hc.w.view(K, Ch).to(dtype), gpu, 'weights'), _vec(hc.b, gpu, 'bias')
        y, labels = _run(ops, lambda: ops.conv1x1_heatmap(xh, wd, bd, K))
        assert _check_builds('hm_120/%s' % dt, labels, 'g128x32 hm' if dt == 'bf16' else 'g128x32 f32 hm') == 0
        _pointwise('hm_120', y, sp['refs']['hm'], torch.float32)

    @pytest.mark.parametrize('dt', R.GROUPED_CASES['wgrad_group'][0])
    def test_grouped_weight_gradients_with_specials(gpu, dt):
        """The first grouped form: the dy of an overwriting item and the x of a slab-reduced strided 3x3 item carry the specials;
        the item that accumulates onto the first one's gradient adds a finite term to rows that are already special."""
        ops = _ops()
        dtype = DT[dt]
        cases, refs = NF.grouped_special('wgrad_group')
        for i in (0, 2):
            NF.case_condition(refs[i], NF.KINDS, 'wgrad_group item %d' % i)
        items = []
        _pitch(dtype, *[ch for shape, _, _, _ in cases for ch in shape[3:5]])
        for (N, H, W, Ci, Co, k, s, p, acc, share), x, dy, dw0 in cases:
            dw = items[share][3] if share is not None else (_vec(dw0, gpu, 'dw') if acc else G.empty((Co, k, k, Ci), torch.float32, gpu, 'dw'))
            items.append((ops.make_desc(N, H, W, Ci, Co, k, k, s, p, dtype), _dev(x, dtype, gpu), _dev(dy, dtype, gpu), dw, acc))
        _, labels = _run(ops, lambda: ops.conv_wgrad_grouped(items))
        assert [' '.join(l.split(' ')[:2]) for l in labels] == GROUPED['wgrad_group'], labels
        for i, ref in enumerate(refs):
            if ref is not None:
                _pointwise('wgrad_group item %d' % i, items[i][3], ref, torch.float32)

    @pytest.mark.parametrize('name,operand', NF.PGEMM_SPECIALS, ids=['%s-%s' % s for s in NF.PGEMM_SPECIALS])
    def test_pgemm_with_specials(gpu, name, operand):
        """mi355_set_pgemm(2): the plain ring and the addend ring, ReLU off and on."""
        import mi355
        ops = _ops()
        lib = mi355.load()
        sp = NF.pgemm_special(name, operand)
        for what, ref in sp['refs'].items():
            NF.case_condition(ref, sp['expect'][what], '%s %s %s' % (name, operand, what))
        c, o, refs = sp['case'], sp['ops'], sp['refs']
        N, Ci, H, W, Co = c.shape
        e_plain, e_add = PGEMM[name][0]
        dtype = torch.bfloat16
        desc = ops.make_desc(N, H, W, Ci, Co, 1, 1, 1, 0, dtype)
        _pitch(dtype, Ci, Co)
        wf, _ = _packs(ops, _vec(c.w.permute(0, 2, 3, 1), gpu, 'master weights'), Co, 1, Ci, Ci, dtype)
        xd, resd, biasd = _dev(o['x'], dtype, gpu), _dev(o['res'], dtype, gpu), _vec(c.bias, gpu, 'bias')
        prev = lib.mi355_set_pgemm(2)
        try:
            for what, fn, exp in (('fwd', lambda: ops.conv_fwd(desc, xd, wf), e_plain),
                                  ('fwd+relu', lambda: ops.conv_fwd(desc, xd, wf, relu=True), None),
                                  ('fwd+bias+res', lambda: ops.conv_fwd(desc, xd, wf, biasd, resd), e_add),
                                  ('fwd+bias+res+relu', lambda: ops.conv_fwd(desc, xd, wf, biasd, resd, relu=True), e_add)):
                if what not in refs:
                    continue
                got, labels = _run(ops, fn)
                build = _build(labels[0])
                assert build.startswith('pgemm '), labels
                if exp is not None:
                    assert _check_builds('%s %s' % (name, what), labels, exp) == 0
                _pointwise('%s %s %s' % (name, operand, what), got, refs[what], dtype)
        finally:
            lib.mi355_set_pgemm(prev)

    @pytest.mark.parametrize('pg', [0, 2], ids=['gather', 'pgemm'])
    def test_bf16_store_overflows_to_inf_and_keeps_subnormals(gpu, pg):
        """Zero weights, the bias carries +-3.4e38 (rounds to +-Inf), the largest finite bf16 and the smallest bf16 subnormal:
        the stored bf16 is the fp32 value rounded once to nearest even, through the gather epilogue and the pgemm epilogue."""
        import mi355
        ops = _ops()
        lib = mi355.load()
        c = NF.store_overflow_case()
        N, Ci, H, W, Co = c['shape']
        dtype = torch.bfloat16
        desc = ops.make_desc(N, H, W, Ci, Co, 1, 1, 1, 0, dtype)
        _pitch(dtype, Ci, Co)
        wf, _ = _packs(ops, _vec(c['w'].permute(0, 2, 3, 1), gpu, 'master weights'), Co, 1, Ci, Ci, dtype)
        xd, bd = _dev(c['x'], dtype, gpu), _vec(c['bias'], gpu, 'bias')
        prev = lib.mi355_set_pgemm(pg)
        try:
            y, labels = _run(ops, lambda: ops.conv_fwd(desc, xd, wf, bd))
        finally:
            lib.mi355_set_pgemm(prev)
        print('\nLABEL store overflow pgemm=%d %s' % (pg, ' | '.join(labels)))
        assert len(labels) == 1 and _build(labels[0]).startswith('pgemm ' if pg else 'g'), labels
        _pointwise('store overflow', y, c['ref'], dtype)


# ---------------------------------------------------------------------------------------------- the forced builds, in children
if GROUP == 'default':
    _abnormal = []        # a child that ended by a signal, an abort or its timeout: nothing more is started on the GPU

    @pytest.mark.parametrize('group', sorted(GROUPS))
    def test_forced_builds_in_a_child_process(gpu, group):
        """This module once more under the switches of GROUPS[group] (read once per process, hence a child): the cases of that
        group only.  One child at a time, each with its own timeout, no retry."""
        if _abnormal:
            pytest.fail('not started after an abnormal exit (%s)' % _abnormal[0])
        env = dict(os.environ, MI355_CONV_EXACT_GROUP=group, **GROUPS[group])
        cmd = [sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-s', '-m', 'gpu', '-p', 'no:cacheprovider']
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
        except subprocess.TimeoutExpired:
            _abnormal.append('%s: timeout' % group)
            pytest.fail('child %s ran into its timeout' % group)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            _abnormal.append('%s: exit status %d' % (group, r.returncode))
        print('\n' + '\n'.join(l for l in r.stdout.splitlines() if l.startswith(('LABEL ', 'STATS '))))
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-2000:]
