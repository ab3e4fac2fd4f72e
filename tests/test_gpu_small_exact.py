"""The small hand-written kernels bit for bit on exact operands (tests/small_exact_ref.py): csrc/pool_layout.hip (A, B),
csrc/pw21.hip (C), csrc/optim.hip (D) and the argument checks of their wrappers (E).

Every comparison is one of two kinds, named next to it:
  [equal]  the same bits as the float64 reference (rounded once to nearest even where the output is bf16); NaN is compared by
           position, not by payload -- the kernels pass a NaN through the hardware's conversions, which keep no promise about
           the payload, and that is the one rule here that differs from a bit-for-bit copy of torch's result;
  [stats]  the tolerances of test_pointwise_k2c_walks_several_tiles_per_block_at_full_size, 1e-5 * (max |mean| + 1) and
           1e-4 * (max M2 + 1): only the mean and M2 columns of pw_k2c_stats, a Welford recurrence in fp32.
Operands go to the device as plain torch casts of exact values, and every cast is checked to have lost nothing.  Every kernel is
called inside its documented contract; section E calls the wrappers outside it and nothing launches there.

Guards (tests/guarded.py).  Sections A-D run inside poisoned guard buffers: every operand is a G.place() copy, every wrapper
call runs in a G.window() (_run), the flanks are checked after the device has been synchronised, and every freshly allocated
floating-point output has no unwritten element.  The row pitch is W * C * esize of the widest feature map of the shape at hand
(the windowed kernels step by image rows), set again for every shape a test loops over.  The in-place kernels (SGD, cast into a
view, = / += of a gradient) have their flanks checked and keep their exact comparison.  The window codes of the max-pool are
bytes: their references hold no 0xFF (asserted), so equality is the check.  Section F calls the ABI with a workspace one byte
short.  Outside the windows: test_maxpool_grid_stride_laps and test_to_nhwc_grid_stride_lap (2 M-chunk cases: flanks of 256
rows would cost time there for nothing new) and section E (nothing launches)."""

import numpy as np
import pytest
import torch

import guarded as G
import small_exact_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()


def _run(ops, label, fn, *args, **kw):
    """One wrapper call inside a guard window; the flanks of everything placed or allocated are intact afterwards."""
    with G.window(ops, label):
        out = fn(*args, **kw)
    torch.cuda.synchronize()
    G.check(label)
    return out


def _written(out, ref):
    """No element of `out` still holds the fill.  Where the reference `ref` (same logical shape) is a NaN the all-ones pattern is
    a legitimate result -- 0xFFFF is a bf16 NaN, and the hardware's conversion keeps no promise about the payload -- so those
    positions are left to the comparison that follows (NaN by position)."""
    ones = out.view(torch.int16 if out.element_size() == 2 else torch.int32) == -1
    return not bool((ones.cpu() & ~torch.isnan(ref.reshape(out.shape))).any())


def _pitch(W, C, dt):
    G.row_pitch(W * C * (2 if dt == 'bf16' else 4))


def _ops():
    import mi355
    from mi355 import ops
    mi355.load()
    return ops


def _feat(v64, dt, gpu, name='feature'):
    """Logical NCHW float64 -> channels_last `dt` on the device; the cast lost nothing."""
    d = R.nhwc(v64, R.TDT[dt]).to(gpu)
    assert R.bits_equal(d.double().cpu().contiguous(), v64.contiguous())
    return G.place(d, name)


def _f32(v64, gpu, name='f32 operand'):
    d = v64.float().contiguous().to(gpu)
    assert torch.equal(d.double().cpu(), v64)
    return G.place(d, name)


def _host(t):
    """Device tensor of the activation type -> logical float64 on the host."""
    return t.double().cpu().contiguous()


def _roomy(t, extra, fill):
    """The same logical channels_last tensor as a view of a buffer with `extra` more elements, those set to `fill`."""
    N, C, H, W = t.shape
    flat = t.permute(0, 2, 3, 1).reshape(-1)
    buf = torch.full((flat.numel() + extra,), fill, dtype=t.dtype, device=t.device)
    buf[:flat.numel()] = flat
    buf = G.place(buf, 'roomy')
    return buf[:flat.numel()].view(N, H, W, C).permute(0, 3, 1, 2), buf


# ================================================================ A. max-pool
@pytest.mark.parametrize('name', list(R.MP_CASES))
def test_maxpool_bit_for_bit(gpu, name):
    ops = _ops()
    c = R.mp_case(name)
    dt = c['dt']
    N, C, H, W = c['x'].shape
    Ho, Wo = R.mp_out(H, W)
    y_ref, code_ref, dx_ref = R.check_exact_maxpool(c)
    assert int(code_ref.max()) <= 8                     # no 0xFF in the reference: a code byte nobody wrote cannot pass
    _pitch(W, C, dt)
    y, arg = _run(ops, 'maxpool_fwd ' + name, ops.maxpool_fwd, _feat(c['x'], dt, gpu, 'x'))
    assert _written(y, y_ref)
    assert y.dtype == R.TDT[dt] and ops.is_nhwc(y) and tuple(y.shape) == (N, C, Ho, Wo)
    assert R.bits_equal(_host(y), y_ref), 'pooled values'                                            # [equal], NaN by position
    assert arg.dtype == torch.uint8 and tuple(arg.shape) == (N, Ho, Wo, C)
    assert torch.equal(arg.cpu(), code_ref.permute(0, 2, 3, 1)), 'window codes'                     # [equal]
    # dy and the codes as views of larger buffers whose tails would count if read (code 1, dy = 64): the window rows and columns
    # past Ho and Wo belong to nobody
    room = (Wo + 2) * C
    dyd, dy_buf = _roomy(_feat(c['dy'], dt, gpu, 'dy'), room, 64.0)
    argd, arg_buf = _roomy(arg.permute(0, 3, 1, 2), room, 1)
    dx = _run(ops, 'maxpool_bwd roomy ' + name, ops.maxpool_bwd, dyd, argd.permute(0, 2, 3, 1), (N, C, H, W))
    assert G.unwritten(dx) == 0
    assert dx.dtype == R.TDT[dt] and ops.is_nhwc(dx) and tuple(dx.shape) == (N, C, H, W)
    assert torch.equal(_host(dx), R.rne(dx_ref, dt)), 'dx'                                           # [equal]
    assert bool((dy_buf[-room:] == 64).all()) and bool((arg_buf[-room:] == 1).all())
    own = R.maxpool_bwd_np(c['dy'].numpy(), arg.cpu().permute(0, 3, 1, 2).numpy(), (N, C, H, W))
    assert np.array_equal(own, dx_ref.numpy()), 'dy scattered through the kernel\'s own codes'     # [equal]
    # the same with dy and the codes ending exactly where their guard flank begins: a window row or column past Ho / Wo that is
    # read would now be 0xFF (an impossible code, a NaN)
    dx = _run(ops, 'maxpool_bwd tight ' + name, ops.maxpool_bwd, _feat(c['dy'], dt, gpu, 'dy'), G.place(arg, 'arg'), (N, C, H, W))
    assert G.unwritten(dx) == 0
    assert torch.equal(_host(dx), R.rne(dx_ref, dt)), 'dx, tight operands'                           # [equal]


def test_maxpool_grid_stride_laps(gpu):
    """2 119 936 output chunks on the 8192-block cap (the forward's second lap) and four laps of the backward; the float64
    reference runs on the device."""
    ops = _ops()
    dt, N, C, H, W = R.MP_LAP
    v, cat, dy = R.mp_operands_np(dt, N, C, H, W)
    x64 = R.mp_assemble(torch.from_numpy(v).to(gpu), torch.from_numpy(cat).to(gpu))
    xd = R.nhwc(x64, R.TDT[dt])
    assert R.bits_equal(xd.double(), x64)
    y_ref, code_ref = R.maxpool_fwd(x64)
    del x64
    y, arg = ops.maxpool_fwd(xd)
    assert R.bits_equal(y.double(), y_ref), 'pooled values'                                          # [equal]
    assert torch.equal(arg, code_ref.permute(0, 2, 3, 1)), 'window codes'                           # [equal]
    del y, y_ref, xd
    dy64 = torch.from_numpy(dy).to(gpu).double()
    dyd = R.nhwc(dy64, R.TDT[dt])
    assert torch.equal(dyd.double(), dy64)
    dx_ref = R.maxpool_bwd(dy64, code_ref, (N, C, H, W))
    assert float(R.maxpool_bwd(dy64.abs(), code_ref, (N, C, H, W)).max()) <= 256          # every partial sum is a bf16 integer
    dx = ops.maxpool_bwd(dyd, arg, (N, C, H, W))
    assert torch.equal(dx.double(), R.rne(dx_ref, dt)), 'dx'                                         # [equal]


# ================================================================ B. layout
@pytest.mark.parametrize('dt', R.DTS)
@pytest.mark.parametrize('C,cpad', R.TO_NHWC_C)
def test_to_nhwc(gpu, dt, C, cpad):
    ops = _ops()
    for N in (1, 3):
        for H, W in R.TO_NHWC_MAPS:
            x = R.layout_values('to_nhwc', N, C, H, W)
            ref = R.to_nhwc(x, dt, cpad)
            _pitch(W, ref.shape[1], dt)
            out = _run(ops, 'to_nhwc %s' % ((N, C, H, W, cpad),), ops.to_nhwc, G.place(x.to(gpu), 'x'), R.TDT[dt], cpad)
            assert _written(out, ref)
            assert ops.is_nhwc(out) and out.dtype == R.TDT[dt]
            assert R.bits_equal(out.cpu().contiguous(), ref), (N, H, W)                              # [equal], pads +0.0


def test_to_nhwc_grid_stride_lap(gpu):
    """4 456 448 chunks on the 16384-block cap (f32)."""
    ops = _ops()
    N, C, cpad, H, W = R.TO_NHWC_LAP
    x = R.layout_values('to_nhwc lap', N, C, H, W).to(gpu)
    out = ops.to_nhwc(x, torch.float32)
    ref = torch.zeros(N, cpad, H, W, device=gpu)
    ref[:, :C] = x
    assert tuple(out.shape) == (N, cpad, H, W) and ops.is_nhwc(out)
    assert R.bits_equal(out.contiguous(), ref)                                                       # [equal]


@pytest.mark.parametrize('dt', R.DTS)
def test_to_nchw_f32(gpu, dt):
    ops = _ops()
    for N in (1, 3):
        for C in R.TO_NCHW_C:
            for H, W in R.TO_NCHW_MAPS:
                x = R.nhwc(R.layout_values('to_nchw', N, C, H, W), R.TDT[dt])
                _pitch(W, C, dt)
                xd = G.place(x.to(gpu), 'x')
                assert ops.is_nhwc(xd)
                y = _run(ops, 'to_nchw_f32 %s' % ((N, C, H, W),), ops.to_nchw_f32, xd)
                assert _written(y, R.to_nchw_f32(x))
                assert y.dtype == torch.float32 and y.is_contiguous()
                assert R.bits_equal(y.cpu(), R.to_nchw_f32(x)), (N, C, H, W)                         # [equal]
                back = _run(ops, 'to_nhwc back %s' % ((N, C, H, W),), ops.to_nhwc, y, R.TDT[dt])
                padded = torch.zeros(back.shape)
                padded[:, :C] = x.float()
                assert _written(back, padded)
                assert R.bits_equal(back[:, :C].cpu().contiguous(), x.contiguous()), (N, C, H, W)    # [equal] round trip
                assert not bool(back[:, C:].ne(0).any())


@pytest.mark.parametrize('dt', R.DTS)
@pytest.mark.parametrize('N,H,W', R.S2D_SHAPES)
def test_to_nhwc_s2d(gpu, dt, N, H, W):
    # No grid-stride lap case: the 16384-block cap equals the B = 64 batch at 512 pixels (64 * 256 * 256 / 256 blocks), so an
    # input that laps would be more than 200 MB of fp32 image; the loop is the one test_to_nhwc_grid_stride_lap walks.
    ops = _ops()
    x = R.layout_values('s2d', N, 3, H, W)
    _pitch(W, 3, 'f32')                  # an image row of the NCHW source; the output's W/2 * 16 elements are no wider
    out = _run(ops, 'to_nhwc_s2d %s' % ((N, H, W),), ops.to_nhwc_s2d, G.place(x.to(gpu), 'x'), R.TDT[dt])
    assert _written(out, R.s2d(x, dt))
    assert ops.is_nhwc(out) and tuple(out.shape) == (N, 16, H // 2, W // 2)
    assert R.bits_equal(out.cpu().contiguous(), R.s2d(x, dt))                                        # [equal]


@pytest.mark.parametrize('dt', R.DTS)
@pytest.mark.parametrize('Co', R.STEM_CO)
def test_stem_pack_and_unpack(gpu, dt, Co):
    ops = _ops()
    w = R.layout_values('stem w', Co, 7, 7, 3)
    out = _run(ops, 'stem_s2d_pack %d' % Co, ops.stem_s2d_pack, G.place(w.reshape(-1).to(gpu), 'w'), R.TDT[dt])
    ref = R.stem_pack(w.double()).float().to(R.TDT[dt])
    assert _written(out, ref)
    assert R.bits_equal(out.cpu().view(Co, 4, 4, 16), ref)                                           # [equal]
    if dt == 'f32':                     # the gradient is fp32 whatever the activation type
        gs = R.int_values('stem gs', -8, 8, Co, 4, 4, 16)
        prior = R.int_values('stem prior', -8, 8, Co, 7, 7, 3)
        for acc in (False, True):
            g = _f32(prior, gpu, 'g') if acc else G.empty((Co, 7, 7, 3), torch.float32, gpu, 'g')
            _run(ops, 'stem_s2d_unpack_grad %d acc=%d' % (Co, acc), ops.stem_s2d_unpack_grad, _f32(gs, gpu, 'gs'), g, acc)
            assert G.unwritten(g) == 0
            assert torch.equal(g.double().cpu(), R.stem_unpack(gs, prior if acc else None))         # [equal]


# ================================================================ C. pw21
def _pw_dev(c, gpu):
    dt = c['dt']
    _pitch(c['W'], c['C'], dt)
    d = dict(x=_feat(c['x'], dt, gpu, 'x'), res=_feat(c['res'], dt, gpu, 'res'), y=_f32(c['y'], gpu, 'y'))
    for k in ('wck', 'wkc', 'bias_k', 'bias_c', 'prior_w'):
        d[k] = _f32(c[k], gpu, k)
    d['wck_t'], d['wkc_t'] = _f32(c['wck'].t().contiguous(), gpu, 'wck_t'), _f32(c['wkc'].t().contiguous(), gpu, 'wkc_t')
    return d


@pytest.mark.parametrize('case', R.C2K_CASES, ids=R.case_id)
def test_pw_c2k(gpu, case):
    """Partial 64-pixel tiles, one and three images, both weight layouts, with and without bias; C = 512 (bf16) takes the
    dynamic-LDS path above 64 KB."""
    ops = _ops()
    dt, C, K = case
    for N in R.PW_N:
        for HW in R.PW_HW:
            c = R.pw_case(dt, N, C, K, HW)
            R.check_exact_pw(c)
            d = _pw_dev(c, gpu)
            for bias in (False, True):
                ref = R.pw_c2k(c['x'], c['wkc'], c['bias_k'] if bias else None)
                b = d['bias_k'] if bias else None
                y = _run(ops, 'pw_c2k %s' % ((dt, N, C, K, HW, bias),), ops.pw_c2k, d['x'], d['wkc'], b, K)
                assert G.unwritten(y) == 0
                assert y.dtype == torch.float32 and y.is_contiguous()
                assert torch.equal(y.double().cpu(), ref), (N, HW, bias, '[K][C]')                   # [equal]
                y = _run(ops, 'pw_c2k [C][K] %s' % ((dt, N, C, K, HW, bias),), ops.pw_c2k, d['x'], d['wkc_t'], b, K, w_transposed=True)
                assert G.unwritten(y) == 0
                assert torch.equal(y.double().cpu(), ref), (N, HW, bias, '[C][K]')                   # [equal]


@pytest.mark.parametrize('case', R.K2C_CASES, ids=R.case_id)
def test_pw_k2c(gpu, case):
    """Ragged last channel group (C = 24, and 264 for a second block), partial pixel tiles, bias / residual / scale_dev on and
    off, both weight layouts.  The bf16 results are real roundings (check_exact_pw counts the exact ties)."""
    ops = _ops()
    dt, C, K = case
    half, one = G.place(torch.tensor(0.5, device=gpu), 'scale_dev 0.5'), G.place(torch.tensor(1.0, device=gpu), 'scale_dev 1')
    for N in R.PW_N:
        for HW in R.PW_HW:
            c = R.pw_case(dt, N, C, K, HW)
            t = R.check_exact_pw(c)
            assert t >= 1 or not R.needs_tie(dt, N, C, K, HW)
            d = _pw_dev(c, gpu)
            for bias, res, scale in R.K2C_MODES:
                ref = R.pw_k2c(c['y'], c['wck'], c['bias_c'] if bias else None, c['res'] if res else None, scale)
                kw = dict(residual=d['res'] if res else None, scale_dev={None: None, 0.5: half, 1.0: one}[scale])
                b = d['bias_c'] if bias else None
                label = 'pw_k2c %s' % ((dt, N, C, K, HW, bias, res, scale),)
                out = _run(ops, label, ops.pw_k2c, d['y'], d['wck'], b, C, R.TDT[dt], **kw)
                assert G.unwritten(out) == 0
                assert out.dtype == R.TDT[dt] and ops.is_nhwc(out)
                assert torch.equal(_host(out), R.rne(ref, dt)), (N, HW, bias, res, scale, '[C][K]')   # [equal]
                out = _run(ops, label + ' [K][C]', ops.pw_k2c, d['y'], d['wck_t'], b, C, R.TDT[dt], w_transposed=True, **kw)
                assert G.unwritten(out) == 0
                assert torch.equal(_host(out), R.rne(ref, dt)), (N, HW, bias, res, scale, '[K][C]')   # [equal]


def _k2c_stats(ops, gpu, dt, C, N, HW, counts):
    K = 21
    c = R.pw_case(dt, N, C, K, HW)
    R.check_exact_pw(c)
    d = _pw_dev(c, gpu)
    ref = R.rne(R.pw_k2c(c['y'], c['wck'], c['bias_c'], c['res']), dt)
    label = 'pw_k2c_stats %s' % ((dt, N, C, HW),)
    plain = _run(ops, label + ' plain', ops.pw_k2c, d['y'], d['wck'], d['bias_c'], C, R.TDT[dt], residual=d['res'])
    out, (partial, ns) = _run(ops, label, ops.pw_k2c_stats, d['y'], d['wck'], d['bias_c'], C, R.TDT[dt], residual=d['res'])
    assert G.unwritten(plain) == 0 and G.unwritten(out) == 0
    assert torch.equal(out, plain)                                                                   # [equal]
    assert torch.equal(_host(out), ref)                                                              # [equal]
    assert ns == N * ((HW + 63) // 64)
    assert partial.numel() == ns * C * 3 and G.unwritten(partial) == 0           # ns_max slices, the last of each image ragged
    p = partial[:ns * C * 3].view(ns, C, 3).double().cpu()
    st = R.slice_stats(ref, HW)                           # of the STORED values
    assert torch.equal(p[:, :, 0], st[:, :, 0]) and set(p[:, :, 0].unique().tolist()) == counts          # [equal]
    assert float((p[:, :, 1] - st[:, :, 1]).abs().max()) <= 1e-5 * float(st[:, :, 1].abs().max() + 1)    # [stats]
    assert float((p[:, :, 2] - st[:, :, 2]).abs().max()) <= 1e-4 * float(st[:, :, 2].abs().max() + 1)    # [stats]


@pytest.mark.parametrize('case', R.K2C_STATS_CASES, ids=R.case_id)
def test_pw_k2c_stats(gpu, case):
    dt, C, N = case
    _k2c_stats(_ops(), gpu, dt, C, N, 100, {64.0, 36.0})


@pytest.mark.parametrize('HW', R.PW_EDGE_HW)
@pytest.mark.parametrize('dt,C', [(dt, C) for dt in R.DTS for C in (24, 264)])
def test_pw_k2c_stats_two_images_at_the_tile_edges(gpu, dt, C, HW):
    """N = 2 at H*W = 1, 63, 64, 65: the partials buffer has exactly ns_max slices and the last slice of each image holds 1, 63,
    64 or 1 pixels."""
    _k2c_stats(_ops(), gpu, dt, C, 2, HW, {float(HW)} if HW <= 64 else {64.0, float(HW - 64)})


@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=R.case_id)
def test_pw_wgrad(gpu, case):
    """Ragged last channel block (C = 24, 264), K other than 21, both layouts of dw, = and +=; the N = 9, 64 x 64 case gives 288
    slices of two 64-pixel groups each."""
    ops = _ops()
    dt, C, K, N, HW = case
    c = R.pw_case(dt, N, C, K, HW)
    R.check_exact_pw(c)
    _pitch(c['W'], C, dt)
    x, y = _feat(c['x'], dt, gpu, 'x'), _f32(c['y'], gpu, 'y')
    for acc in (False, True):
        ref = R.pw_wgrad(c['x'], c['y'], c['prior_w'] if acc else None)
        for kc in (True, False):
            prior = c['prior_w'] if kc else c['prior_w'].t().contiguous()
            dw = _f32(prior, gpu, 'dw') if acc else G.empty(prior.shape, torch.float32, gpu, 'dw')
            _run(ops, 'pw_wgrad %s acc=%d kc=%d' % (case, acc, kc), ops.pw_wgrad, x, y, dw, kc, acc)      # workspace: exactly
            assert G.unwritten(dw) == 0                                                  # mi355_pw_wgrad_workspace bytes
            got = dw.double().cpu()
            assert torch.equal(got if kc else got.t(), ref), (acc, kc)                               # [equal]


@pytest.mark.parametrize('case', R.ROWSUM_CASES, ids=R.case_id)
def test_hm_rowsum(gpu, case):
    ops = _ops()
    N, K, HW = case
    c = R.rowsum_case(N, K, HW)
    R.check_exact_rowsum(c)
    _pitch(c['y'].shape[3], 1, 'f32')
    y = _f32(c['y'], gpu, 'y')
    for acc in (False, True):
        out = _f32(c['prior'], gpu, 'out') if acc else G.empty((K,), torch.float32, gpu, 'out')
        _run(ops, 'hm_rowsum %s acc=%d' % (case, acc), ops.hm_rowsum, y, out, acc)       # workspace: exactly N * K * 4 bytes
        assert G.unwritten(out) == 0
        assert torch.equal(out.double().cpu(), R.hm_rowsum(c['y'], c['prior'] if acc else None)), acc    # [equal]


# ================================================================ D. optimiser
def _sgd_run(ops, gpu, c, nesterov, wd, lowp, off=0, room=0):
    """Three steps on views [off : off + n] of buffers with `room` more elements; returns the whole buffers."""
    n = c['n']
    tot = n + room
    sent = 544.0
    P = torch.full((tot,), sent, device=gpu); P[off:off + n] = _f32(c['p'], gpu)
    B = torch.full((tot,), sent, device=gpu); B[off:off + n] = 0
    # the whole buffers sit in guards: with room = 0 the views end where the back flank begins
    P, B, Gr = G.place(P, 'p'), G.place(B, 'buf'), G.place(torch.full((tot,), sent, device=gpu), 'g')
    L = G.place(torch.full((tot,), sent, dtype=torch.bfloat16, device=gpu), 'p_lowp') if lowp else None
    lr_dev = G.place(torch.zeros((), device=gpu), 'lr_dev')
    for i, (g, lr) in enumerate(zip(c['g'], R.SGD_LRS)):
        Gr[off:off + n] = _f32(g, gpu)
        lr_dev.fill_(lr)
        _run(ops, 'sgd_nesterov n=%d step %d' % (n, i), ops.sgd_nesterov, P[off:off + n], Gr[off:off + n], B[off:off + n], lr_dev,
             R.SGD_MU, wd, nesterov, L[off:off + n] if lowp else None)
    return P, B, L


@pytest.fixture(scope='module')
def sgd_refs():
    """n -> the operands, (nesterov, wd) -> the float64 result: each computed once per module."""
    return {}


def _sgd_ref(refs, n, nesterov, wd):
    if n not in refs:
        refs[n] = dict(c=R.sgd_case(n))
    e = refs[n]
    if (nesterov, wd) not in e:
        e[(nesterov, wd)] = R.check_exact_sgd(e['c'], nesterov, wd)
    return e['c'], e[(nesterov, wd)]


@pytest.mark.parametrize('case', R.SGD_CASES, ids=R.case_id)
def test_sgd_three_steps(gpu, sgd_refs, case):
    """The scalar tail alone (n < 4), every n % 4, the second grid lap, Nesterov and plain momentum, wd on and off, with and
    without the bf16 copy; lr changes between the steps through lr_dev."""
    ops = _ops()
    n, nesterov, wd = case
    c, (p_ref, buf_ref) = _sgd_ref(sgd_refs, n, nesterov, wd)
    for lowp in (False, True):
        P, B, L = _sgd_run(ops, gpu, c, nesterov, wd, lowp)
        assert torch.equal(P.double().cpu(), p_ref), 'p'                                             # [equal]
        assert torch.equal(B.double().cpu(), buf_ref), 'buf'                                         # [equal]
        if lowp:
            assert torch.equal(L.double().cpu(), R.rne(p_ref, 'bf16')), 'p_lowp'                     # [equal]


@pytest.mark.parametrize('n', [3, 1025])
def test_sgd_on_views_at_an_offset(gpu, sgd_refs, n):
    """Views [4 : 4 + n] of larger buffers, as FusedSGD.step passes for its runs: the elements outside stay untouched."""
    ops = _ops()
    c, (p_ref, buf_ref) = _sgd_ref(sgd_refs, n, True, 0.25)
    P, B, L = _sgd_run(ops, gpu, c, True, 0.25, True, off=4, room=12)
    assert torch.equal(P[4:4 + n].double().cpu(), p_ref)                                             # [equal]
    assert torch.equal(B[4:4 + n].double().cpu(), buf_ref)                                           # [equal]
    assert torch.equal(L[4:4 + n].double().cpu(), R.rne(p_ref, 'bf16'))                              # [equal]
    for t in (P, B, L):
        outside = torch.cat([t[:4], t[4 + n:]]).float().cpu()
        assert torch.equal(outside, torch.full((12,), 544.0)), 'outside the view'                    # [equal]


@pytest.mark.parametrize('dt', R.DTS)
@pytest.mark.parametrize('n', R.CAST_N)
def test_cast_f32(gpu, dt, n):
    ops = _ops()
    src = R.cast_values(n)
    dst = G.place(torch.full((n + 3,), 544.0, dtype=R.TDT[dt], device=gpu), 'dst')
    _run(ops, 'cast_f32 %s n=%d' % (dt, n), ops.cast_f32, G.place(src.to(gpu), 'src'), dst[:n])
    tight = G.empty((n,), R.TDT[dt], gpu, 'dst, tight')               # ... and a destination that ends at its flank
    _run(ops, 'cast_f32 tight %s n=%d' % (dt, n), ops.cast_f32, G.place(src.to(gpu), 'src'), tight)
    assert _written(tight, src)
    assert R.bits_equal(tight.cpu(), src.to(R.TDT[dt]))                                              # [equal], NaN by position
    assert R.bits_equal(dst[:n].cpu(), src.to(R.TDT[dt]))                                            # [equal], NaN by position
    assert torch.equal(dst[n:].float().cpu(), torch.full((3,), 544.0))                               # [equal]


# ================================================================ F. a workspace one byte short: nothing launches
def _abi_refuses(ops, name, args, ws, out):
    """The entry point returns the workspace error ahead of its launches: the launch log stays empty, the output and the
    workspace keep their fill and no flank changes."""
    import mi355
    ops.prof_reset(); ops.prof_enable(2)
    try:
        rc = getattr(mi355.load(), name)(*args)
        torch.cuda.synchronize()
        assert rc == -3                                  # MI355_EWORKSPACE
        assert 'workspace too small' in mi355.load().mi355_last_error().decode()
        assert ops.prof_launches() == []
    finally:
        ops.prof_enable(0); ops.prof_reset()
    G.check(name + ', workspace one byte short')
    assert G.unwritten(out) == out.numel() * 4 and G.unwritten(ws.view(torch.float32)) == ws.numel()


@pytest.mark.parametrize('dt', R.DTS)
def test_pw_wgrad_workspace_one_byte_short(gpu, dt):
    import mi355
    from mi355 import dtype_code, ptr, stream_ptr
    ops = _ops()
    N, C, K, HW = 3, 24, 21, 64
    c = R.pw_case(dt, N, C, K, HW)
    _pitch(c['W'], C, dt)
    x, y = _feat(c['x'], dt, gpu, 'x'), _f32(c['y'], gpu, 'y')
    need = mi355.load().mi355_pw_wgrad_workspace(N, HW, C, K)
    assert need == 3 * K * C * 4                          # three slices of 64 pixels
    with G.window(ops, 'pw_wgrad ws'):
        ws = ops.workspace(need, gpu)
    dw = G.empty((K, C), torch.float32, gpu, 'dw')
    _abi_refuses(ops, 'mi355_pw_wgrad', (ptr(x), ptr(y), ptr(dw), 1, 0, N, HW, C, K, dtype_code(R.TDT[dt]), ptr(ws), need - 1, stream_ptr()), ws, dw)
    # ... and with exactly `need` bytes it runs
    mi355.call('mi355_pw_wgrad', ptr(x), ptr(y), ptr(dw), 1, 0, N, HW, C, K, dtype_code(R.TDT[dt]), ptr(ws), need, stream_ptr())
    torch.cuda.synchronize()
    G.check('pw_wgrad, exact workspace')
    assert G.unwritten(dw) == 0 and torch.equal(dw.double().cpu(), R.pw_wgrad(c['x'], c['y']))     # [equal]


def test_hm_rowsum_workspace_one_byte_short(gpu):
    import mi355
    from mi355 import ptr, stream_ptr
    ops = _ops()
    N, K, HW = 3, 21, 255
    c = R.rowsum_case(N, K, HW)
    _pitch(c['y'].shape[3], 1, 'f32')
    y = _f32(c['y'], gpu, 'y')
    need = N * K * 4
    with G.window(ops, 'hm_rowsum ws'):
        ws = ops.workspace(need, gpu)
    out = G.empty((K,), torch.float32, gpu, 'out')
    _abi_refuses(ops, 'mi355_hm_rowsum', (ptr(y), ptr(out), 0, N, K, HW, ptr(ws), need - 1, stream_ptr()), ws, out)
    mi355.call('mi355_hm_rowsum', ptr(y), ptr(out), 0, N, K, HW, ptr(ws), need, stream_ptr())
    torch.cuda.synchronize()
    G.check('hm_rowsum, exact workspace')
    assert G.unwritten(out) == 0 and torch.equal(out.double().cpu(), R.hm_rowsum(c['y']))          # [equal]


# ================================================================ E. wrapper checks: nothing launches
def test_wrappers_refuse_what_the_kernels_cannot_index(gpu):
    """Every case raises Mi355Error before any launch: in the wrapper, or in the host half of the entry point, which returns
    its error ahead of the launch.  Only allocations happen here (torch.empty launches nothing)."""
    from mi355 import Mi355Error
    ops = _ops()
    bf, f32 = torch.bfloat16, torch.float32
    e = lambda *s, dt=f32, dev=gpu: torch.empty(*s, dtype=dt, device=dev)
    nhwc = lambda N, C, H, W, dt=bf: ops.nhwc_empty(N, C, H, W, dt, gpu)
    cpu_nhwc = lambda N, C, H, W, dt=bf: ops.nhwc_empty(N, C, H, W, dt, torch.device('cpu'))
    x, dy, arg = nhwc(2, 16, 6, 6), nhwc(2, 16, 3, 3), e(2, 3, 3, 16, dt=torch.uint8)
    f, hm, w, bk, bc = nhwc(1, 256, 8, 8), e(1, 21, 8, 8), e(21 * 256), e(21), e(256)
    cases = {
        # --- the wrappers' own checks
        'maxpool_fwd cpu': (lambda: ops.maxpool_fwd(cpu_nhwc(2, 16, 6, 6)), 'CUDA/HIP'),
        'maxpool_fwd nchw': (lambda: ops.maxpool_fwd(e(2, 16, 6, 6, dt=bf)), 'channels_last'),
        'maxpool_bwd cpu dy': (lambda: ops.maxpool_bwd(cpu_nhwc(2, 16, 3, 3), arg, (2, 16, 6, 6)), 'CUDA/HIP'),
        'maxpool_bwd cpu arg': (lambda: ops.maxpool_bwd(dy, e(2, 3, 3, 16, dt=torch.uint8, dev='cpu'), (2, 16, 6, 6)), 'CUDA/HIP'),
        'maxpool_bwd nchw dy': (lambda: ops.maxpool_bwd(e(2, 16, 3, 3, dt=bf), arg, (2, 16, 6, 6)), 'channels_last'),
        'maxpool_bwd dy shape': (lambda: ops.maxpool_bwd(nhwc(2, 16, 3, 2), arg, (2, 16, 6, 6)), 'the launch indexes'),
        'maxpool_bwd dy of another input': (lambda: ops.maxpool_bwd(dy, arg, (2, 16, 8, 8)), 'the launch indexes'),
        'maxpool_bwd short arg': (lambda: ops.maxpool_bwd(dy, e(2 * 3 * 3 * 16 - 1, dt=torch.uint8), (2, 16, 6, 6)), 'buffer of'),
        'maxpool_bwd int32 arg': (lambda: ops.maxpool_bwd(dy, e(2, 3, 3, 16, dt=torch.int32), (2, 16, 6, 6)), 'uint8'),
        'pw_c2k cpu': (lambda: ops.pw_c2k(cpu_nhwc(1, 256, 8, 8), w, bk, 21), 'CUDA/HIP'),
        'pw_c2k cpu w': (lambda: ops.pw_c2k(f, e(21 * 256, dev='cpu'), bk, 21), 'CUDA/HIP'),
        'pw_c2k nchw': (lambda: ops.pw_c2k(e(1, 256, 8, 8, dt=bf), w, bk, 21), 'channels_last'),
        'pw_c2k short w': (lambda: ops.pw_c2k(f, e(21 * 256 - 1), bk, 21), 'buffer of'),
        'pw_c2k short bias': (lambda: ops.pw_c2k(f, w, e(20), 21), 'buffer of'),
        'pw_k2c cpu': (lambda: ops.pw_k2c(e(1, 21, 8, 8, dev='cpu'), w, bc, 256, bf), 'CUDA/HIP'),
        'pw_k2c strided y': (lambda: ops.pw_k2c(e(1, 21, 8, 16)[:, :, :, ::2], w, bc, 256, bf), 'contiguous fp32'),
        'pw_k2c bf16 y': (lambda: ops.pw_k2c(e(1, 21, 8, 8, dt=bf), w, bc, 256, bf), 'contiguous fp32'),
        'pw_k2c short w': (lambda: ops.pw_k2c(hm, e(21 * 256 - 1), bc, 256, bf), 'buffer of'),
        'pw_k2c short bias': (lambda: ops.pw_k2c(hm, w, e(255), 256, bf), 'buffer of'),
        'pw_k2c nchw residual': (lambda: ops.pw_k2c(hm, w, bc, 256, bf, residual=e(1, 256, 8, 8, dt=bf)), 'channels_last'),
        'pw_k2c residual of another map': (lambda: ops.pw_k2c(hm, w, bc, 256, bf, residual=nhwc(1, 256, 8, 7)), 'the launch indexes'),
        'pw_k2c_stats cpu': (lambda: ops.pw_k2c_stats(e(1, 21, 8, 8, dev='cpu'), w, bc, 256, bf), 'CUDA/HIP'),
        'pw_k2c_stats strided y': (lambda: ops.pw_k2c_stats(e(1, 21, 8, 16)[:, :, :, ::2], w, bc, 256, bf), 'contiguous fp32'),
        'pw_k2c_stats short w': (lambda: ops.pw_k2c_stats(hm, e(21 * 256 - 1), bc, 256, bf), 'buffer of'),
        'pw_k2c_stats short bias': (lambda: ops.pw_k2c_stats(hm, w, e(255), 256, bf), 'buffer of'),
        'pw_k2c_stats nchw residual': (lambda: ops.pw_k2c_stats(hm, w, bc, 256, bf, residual=e(1, 256, 8, 8, dt=bf)), 'channels_last'),
        'pw_wgrad cpu': (lambda: ops.pw_wgrad(cpu_nhwc(1, 256, 8, 8), hm, w, True, False), 'CUDA/HIP'),
        'pw_wgrad nchw': (lambda: ops.pw_wgrad(e(1, 256, 8, 8, dt=bf), hm, w, True, False), 'channels_last'),
        'pw_wgrad strided y': (lambda: ops.pw_wgrad(f, e(1, 21, 8, 16)[:, :, :, ::2], w, True, False), 'contiguous fp32'),
        'pw_wgrad short dw': (lambda: ops.pw_wgrad(f, hm, e(21 * 256 - 1), True, False), 'buffer of'),
        # --- refusals of the host code, each ahead of its launch
        'pw_c2k K = 33': (lambda: ops.pw_c2k(f, e(33 * 256), e(33), 33), 'unsupported shape'),
        'pw_k2c K = 33': (lambda: ops.pw_k2c(e(1, 33, 8, 8), e(33 * 256), bc, 256, bf), 'unsupported shape'),
        'pw_wgrad K = 33': (lambda: ops.pw_wgrad(f, e(1, 33, 8, 8), e(33 * 256), True, False), 'unsupported shape'),
        'pw_c2k C % 8': (lambda: ops.pw_c2k(nhwc(1, 12, 8, 8), e(21 * 12), bk, 21), 'unsupported shape'),
        'pw_k2c C % 4': (lambda: ops.pw_k2c(hm, e(21 * 6), e(6), 6, f32), 'unsupported shape'),
        'maxpool_fwd C % 8': (lambda: ops.maxpool_fwd(nhwc(1, 12, 6, 6)), 'bad args'),
        'pw_wgrad H*W = 100': (lambda: ops.pw_wgrad(nhwc(1, 256, 10, 10), e(1, 21, 10, 10), w, True, False), 'multiple of 64'),
        'pw_c2k f32 C = 512': (lambda: ops.pw_c2k(nhwc(1, 512, 8, 8, f32), e(21 * 512), bk, 21), 'too large'),
        'sgd view at offset 1': (lambda: ops.sgd_nesterov(e(101)[1:], e(101)[1:], e(101)[1:], e(()), 0.5, 0.25, True), '16-byte aligned'),
        'to_nhwc_s2d odd extent': (lambda: ops.to_nhwc_s2d(e(1, 3, 6, 7)), 'even extents'),
    }
    for name, (call, what) in cases.items():
        with pytest.raises(Mi355Error, match=what):
            call()
