"""The BatchNorm kernels (csrc/bn.hip) bit for bit on exact integer operands (tests/bn_exact_ref.py).

Every comparison here is one of three kinds, named next to it:
  [equal]  torch.equal with the float64 reference (rounded to nearest even into the activation type where that is bf16);
  [bound]  the derived bound B of the roundings that remain (ragged row counts, the forward's apply pass);
  [stats]  the project's own tightest statistics tolerances (test_conv_fwd_concat_k): rtol 1e-5 / atol 1e-6 on means,
           rtol 2e-5 / atol 1e-6 on invstd and variances.
Operands are plain torch casts of exact values, copied into 0xFF-filled guard buffers (tests/guarded.py); every call runs inside
a guard window, so the tensors the wrappers allocate (y, dx, dres, mean, invstd, ss, coeff, masks) and the workspace -- of exactly
mi355_bn_workspace bytes -- are guard buffers too: a store outside a result changes a flank, an element a launch skipped stays a
NaN, and a chunk load past an operand reads NaN.  The float64 references are the functions test_bn_exact_cpu.py holds against
torch on the CPU, evaluated with torch's float64 on the device so that the 16 M-element cases stay within seconds.  The form
of the backward that ran (reduce + finalize + apply, or the one-launch LDS-resident kernel) is read from the launch log, so a
silent fallback cannot make two runs of one path pass as two paths.  Nothing here provokes a give-up of the resident kernel.

Section i runs the same kernels with a NaN, a +Inf or a -Inf in one operand (tests/nonfinite_ref.py): a special stays inside its
channel, a masked one is dropped by a select and changes no bit, and the mask of a NaN forward output lets the gradient through."""
import pytest
import torch

import bn_exact_ref as R
import guarded as G
import nonfinite_ref as NF

pytestmark = pytest.mark.gpu

MEAN_TOL = dict(rtol=1e-5, atol=1e-6)
VAR_TOL = dict(rtol=2e-5, atol=1e-6)


def _ops():
    import mi355
    from mi355 import ops
    mi355.load()
    return ops


@pytest.fixture(scope='module', autouse=True)
def launch_log(gpu):
    ops = _ops()
    assert ops.bn_resident_timeouts() == 0
    ops.prof_enable(2)          # level 2: every logged family (BatchNorm launches are family 1)
    yield
    ops.prof_enable(0)
    _HOLD.clear()
    assert ops.bn_resident_timeouts() == 0


@pytest.fixture(autouse=True)
def guards():
    """No guard buffer of one test is charged to the next (tests/guarded.py); the operands _HOLD keeps stay under watch."""
    yield
    torch.cuda.synchronize()
    G.check('end of test')


_HOLD = {}       # the operands and references of the (rows, C) in hand: consecutive cases of one shape share them


def _case(gpu, rows, C, mirror=False):
    key = (rows, C, mirror)
    if key not in _HOLD:
        _HOLD.clear()
        c = R.make_case(rows, C, device=gpu, mirror=mirror)
        G.row_pitch(C * 4)          # the widest row of the case (fp32): the flanks of its vectors and of the workspace hold 256 of them
        c['dev'], c['ref'] = {}, {}
        _HOLD[key] = c
    return _HOLD[key]


def _put(mat, dt):
    """A [rows][C] matrix as a channels_last feature map of type dt, inside a guard buffer (tests/guarded.py)."""
    return G.place(R.nchw(mat).to(R.TDT[dt]).contiguous(memory_format=torch.channels_last), 'feature map')


def _vec(t, what='vector'):
    """A per-channel vector, a mask, a partials buffer or an fp8 record, inside a guard buffer."""
    return G.place(t.contiguous(), what)


def _whole(what, *ts):
    """The launch wrote all of each tensor: no element is still the guard fill (a NaN no result here may be)."""
    for t in ts:
        if t is not None:
            assert t.data_ptr() % G.BOUNDARY == G.START, '%s: not in a guard buffer' % what          # (the allocator's own blocks start on the boundary)
            assert G.unwritten(t) == 0, '%s: %d bytes were never written' % (what, G.unwritten(t))


def _dev(c, dt, residual=True):
    """The case's operands in the activation type (plain torch casts of exact values) and its fp32 per-channel vectors."""
    key = (dt, residual)
    if key not in c['dev']:
        y = R.fwd_y(c, residual, True)
        d = dict(x=_put(c['x'], dt), dy=_put(c['dy'], dt), res=_put(c['res'], dt), y=_put(y, dt), mask=_vec(R.pack_mask(y > 0, R.PER[dt]), 'mask'))
        for k in ('gamma', 'beta', 'mean', 'invstd'):
            d[k] = _vec(c[k].float(), k)
        for k in ('x', 'dy', 'res', 'y'):
            assert torch.equal(R.rows_of(d[k]).double(), c[k] if k != 'y' else y)          # the casts lost nothing
        c['dev'][key] = d
    return c['dev'][key]


def _ref(c, source, residual=True):
    key = (source if source != 3 else 1, residual)
    if key not in c['ref']:
        mask = None if source == 0 else (c['ypre'] > 0 if source == 2 else R.fwd_y(c, residual, True) > 0)
        c['ref'][key] = R.bn_bwd(c, mask)
    return c['ref'][key]


def _labels(ops, fn):
    """fn() with the labels of its launches, inside a guard window: every tensor the wrapper allocates and its workspace are
    0xFF-filled buffers between 0xFF flanks, and no flank byte -- theirs or an operand's -- may have changed afterwards."""
    ops.prof_reset()
    with G.window(ops, 'bn call'):
        out = fn()
    torch.cuda.synchronize()
    labels = [l['label'] for l in ops.prof_launches()]
    G.check(' | '.join(labels))
    return out, labels


def _backward(ops, c, dt, form, relu, dres, acc, partial=None, q8=None, residual=True):
    """One mi355_bn_bwd in the forced form: (dx, dres, dgamma, dbeta, launch labels).  dgamma / dbeta start from integer priors
    (accumulate) or from a sentinel the kernel must overwrite."""
    d = _dev(c, dt, residual)
    C, gpu = c['C'], c['x'].device
    dg = _vec(R.int_prior(C, 'dg', gpu).float() if acc else torch.full((C,), 777.0, device=gpu), 'dgamma')
    db = _vec(R.int_prior(C, 'db', gpu).float() if acc else torch.full((C,), -777.0, device=gpu), 'dbeta')
    prev = ops.bn_set_resident(1 if form == 'resident' else 0)
    try:
        (dx, dr), labels = _labels(ops, lambda: ops.bn_bwd(d['dy'], d['x'], d['y'] if relu == 1 else None, d['gamma'], d['mean'], d['invstd'],
                                                          dg, db, acc, relu != 0, dres, beta=d['beta'], partial=partial,
                                                          relu_mask=d['mask'] if relu == 3 else None, q8=q8))
    finally:
        ops.bn_set_resident(prev)
    _whole('dx / dres', dx, dr)
    return dx, dr, dg, db, labels


def _assert_form(labels, form):
    if form == 'resident':
        assert labels and all(l.startswith('bn_bwd_res ') for l in labels), labels
    else:
        assert [l.split(' ')[0] for l in labels] == ['bn_bwd_reduce', 'bn_bwd_finalize', 'bn_bwd_apply'], labels


def _assert_sums(c, r, dr, dg, db, dres, acc, dt):
    gpu = c['x'].device
    pg = R.int_prior(c['C'], 'dg', gpu) if acc else 0
    pb = R.int_prior(c['C'], 'db', gpu) if acc else 0
    assert torch.equal(dg.double(), r['s2'] + pg), 'dgamma'           # [equal]
    assert torch.equal(db.double(), r['s1'] + pb), 'dbeta'            # [equal]
    if dres:
        assert torch.equal(R.rows_of(dr).double(), r['dres']), 'dres'      # [equal]
    else:
        assert dr is None


# ---------------------------------------------------------------- a. backward, bit for bit
@pytest.mark.parametrize('case', R.bwd_cases(R.BWD_SHAPES, R.BWD_MODES), ids=R.case_id)
def test_backward_bit_for_bit(gpu, case):
    rows, C, dt, form, relu, dres, acc = case
    ops = _ops()
    c = _case(gpu, rows, C)
    r = _ref(c, relu)
    dx, dr, dg, db, labels = _backward(ops, c, dt, form, relu, dres, acc)
    _assert_form(labels, form)
    _assert_sums(c, r, dr, dg, db, dres, acc, dt)
    assert torch.equal(R.rows_of(dx).double(), R.rne(r['dx'], dt)), 'dx'       # [equal]
    assert ops.bn_resident_timeouts() == 0


# ---------------------------------------------------------------- b. backward, ragged row counts
@pytest.mark.parametrize('case', R.bwd_cases(R.RAGGED_SHAPES, R.RAGGED_MODES), ids=R.case_id)
def test_backward_ragged_rows(gpu, case):
    rows, C, dt, form, relu, dres, acc = case
    ops = _ops()
    c = _case(gpu, rows, C)
    r = _ref(c, relu)
    dx, dr, dg, db, labels = _backward(ops, c, dt, form, relu, dres, acc)
    _assert_form(labels, form)
    _assert_sums(c, r, dr, dg, db, dres, acc, dt)
    # [bound] 1.0f / rows is rounded, so dx = k0 * (g - k1 - xhat * k2) is no longer exact.  k0, g and xhat are; the roundings
    # left are at most six: 1 / rows, s1 * inv, s2 * inv, xhat * k2 (or its FMA), g - k1, ... - xhat * k2.  Each is one unit of
    # roundoff 2^-24 relative to a value no larger than |g| + |k1| + |xhat * k2|; the factor 8 covers the six.
    B = R.dx_bound(r)
    got = R.rows_of(dx).double()
    if dt == 'f32':
        assert bool(((got - r['dx']).abs() <= B).all()), float(((got - r['dx']).abs() - B).max())
    else:
        assert bool((R.rne(r['dx'] - B, dt) <= got).all()) and bool((got <= R.rne(r['dx'] + B, dt)).all())
    assert ops.bn_resident_timeouts() == 0


# ---------------------------------------------------------------- c. mi355_bn_bwd_partials and the finalize loop edges
@pytest.mark.parametrize('case', R.BWD_PARTIAL_CASES, ids=R.case_id)
def test_backward_from_crafted_partials(gpu, case):
    ns, rows, C, dt, relu, dres, acc = case
    ops = _ops()
    c = _case(gpu, rows, C)
    r = _ref(c, relu)
    p = _vec(R.bwd_partials(r['s1'], r['s2'], ns, relu).float(), 'partials')
    dx, dr, dg, db, labels = _backward(ops, c, dt, 'three', relu, dres, acc, partial=(p, ns))
    _assert_sums(c, r, dr, dg, db, dres, acc, dt)
    assert torch.equal(R.rows_of(dx).double(), R.rne(r['dx'], dt)), 'dx'       # [equal]


# ---------------------------------------------------------------- d. forward statistics that notice one row
def _running_start(C, gpu):
    return R.int_prior(C, 'rm', gpu), R.int_prior(C, 'rv', gpu).abs() + 1


@pytest.mark.parametrize('updates', R.STAT_UPDATES)
@pytest.mark.parametrize('shape', R.STATS_SHAPES, ids=R.case_id)
def test_forward_statistics(gpu, shape, updates):
    rows, C, dt = shape
    ops = _ops()
    s = R.stats_case(rows, C, device=gpu)
    rm0, rv0 = _running_start(C, gpu)
    f = R.train_fwd(s['x'], s['gamma'], s['beta'], rm0=rm0, rv0=rv0, repeats=updates)
    rm, rv, nbt = _vec(rm0.float(), 'running_mean'), _vec(rv0.float(), 'running_var'), _vec(torch.full((), 5, dtype=torch.int64, device=gpu), 'nbt')
    x, gamma, beta = _put(s['x'], dt), _vec(s['gamma'].float(), 'gamma'), _vec(s['beta'].float(), 'beta')
    (y, mean, invstd), _ = _labels(ops, lambda: ops.bn_train_fwd(x, None, gamma, beta, rm, rv, nbt, R.EPS, R.MOMENTUM, False, stat_updates=updates))
    _whole('y / mean / invstd', y, mean, invstd)
    assert torch.allclose(mean.double(), f['mean'], **MEAN_TOL), float((mean.double() - f['mean']).abs().max())          # [stats]
    assert torch.allclose(invstd.double(), f['invstd'], **VAR_TOL), float((invstd.double() / f['invstd'] - 1).abs().max())   # [stats]
    assert int(nbt) == 5 + updates
    if updates == 0:
        assert torch.equal(rm, rm0.float()) and torch.equal(rv, rv0.float())          # [equal] the sentinels are untouched
    else:
        assert torch.allclose(rm.double(), f['rm'], **MEAN_TOL)       # [stats]
        assert torch.allclose(rv.double(), f['rv'], **VAR_TOL)        # [stats]


# ---------------------------------------------------------------- e. forward apply, eval forward and the mask bits
@pytest.mark.parametrize('res,relu', R.APPLY_MODES)
@pytest.mark.parametrize('shape', R.APPLY_SHAPES, ids=R.case_id)
def test_forward_apply_eval_and_mask_bits(gpu, shape, res, relu):
    """apply_grid gives bn_apply_kernel rows / (4 TY) blocks per column group (below its cap of 2048), each striding by
    gridDim.y * TY rows: four trips of the grid-stride loop at (32768, 64) in either type (256 x 32 rows per trip in bf16,
    512 x 16 in fp32), five at (315, 64) in bf16 (2 x 32 rows per trip)."""
    rows, C, dt = shape
    ops = _ops()
    c = _case(gpu, rows, C)
    d = _dev(c, dt)
    rd = d['res'] if res else None
    rm0, rv0 = _running_start(C, gpu)
    nbt = _vec(torch.zeros((), dtype=torch.int64, device=gpu), 'nbt')
    rm, rv = lambda: _vec(rm0.float(), 'running_mean'), lambda: _vec(rv0.float(), 'running_var')
    with G.window(ops, 'bn_relu_mask'):
        mask = ops.bn_relu_mask(d['x'])          # 0xFF bytes between flanks: the forward must write every one of them
    (y, mean_k, invstd_k), _ = _labels(ops, lambda: ops.bn_train_fwd(d['x'], rd, d['gamma'], d['beta'], rm(), rv(), nbt, R.EPS, R.MOMENTUM, relu, relu_mask=mask))
    (y2, mean2, invstd2), _ = _labels(ops, lambda: ops.bn_train_fwd(d['x'], rd, d['gamma'], d['beta'], rm(), rv(), nbt, R.EPS, R.MOMENTUM, relu))
    _whole('y / mean / invstd', y, mean_k, invstd_k, y2, mean2, invstd2)
    if dt == 'f32':
        _whole('mask', mask)         # (an fp32 mask byte holds four bits: 0xFF is not one; a bf16 byte of eight set bits is)
    assert torch.equal(y, y2) and torch.equal(mean_k, mean2) and torch.equal(invstd_k, invstd2)        # [equal]
    # the statistics the kernel saved (held to float64 by test_forward_statistics) define the reference of the apply pass
    # [bound] sc = g * invstd and sh = b - mean * sc are rounded, then x * sc + sh (+ res): at most five roundings touch each
    # of the terms below; the factor 8 covers them
    sc = c['gamma'] * invstd_k.double()
    pre = (c['x'] - mean_k.double()) * sc + c['beta'] + (c['res'] if res else 0)
    B = 8 * R.U32 * ((c['x'] * sc).abs() + (mean_k.double() * sc).abs() + c['beta'].abs() + (c['res'].abs() if res else 0))
    lo, hi = (torch.clamp(pre - B, min=0.0), torch.clamp(pre + B, min=0.0)) if relu else (pre - B, pre + B)
    got = R.rows_of(y).double()
    if dt == 'f32':
        assert bool((lo <= got).all()) and bool((got <= hi).all())                           # [bound]
    else:
        assert bool((R.rne(lo, dt) <= got).all()) and bool((got <= R.rne(hi, dt)).all())      # [bound]
    bits = R.unpack_mask(mask, rows, C, R.PER[dt])
    sure = pre.abs() > B
    assert float(sure.double().mean()) > 0.8
    assert torch.equal(bits[sure], (pre > 0)[sure])               # [bound] the bit is y > 0 wherever the bound leaves no doubt
    # eval forward: running_mean integers, running_var powers of four
    rmean, rvar = c['mean'], 1.0 / (c['invstd'] * c['invstd'])
    rmean_d, rvar_d = _vec(rmean.float(), 'running_mean'), _vec(rvar.float(), 'running_var')
    ye, _ = _labels(ops, lambda: ops.bn_eval_fwd(d['x'], rd, d['gamma'], d['beta'], rmean_d, rvar_d, R.EPS, relu))
    _whole('eval y', ye)
    sce = c['gamma'] / torch.sqrt(rvar + R.EPS)
    pree = (c['x'] - rmean) * sce + c['beta'] + (c['res'] if res else 0)
    Be = 8 * R.U32 * ((c['x'] * sce).abs() + (rmean * sce).abs() + c['beta'].abs() + (c['res'].abs() if res else 0))
    lo, hi = (torch.clamp(pree - Be, min=0.0), torch.clamp(pree + Be, min=0.0)) if relu else (pree - Be, pree + Be)
    got = R.rows_of(ye).double()
    if dt == 'f32':
        assert bool((lo <= got).all()) and bool((got <= hi).all())                           # [bound]
    else:
        assert bool((R.rne(lo, dt) <= got).all()) and bool((got <= R.rne(hi, dt)).all())      # [bound]


# ---------------------------------------------------------------- f. mi355_bn_train_fwd_partials at its finalize edges
@pytest.mark.parametrize('case', R.FWD_PARTIAL_CASES, ids=R.case_id)
def test_forward_from_crafted_partials(gpu, case):
    """512 slices switch to bn_finalize_wide_kernel; 1024 and 2048 are the loop strides of the two finalize kernels."""
    ns, C, dt = case
    ops = _ops()
    p = R.sliced_stats_partials(ns, C, device=gpu)
    n, mean, m2 = R.combine_fwd_partials(p)
    x = _put(R.stats_case(16, C, device=gpu)['x'], dt)              # tiny: only the statistics are under test
    gamma, beta = _vec(torch.ones(C, device=gpu), 'gamma'), _vec(torch.zeros(C, device=gpu), 'beta')
    rm0, rv0 = _running_start(C, gpu)
    pd = _vec(p.float(), 'partials')
    for updates in (1, 3):
        rm, rv, nbt = _vec(rm0.float(), 'running_mean'), _vec(rv0.float(), 'running_var'), _vec(torch.full((), 7, dtype=torch.int64, device=gpu), 'nbt')
        (y, mean_k, invstd_k), _ = _labels(ops, lambda: ops.bn_train_fwd(x, None, gamma, beta, rm, rv, nbt, R.EPS, R.MOMENTUM, False, stat_updates=updates,
                                                                         partial=(pd, ns)))
        _whole('y / mean / invstd', y, mean_k, invstd_k)
        rmr, rvr = R.running(mean, m2, float(n[0]), rm0, rv0, R.MOMENTUM, updates)
        assert torch.allclose(mean_k.double(), mean, **MEAN_TOL), float((mean_k.double() - mean).abs().max())        # [stats]
        assert torch.allclose(invstd_k.double(), 1.0 / torch.sqrt(m2 / n + R.EPS), **VAR_TOL)                          # [stats]
        assert torch.allclose(rm.double(), rmr, **MEAN_TOL) and torch.allclose(rv.double(), rvr, **VAR_TOL)          # [stats]
        assert int(nbt) == 7 + updates


# ---------------------------------------------------------------- g. mi355_colsum and mi355_apply_relu_mask
@pytest.mark.parametrize('shape', R.COLSUM_SHAPES, ids=R.case_id)
def test_colsum_bit_for_bit(gpu, shape):
    rows, C, dt = shape
    ops = _ops()
    c = _case(gpu, rows, C)
    d = _dev(c, dt)
    out = _vec(torch.full((C,), 777.0, device=gpu), 'out')
    _labels(ops, lambda: ops.colsum(d['dy'], out, False))
    assert torch.equal(out.double(), R.colsum(c['dy']))                 # [equal]
    prior = R.int_prior(C, 'colsum', gpu)
    out = _vec(prior.float(), 'out')
    _labels(ops, lambda: ops.colsum(d['dy'], out, True))
    assert torch.equal(out.double(), R.colsum(c['dy'], prior))          # [equal]


@pytest.mark.parametrize('shape', R.MASK_APPLY_SHAPES, ids=R.case_id)
def test_apply_relu_mask_bit_for_bit(gpu, shape):
    """(16400, 512) in bf16 holds 1 049 600 chunks: more than the 4096 blocks x 256 threads of the launch, so the grid-stride
    loop runs past its first trip."""
    rows, C, dt = shape
    ops = _ops()
    c = _case(gpu, rows, C)
    per = R.PER[dt]
    b = R.mask_bytes(rows * C // per, 'apply').to(gpu)
    g, bd = _put(c['dy'], dt), _vec(b, 'mask')
    out, _ = _labels(ops, lambda: ops.apply_relu_mask(g, bd))
    assert torch.equal(R.rows_of(out).double(), R.apply_relu_mask(c['dy'], b, per))          # [equal]


# ---------------------------------------------------------------- h. fp8 side outputs (bf16 only)
def _q8(d, gpu):
    N, C, H, W = d['x'].shape
    q = G.empty((N, H, W, C), torch.uint8, gpu, 'fp8 copy').permute(0, 3, 1, 2)         # nothing but the guard fill (an e4m3 / e5m2 NaN)
    st = _vec(torch.tensor([1.0, 1.0, 0.0, 0.0], device=gpu), 'fp8 state')           # {scale, descale, amax bits, pad}: scale 1, y * scale is exact
    return q, st


def _amax_of(st):
    return float(st[2:3].view(torch.int32).view(torch.float32))


@pytest.mark.parametrize('rows,C', R.FP8_SHAPES)
def test_fp8_side_output_of_the_forward(gpu, rows, C):
    """The e4m3 copy is the cast of the values AS STORED.  y itself cannot be made exact in e4m3 (invstd = 1 / sqrt(var + eps)
    is never a power of two), so both sides round the same bf16 values; |y| stays far below 448, nothing saturates."""
    ops = _ops()
    c = _case(gpu, rows, C, mirror=True)
    d = _dev(c, 'bf16', residual=False)
    rm0, rv0 = _running_start(C, gpu)
    nbt = _vec(torch.zeros((), dtype=torch.int64, device=gpu), 'nbt')
    for relu in (False, True):
        q, st = _q8(d, gpu)
        rm, rv = lambda: _vec(rm0.float(), 'running_mean'), lambda: _vec(rv0.float(), 'running_var')
        (y, _, _), _ = _labels(ops, lambda: ops.bn_train_fwd(d['x'], None, d['gamma'], d['beta'], rm(), rv(), nbt, R.EPS, R.MOMENTUM, relu, q8=(q, st)))
        (y0, _, _), _ = _labels(ops, lambda: ops.bn_train_fwd(d['x'], None, d['gamma'], d['beta'], rm(), rv(), nbt, R.EPS, R.MOMENTUM, relu))
        _whole('y / fp8 copy', y, y0, q)
        assert torch.equal(y, y0)                                      # [equal]
        assert float(y.float().abs().max()) < 448
        assert torch.equal(q.view(torch.uint8), y.float().to(torch.float8_e4m3fn).view(torch.uint8))      # [equal]
        assert _amax_of(st) == float(y.float().abs().max())           # [equal]


@pytest.mark.parametrize('relu,dres', [(0, False), (1, True), (2, False), (3, True)])
@pytest.mark.parametrize('rows,C', R.FP8_SHAPES)
def test_fp8_side_output_of_the_backward(gpu, rows, C, relu, dres):
    """Mirrored rows (the second half repeats the first with dy negated): both sums vanish, dx = k0 * g is 1, 2 or 3 times a
    power of two, exact in e5m2.  The side output is written by the three-launch form only: asked for with the one-launch form
    switched ON, the launch log must still show reduce + finalize + apply."""
    ops = _ops()
    c = _case(gpu, rows, C, mirror=True)
    d = _dev(c, 'bf16', residual=False)
    r = _ref(c, relu, residual=False)
    q, st = _q8(d, gpu)
    dx, dr, dg, db, labels = _backward(ops, c, 'bf16', 'resident', relu, dres, False, q8=(q, st), residual=False)
    _assert_form(labels, 'three')
    _whole('fp8 copy', q)
    _assert_sums(c, r, dr, dg, db, dres, False, 'bf16')
    assert float(r['s1'].abs().max()) == 0 and float(r['s2'].abs().max()) == 0
    assert torch.equal(R.rows_of(dx).double(), r['dx'])               # [equal] (exact in bf16 without rounding)
    assert torch.equal(q.view(torch.uint8), dx.float().to(torch.float8_e5m2).view(torch.uint8))          # [equal]
    assert _amax_of(st) == float(dx.float().abs().max()) and _amax_of(st) > 0          # [equal]
    assert ops.bn_resident_timeouts() == 0


# ---------------------------------------------------------------- i. NaN, +Inf and -Inf operands (tests/nonfinite_ref.py)
# One operand at a time holds a special; every other value is the exact operand of the cases above.  A channel's reductions are
# its own: the channel that holds the special follows the reduced rule (non-finite where the float64 reference is), and every
# OTHER channel has the bits of the run without the special -- which the sections above hold to float64.
NF_SHAPES = [(3, 64, 'bf16'), (3, 64, 'f32'), (315, 64, 'bf16'), (315, 64, 'f32'), (315, 192, 'bf16')]          # the smallest ragged shapes
NF_BWD_SHAPES = [(315, 64, 'bf16'), (315, 64, 'f32'), (256, 64, 'bf16'), (256, 64, 'f32')]      # ragged and one row per block; both forms run
NF_BWD_CASES = [(rows, C, dt, form, relu, dres) for rows, C, dt in NF_BWD_SHAPES for form in ('three', 'resident')
                for relu in (0, 1, 2, 3) for dres in (False, True) if not (form == 'resident' and relu == 1) and (dres is False or relu in (1, 3))]


def _same_bits(a, b):
    """Two results of one kernel on operands that differ elsewhere: every bit, NaN payloads included."""
    if a is None or b is None:
        return a is None and b is None
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _other_channels_unchanged(what, got, clean, bad):
    """Per-channel vectors [C] or feature maps [N][C][H][W]: outside the channels of `bad`, the bits of the clean run."""
    keep = [ch for ch in range(got.shape[0] if got.dim() == 1 else got.shape[1]) if ch not in bad]
    a, b = (got[keep], clean[keep]) if got.dim() == 1 else (got[:, keep], clean[:, keep])
    assert _same_bits(a, b), '%s: a special in channel(s) %s changed another channel' % (what, sorted(bad))


def _seeded(mat, positions):
    return NF.seed_specials(mat, positions)


@pytest.mark.parametrize('updates,res,relu', [(1, False, False), (2, True, True), (1, True, False)])
@pytest.mark.parametrize('shape', NF_SHAPES, ids=R.case_id)
def test_training_forward_with_an_inf_and_a_nan_channel(gpu, shape, updates, res, relu):
    rows, C, dt = shape
    ops = _ops()
    G.row_pitch(C * 4)
    s = R.stats_case(rows, C, device=gpu)
    c_inf, c_nan = C - 1, 0
    x2 = _seeded(s['x'], [((rows - 1, c_inf), '+inf'), ((rows // 2, c_nan), 'nan')])
    resid = R.int_prior(C, 'nf res', gpu).view(1, C).expand(rows, C).contiguous() if res else None
    rm0, rv0 = _running_start(C, gpu)
    ref = R.train_fwd(x2, s['gamma'], s['beta'], res=resid, relu=relu, rm0=rm0, rv0=rv0, repeats=updates)
    yref = NF.relu_keep_nan(ref['ypre']) if relu else ref['ypre']
    assert bool((yref[:, [c_inf, c_nan]] != yref[:, [c_inf, c_nan]]).all()) and 4 * int(torch.isfinite(yref).sum()) >= yref.numel()
    for k in ('mean', 'invstd', 'rm', 'rv'):
        assert not bool(torch.isfinite(ref[k][[c_inf, c_nan]]).any()) and int(torch.isfinite(ref[k]).sum()) == C - 2, k
    gamma, beta = _vec(s['gamma'].float(), 'gamma'), _vec(s['beta'].float(), 'beta')
    rd = _put(resid, dt) if res else None
    runs = []
    for x in (s['x'], x2):
        rm, rv, nbt = _vec(rm0.float(), 'running_mean'), _vec(rv0.float(), 'running_var'), _vec(torch.full((), 5, dtype=torch.int64, device=gpu), 'nbt')
        xd = _put(x, dt)
        (y, mean, invstd), _ = _labels(ops, lambda: ops.bn_train_fwd(xd, rd, gamma, beta, rm, rv, nbt, R.EPS, R.MOMENTUM, relu, stat_updates=updates))
        _whole('y / mean / invstd', y, mean, invstd)
        assert int(nbt) == 5 + updates
        runs.append((y, mean, invstd, rm, rv))
    (yc, meanc, invc, rmc, rvc), (y, mean, invstd, rm, rv) = runs
    bad = {c_inf, c_nan}
    got = R.rows_of(y)
    assert bool((got[:, [c_inf, c_nan]] != got[:, [c_inf, c_nan]]).all()), 'the two channels come out entirely NaN'
    _other_channels_unchanged('y', y, yc, bad)
    for what, a, b, tol in (('mean', mean, meanc, MEAN_TOL), ('invstd', invstd, invc, VAR_TOL), ('running_mean', rm, rmc, MEAN_TOL), ('running_var', rv, rvc, VAR_TOL)):
        _other_channels_unchanged(what, a, b, bad)
        r = ref[{'mean': 'mean', 'invstd': 'invstd', 'running_mean': 'rm', 'running_var': 'rv'}[what]]
        bad_msg = NF.reduced_mismatch(a, r, **tol)           # [stats] on the finite channels, non-finite in the two others
        assert bad_msg is None, '%s: %s' % (what, bad_msg)


@pytest.mark.parametrize('res,relu', R.APPLY_MODES)
@pytest.mark.parametrize('shape', NF_SHAPES[2:], ids=R.case_id)
def test_eval_forward_and_apply_with_specials(gpu, shape, res, relu):
    """Pointwise: the class of every element is the reference's (the ReLU keeps NaN, -Inf becomes 0, a negative gamma turns the
    infinities round), the finite elements stay within the [bound] of test_forward_apply_eval_and_mask_bits."""
    rows, C, dt = shape
    ops = _ops()
    c = _case(gpu, rows, C)
    pos = [((rows - 1, C - 1), 'nan'), ((0, 0), '+inf'), ((rows // 2, C // 2), '-inf')]
    neg = (c['gamma'] < 0).nonzero().view(-1).tolist()          # x: both infinities under a negative gamma, so that each comes out as the other
    xpos = [((rows - 1, C - 1), 'nan'), ((0, neg[0]), '+inf'), ((rows // 2, neg[-1]), '-inf')]
    assert len(neg) >= 2
    rmean, rvar = c['mean'], 1.0 / (c['invstd'] * c['invstd'])
    rmean_d, rvar_d = _vec(rmean.float(), 'running_mean'), _vec(rvar.float(), 'running_var')
    gamma, beta = _vec(c['gamma'].float(), 'gamma'), _vec(c['beta'].float(), 'beta')
    sce = c['gamma'] / torch.sqrt(rvar + R.EPS)
    for operand in (('x', 'res') if res else ('x',)):
        x = _seeded(c['x'], xpos) if operand == 'x' else c['x']
        rs = _seeded(c['res'], pos) if operand == 'res' else c['res']
        xd, rd = _put(x, dt), (_put(rs, dt) if res else None)
        pree = (x - rmean) * sce + c['beta'] + (rs if res else 0)
        want = NF.relu_keep_nan(pree) if relu else pree
        NF.case_condition(want, ('nan', '+inf') if relu else NF.KINDS, 'eval %s' % operand)
        ye, _ = _labels(ops, lambda: ops.bn_eval_fwd(xd, rd, gamma, beta, rmean_d, rvar_d, R.EPS, relu))
        _whole('eval y', ye)
        got = R.rows_of(ye).double()
        assert torch.equal(NF.classes(got), NF.classes(R.rne(want, dt))), 'eval forward, special in %s: %d classes differ' % (operand, int((NF.classes(got) != NF.classes(want)).sum()))
        fin = torch.isfinite(pree)
        assert not relu or not bool(got[pree == -NF.INF].ne(0).any())          # (-Inf through the ReLU: an exact zero)
        Be = 8 * R.U32 * ((x * sce).abs() + (rmean * sce).abs() + c['beta'].abs() + (rs.abs() if res else 0))
        lo, hi = (torch.clamp(pree - Be, min=0.0), torch.clamp(pree + Be, min=0.0)) if relu else (pree - Be, pree + Be)
        lo, hi = (lo, hi) if dt == 'f32' else (R.rne(lo, dt), R.rne(hi, dt))
        assert bool((lo[fin] <= got[fin]).all()) and bool((got[fin] <= hi[fin]).all())          # [bound]
    if res:
        # the apply pass of the training forward: the statistics are x's and clean, the special rides in on the residual and
        # stays in its element; every other element keeps the bits of the clean run
        rm0, rv0 = _running_start(C, gpu)
        nbt = _vec(torch.zeros((), dtype=torch.int64, device=gpu), 'nbt')
        xd = _put(c['x'], dt)
        outs = []
        for rs in (c['res'], _seeded(c['res'], pos)):
            rd = _put(rs, dt)
            (y, mean, invstd), _ = _labels(ops, lambda: ops.bn_train_fwd(xd, rd, gamma, beta, _vec(rm0.float(), 'running_mean'), _vec(rv0.float(), 'running_var'),
                                                                     nbt, R.EPS, R.MOMENTUM, relu))
            _whole('y', y)
            outs.append((R.rows_of(y), mean, invstd))
        (yc, mc, ic), (y, m, i) = outs
        assert _same_bits(m, mc) and _same_bits(i, ic)
        want = torch.zeros(rows, C, dtype=torch.int8, device=gpu)
        for (r, ch), kd in pos:
            want[r, ch] = NF.CLASS_OF[kd] if not (relu and kd == '-inf') else NF.FINITE
        assert torch.equal(NF.classes(y), want)
        assert float(y[rows // 2, C // 2]) == 0.0 or not relu
        seeded = torch.zeros(rows, C, dtype=torch.bool, device=gpu)
        for (r, ch), _ in pos:
            seeded[r, ch] = True
        assert _same_bits(y[~seeded], yc[~seeded])


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_bn_relu_maxpool_with_specials(gpu, dt):
    """A NaN wins its windows (the last NaN of a window is the kept position), -Inf loses to everything, +Inf wins unless a NaN is
    there: the one-pass kernel against small_exact_ref.maxpool_fwd of the BatchNorm + ReLU output of the separate pass, on clean
    statistics partials (crafted from the clean x, so that only the apply + pool part sees the specials)."""
    import small_exact_ref as S
    ops = _ops()
    N, H, W, C = 3, 18, 14, 64
    rows = N * H * W
    G.row_pitch(C * 4)
    s = R.stats_case(256, C, device=gpu)          # per-channel mean / gamma / beta recipe; the values below are this module's own
    rng = torch.Generator().manual_seed(7)
    x = (torch.randint(-3, 4, (rows, C), generator=rng).double().to(gpu) + s['mean_c'])
    bounds = [(r0, min(rows, r0 + 64)) for r0 in range(0, rows, 64)]
    part = _vec(R.fwd_partials(x, bounds).float().reshape(-1), 'partials')
    pos = []
    for i, (n, h, w) in enumerate([(0, 0, 0), (0, 1, 1), (1, 8, 7), (1, 8, 8), (1, 9, 7), (2, 17, 13), (2, 5, 5), (2, 6, 6)]):
        # (1, 8, 7), (1, 8, 8) and (1, 9, 7) share a channel: windows with two NaN, and with a NaN and a +Inf
        pos.append((((n * H + h) * W + w, (63, 54, 45, 45, 45, 18, 9, 0)[i]), ('nan', 'nan', 'nan', '+inf', 'nan', '-inf', '+inf', '-inf')[i]))
    x2 = _seeded(x, pos)
    xd = G.place(x2.view(N, H, W, C).permute(0, 3, 1, 2).to(R.TDT[dt]).contiguous(memory_format=torch.channels_last), 'feature map')
    gamma, beta = _vec(s['gamma'].float(), 'gamma'), _vec(s['beta'].float(), 'beta')
    res = []
    for fused in (False, True):
        rm, rv, nbt = _vec(torch.zeros(C, device=gpu), 'running_mean'), _vec(torch.ones(C, device=gpu), 'running_var'), _vec(torch.zeros((), dtype=torch.int64, device=gpu), 'nbt')
        if fused:
            (p, arg, mean, invstd), _ = _labels(ops, lambda: ops.bn_relu_maxpool_fwd(xd, gamma, beta, rm, rv, nbt, R.EPS, R.MOMENTUM, 1, (part, len(bounds))))
        else:
            (z, mean, invstd), _ = _labels(ops, lambda: ops.bn_train_fwd(xd, None, gamma, beta, rm, rv, nbt, R.EPS, R.MOMENTUM, True, partial=(part, len(bounds))))
            _whole('z', z)
        res.append((mean, invstd, rm, rv))
    _whole('pooled / codes', p, arg)
    for a, b in zip(*res):
        assert _same_bits(a, b) and bool(torch.isfinite(a).all())
    zc = NF.classes(z)
    assert int((zc == NF.IS_NAN).sum()) == 4 and int((zc == NF.POS_INF).sum()) + int((zc == NF.NEG_INF).sum()) >= 1
    y_ref, code_ref = S.maxpool_fwd(z.double().cpu())
    assert 4 * int(torch.isfinite(y_ref).sum()) >= y_ref.numel() and bool((y_ref != y_ref).any())
    assert S.bits_equal(p.double().cpu().contiguous(), y_ref), 'pooled values'
    assert torch.equal(arg.cpu(), code_ref.permute(0, 2, 3, 1)), 'window codes'


@pytest.mark.parametrize('case', NF_BWD_CASES, ids=R.case_id)
def test_backward_with_specials(gpu, case):
    """(a) a NaN in dy where the gradient is live: the channel's dgamma / dbeta are non-finite and its dx is NaN throughout;
    (b) a NaN in dy where the ReLU mask clears it: nothing changes, bit for bit (a select, as ATen's threshold_backward);
    (c) a +Inf in x: the channel's dgamma and dx are non-finite.  Every other channel has the bits of the clean run."""
    rows, C, dt, form, relu, dres = case
    ops = _ops()
    c = _case(gpu, rows, C)
    d = _dev(c, dt)
    keep = None if relu == 0 else (c['ypre'] > 0 if relu == 2 else R.fwd_y(c, True, True) > 0)
    clean = _backward(ops, c, dt, form, relu, dres, False)
    _assert_form(clean[4], form)

    def run(**over):
        saved = {k: d[k] for k in over}
        d.update({k: _put(v, dt) for k, v in over.items()})
        try:
            out = _backward(ops, c, dt, form, relu, dres, False)
        finally:
            d.update(saved)
        _assert_form(out[4], form)
        return out

    live = NF.bn_positions(rows, C, keep, True)[0]
    ch = live[1]
    dx, dr, dg, db, _ = run(dy=_seeded(c['dy'], [(live, 'nan')]))
    ref = NF.bn_bwd_select(dict(c, dy=_seeded(c['dy'], [(live, 'nan')])), keep)
    assert not bool(torch.isfinite(ref['dgamma'][ch])) and not bool(torch.isfinite(ref['dx'][:, ch]).any()) and int(torch.isfinite(ref['dbeta']).sum()) == C - 1
    assert NF.reduced_mismatch(dg, ref['dgamma']) is None and NF.reduced_mismatch(db, ref['dbeta']) is None, '(a) dgamma / dbeta'
    got = R.rows_of(dx)
    assert bool((got[:, ch] != got[:, ch]).all()), '(a) the channel of a live NaN: dx is NaN throughout'
    for what, a, b in (('dx', dx, clean[0]), ('dgamma', dg, clean[2]), ('dbeta', db, clean[3])):
        _other_channels_unchanged('(a) ' + what, a, b, {ch})
    if dres:
        want = NF.classes(ref['dres'])
        assert torch.equal(NF.classes(R.rows_of(dr)), want) and int((want != 0).sum()) == 1
        assert _same_bits(R.rows_of(dr)[want == 0], R.rows_of(clean[1])[want == 0])
    if keep is not None:
        masked = NF.bn_positions(rows, C, keep, False)
        out = run(dy=_seeded(c['dy'], [(p, 'nan') for p in masked]))
        for what, a, b in zip(('dx', 'dres', 'dgamma', 'dbeta'), out[:4], clean[:4]):
            assert _same_bits(a, b), '(b) a masked NaN changed %s' % what
    if relu == 1:
        # the mask is !(y <= 0), ATen's threshold_backward: a NaN in the stored forward output lets the gradient through (it used to
        # count as masked: y > 0 is false for NaN, and dbeta stayed finite where torch's is NaN).  At a masked element, a NaN in y
        # gives the bits of a run with a positive y there.
        y = R.fwd_y(c, True, True)
        at = NF.bn_positions(rows, C, keep, False)[0]
        one = y.clone()
        one[at] = 1.0
        a, b = run(y=_seeded(y, [(at, 'nan')])), run(y=one)
        for what, p, q in zip(('dx', 'dres', 'dgamma', 'dbeta'), a[:4], b[:4]):
            assert _same_bits(p, q), 'a NaN in y does not let the gradient through: %s' % what
        assert not _same_bits(a[3], clean[3]) or float(c['dy'][at]) == 0.0
    xpos = (rows // 2, C - 1)
    x2 = _seeded(c['x'], [(xpos, '+inf')])
    dx, dr, dg, db, _ = run(x=x2)
    keep2 = keep if relu != 2 else ((x2 - c['mean']) * c['invstd'] * c['gamma'] + c['beta']) > 0
    ref = NF.bn_bwd_select(dict(c, x=x2), keep2)
    assert not bool(torch.isfinite(ref['dgamma'][C - 1])) and not bool(torch.isfinite(ref['dx'][:, C - 1]).any())
    assert NF.reduced_mismatch(dg, ref['dgamma']) is None and NF.reduced_mismatch(db, ref['dbeta']) is None, '(c) dgamma / dbeta'
    got = R.rows_of(dx)
    assert not bool(torch.isfinite(got[:, C - 1]).any()), '(c) the channel of an Inf in x: dx is non-finite throughout'
    for what, a, b in (('dx', dx, clean[0]), ('dgamma', dg, clean[2]), ('dbeta', db, clean[3])):
        _other_channels_unchanged('(c) ' + what, a, b, {C - 1})
    assert ops.bn_resident_timeouts() == 0


@pytest.mark.parametrize('shape', NF_SHAPES, ids=R.case_id)
def test_colsum_and_mask_apply_with_specials(gpu, shape):
    rows, C, dt = shape
    ops = _ops()
    c = _case(gpu, rows, C)
    pos = [((rows - 1, C - 1), 'nan'), ((0, 0), '+inf'), ((rows // 2, C // 2), '-inf')]
    dy2 = _seeded(c['dy'], pos)
    dyd = _put(dy2, dt)
    for acc in (False, True):
        prior = R.int_prior(C, 'colsum', gpu)
        out = _vec(prior.float() if acc else torch.full((C,), 777.0, device=gpu), 'out')
        _labels(ops, lambda: ops.colsum(dyd, out, acc))
        ref = R.colsum(dy2, prior if acc else None)
        assert int((~torch.isfinite(ref)).sum()) == 3
        bad = NF.reduced_mismatch(out, ref)                                   # finite sums [equal], the three channels non-finite
        assert bad is None, bad
    # apply_relu_mask: a select -- a special under a cleared bit becomes an exact zero, one under a set bit stays
    per = R.PER[dt]
    b = R.mask_bytes(rows * C // per, 'apply').to(gpu)
    bits = R.unpack_mask(b, rows, C, per)
    pos, used = [], set()
    for kd, want in (('nan', False), ('nan', True), ('+inf', True), ('-inf', False)):          # each in a channel of its own, from the last one down
        r, ch = next((int(r), int(ch)) for r, ch in (bits == want).nonzero().flip(0).tolist() if ch not in used)
        used.add(ch)
        pos.append(((r, ch), kd))
    g2 = _seeded(c['dy'], pos)
    out, _ = _labels(ops, lambda: ops.apply_relu_mask(_put(g2, dt), _vec(b, 'mask')))
    ref = NF.relu_bwd_select(g2, bits)
    assert NF.class_counts(ref)[NF.IS_NAN] == 1 and NF.class_counts(ref)[NF.POS_INF] == 1 and NF.class_counts(ref)[NF.NEG_INF] == 0
    bad = NF.pointwise_mismatch(R.rows_of(out), ref, R.TDT[dt])
    assert bad is None, bad
