"""The float64 BatchNorm reference of bn_exact_ref.py held against torch's own batch_norm and autograd, and the range condition
of every case of test_gpu_bn_exact.py asserted without a GPU: a case that leaves the exact range fails here, not there."""
import pytest
import torch
import torch.nn.functional as F

import bn_exact_ref as R


def _torch_fwd_bwd(x, gamma, beta, res, relu, dy, rm0, rv0, eps=R.EPS):
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    rr = res.clone().requires_grad_(True) if res is not None else None
    rm, rv = rm0.clone(), rv0.clone()
    y = F.batch_norm(R.nchw(xr), rm, rv, gr, br, True, R.MOMENTUM, eps)
    if rr is not None:
        y = y + R.nchw(rr)
    if relu:
        y = F.relu(y)
    y.backward(R.nchw(dy))
    return R.rows_of(y.detach()), xr.grad, None if rr is None else rr.grad, gr.grad, br.grad, rm, rv


@pytest.mark.parametrize('rows,C', [(315, 8), (256, 24), (16, 64)])
@pytest.mark.parametrize('res,relu', [(False, False), (False, True), (True, True)])
def test_reference_matches_torch_in_float64(rows, C, res, relu):
    """Train forward, its running statistics, backward and eval forward against torch in float64.  The inputs and beta are
    shifted by 0.25 (batch statistics remove a shift of x alone), so no pre-activation is exactly 0 where rounding noise in either
    implementation would decide the ReLU."""
    c = R.make_case(rows, C)
    c = dict(c, beta=c['beta'] + 0.25)
    x = c['x'] + 0.25
    r = c['res'] if res else None
    rm0, rv0 = R.int_prior(C, 'rm'), R.int_prior(C, 'rv').abs() + 1
    f = R.train_fwd(x, c['gamma'], c['beta'], r, relu, rm0=rm0, rv0=rv0, repeats=1)
    assert float(f['ypre'].abs().min()) > 1e-9
    y, dx, dres, dg, db, rm, rv = _torch_fwd_bwd(x, c['gamma'], c['beta'], r, relu, c['dy'], rm0, rv0)
    assert torch.allclose(f['y'], y, rtol=1e-12, atol=1e-12)
    assert torch.allclose(f['rm'], rm, rtol=1e-12, atol=1e-12) and torch.allclose(f['rv'], rv, rtol=1e-12, atol=1e-12)
    # the backward reference takes the statistics as inputs
    b = R.bn_bwd(dict(c, x=x, mean=f['mean'], invstd=f['invstd']), f['mask'] if relu else None)
    assert torch.allclose(b['dx'], dx, rtol=1e-10, atol=1e-10)
    assert torch.allclose(b['dgamma'], dg, rtol=1e-10, atol=1e-10) and torch.allclose(b['dbeta'], db, rtol=1e-10, atol=1e-10)
    if res:
        assert torch.allclose(b['dres'], dres, rtol=0, atol=0)
    # three momentum updates = three forward passes over the same batch
    rm3, rv3 = rm0.clone(), rv0.clone()
    for _ in range(3):
        F.batch_norm(R.nchw(x), rm3, rv3, c['gamma'], c['beta'], True, R.MOMENTUM, R.EPS)
    f3 = R.train_fwd(x, c['gamma'], c['beta'], rm0=rm0, rv0=rv0, repeats=3)
    assert torch.allclose(f3['rm'], rm3, rtol=1e-12, atol=1e-12) and torch.allclose(f3['rv'], rv3, rtol=1e-12, atol=1e-12)
    f0 = R.train_fwd(x, c['gamma'], c['beta'], rm0=rm0, rv0=rv0, repeats=0)
    assert torch.equal(f0['rm'], rm0) and torch.equal(f0['rv'], rv0)
    # eval forward
    ye = F.batch_norm(R.nchw(x), rm0, rv0, c['gamma'], c['beta'], False, R.MOMENTUM, R.EPS)
    if res:
        ye = ye + R.nchw(r)
    if relu:
        ye = F.relu(ye)
    assert torch.allclose(R.eval_fwd(x, c['gamma'], c['beta'], rm0, rv0, r, relu), R.rows_of(ye), rtol=1e-12, atol=1e-12)


def test_generator_is_exact_and_a_tenth_of_the_pre_activations_are_zero():
    c = R.make_case(1024, 64)
    assert torch.equal(c['ypre'], (c['x'] - c['mean']) * (c['gamma'] * c['invstd']) + c['beta'])
    assert float(c['x'].abs().max()) <= 12 and bool((c['gamma'] < 0).any()) and bool((c['gamma'] > 0).any())
    assert 0.06 <= float((c['ypre'] == 0).double().mean()) <= 0.2
    assert float(((c['ypre'] + c['res']) == 0).double().mean()) >= 0.03


def test_zero_ties_follow_the_kernels_strict_greater_than():
    """The kernels document the mask as y > 0: a pre-activation of exactly 0 passes no gradient, from every mask source."""
    c = R.make_case(256, 64)
    for source, pre in ((1, c['ypre'] + c['res']), (2, c['ypre']), (3, c['ypre'] + c['res'])):
        m = R.relu_mask(c, source)
        assert bool((pre == 0).any())
        assert not bool(m[pre == 0].any()) and bool(m[pre > 0].all()) and not bool(m[pre < 0].any())
        assert torch.equal(R.bn_bwd(c, m)['dres'][pre == 0], torch.zeros(int((pre == 0).sum()), dtype=torch.float64))
    assert R.relu_mask(c, 0) is None
    assert not torch.equal(R.relu_mask(c, 1), R.relu_mask(c, 2))        # the residual moves the mask: sources 1 / 3 are not source 2


@pytest.mark.parametrize('per', [4, 8])
def test_mask_bytes_cover_chunks_in_memory_order(per):
    """Byte i covers NHWC chunk i, bit e its element e."""
    rows, C = 5, 3 * per
    m = torch.zeros(rows, C, dtype=torch.bool)
    m[2, per + 3] = True
    b = R.pack_mask(m, per)
    assert int(b[2 * 3 + 1]) == 1 << 3 and int(b.sum()) == 1 << 3
    rnd = R.mask_bytes(rows * 3, 'layout')
    assert torch.equal(R.pack_mask(R.unpack_mask(rnd, rows, C, per), per), rnd if per == 8 else rnd & 15)
    g = torch.arange(1, rows * C + 1, dtype=torch.float64).view(rows, C)
    assert torch.equal(R.apply_relu_mask(g, b, per), g * m)


def _modes_of(cases):
    seen = {}
    for rows, C, dt, form, relu, dres, acc in cases:
        seen.setdefault((rows, C, dt), set()).add((relu, acc))
    return seen


@pytest.mark.parametrize('shape', R.BWD_SHAPES, ids=R.case_id)
def test_range_condition_holds_for_every_backward_case(shape):
    rows, C, dt = shape
    c = R.make_case(rows, C)
    modes = _modes_of(R.bwd_cases([shape], R.BWD_MODES))[shape]
    assert {m[0] for m in modes} == {0, 1, 2, 3}
    for source in (0, 1, 2):            # (source 3 applies the mask of source 1)
        for acc in (False, True):
            R.check_exact(c, R.relu_mask(c, source), dt, R.int_prior(C, 'dg') if acc else None, R.int_prior(C, 'db') if acc else None)
    if rows * C >= 256 * 64:
        assert float((c['ypre'] == 0).double().mean()) > 0.03


@pytest.mark.parametrize('shape', R.RAGGED_SHAPES, ids=R.case_id)
def test_sums_stay_exact_for_every_ragged_case(shape):
    rows, C, dt = shape
    c = R.make_case(rows, C)
    for source in (0, 1, 2):
        r = R.check_exact(c, R.relu_mask(c, source), dt, R.int_prior(C, 'dg'), R.int_prior(C, 'db'), pow2_rows=False)
        # what the bound is made of is finite and the bound is far below the bf16 spacing of the values it brackets
        B = R.dx_bound(r)
        assert bool(torch.isfinite(B).all()) and float(B.max()) <= 8 * R.U32 * 2 * (3 + 3 + 12)


def test_range_check_refuses_a_case_outside_the_range():
    c = R.make_case(256, 8)
    R.check_exact(c, None, 'bf16')
    with pytest.raises(AssertionError):
        R.check_exact(dict(c, x=c['x'] + 1.0 / 1024), None, 'bf16')            # not a bf16 value
    with pytest.raises(AssertionError):
        R.check_exact(dict(c, invstd=c['invstd'] * 3), None, 'f32')             # xhat no integer
    with pytest.raises(AssertionError):
        R.check_exact(dict(c, rows=255, x=c['x'][:255], dy=c['dy'][:255], res=c['res'][:255], xhat=c['xhat'][:255],
                           ypre=c['ypre'][:255]), None, 'f32')                   # rows no power of two


def test_one_lost_row_breaks_the_exact_comparison_and_seldom_the_old_tolerance():
    """What the bit-for-bit comparison is for: a reduction that drops its last row at 1024 rows moves dgamma / dbeta by one
    row's contribution, which in most channels is inside the 2e-3 * (max + 1) * 8 the tolerance test allows in bf16."""
    c = R.make_case(1024, 64)
    full = R.bn_bwd(c)
    short = R.bn_bwd(dict(c, x=c['x'][:-1], dy=c['dy'][:-1], rows=1024))
    for k in ('dgamma', 'dbeta'):
        assert not torch.equal(short[k], full[k])
        within = (short[k] - full[k]).abs() <= 2e-3 * (float(full[k].abs().max()) + 1) * 8
        assert float(within.double().mean()) > 0.75


@pytest.mark.parametrize('case', [c for c in R.BWD_PARTIAL_CASES if c[3] == 'f32' and c[4] == 0], ids=R.case_id)
def test_crafted_backward_partials_add_up(case):
    ns, rows, C, dt, relu, dres, acc = case
    c = R.make_case(rows, C)
    for source in (0, 3):
        r = R.check_exact(c, R.relu_mask(c, source), 'bf16')
        p = R.bwd_partials(r['s1'], r['s2'], ns, source)
        assert tuple(p.shape) == (ns, C, 2) and torch.equal(p, p.round())
        assert torch.equal(p[:, :, 0].sum(0), r['s1']) and torch.equal(p[:, :, 1].sum(0), r['s2'])
        assert torch.equal(p.float().double(), p)
        if ns > 2:
            assert bool((p < 0).any()) and bool((p > 0).any())


def test_forward_partials_of_a_row_partition_recombine():
    s = R.stats_case(1000, 24)
    x = s['x']
    bounds = [(0, 0), (0, 1), (1, 64), (64, 64), (64, 315), (315, 1000), (1000, 1000)]
    p = R.fwd_partials(x, bounds)
    assert float(p[0].abs().max()) == 0 and float(p[3].abs().max()) == 0 and float(p[6].abs().max()) == 0
    n, mean, m2 = R.combine_fwd_partials(p)
    f = R.train_fwd(x, s['gamma'], s['beta'])
    assert torch.equal(n, torch.full((24,), 1000.0, dtype=torch.float64))
    assert torch.allclose(mean, f['mean'], rtol=1e-13, atol=1e-13) and torch.allclose(m2 / 1000, f['var'], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('shape', R.STATS_SHAPES, ids=R.case_id)
def test_one_lost_or_doubled_row_moves_the_mean_past_the_tolerance(shape):
    rows, C, dt = shape
    s = R.stats_case(rows, C)
    x = s['x']
    assert torch.equal(R.rne(x, dt), x) and float((x - s['mean_c']).abs().min()) >= 2
    assert float(s['mean_c'].abs().min()) >= 1
    if rows < 3:
        return
    mean = x.mean(0)
    tol = 1e-6 + 1e-5 * mean.abs()
    # dropping row i: (rows * mean - x_i) / (rows - 1); doubling it: (rows * mean + x_i) / (rows + 1)
    drop = ((rows * mean - x) / (rows - 1) - mean).abs()
    twice = ((rows * mean + x) / (rows + 1) - mean).abs()
    assert bool((drop > 10 * tol).all()) and bool((twice > 10 * tol).all())


@pytest.mark.parametrize('ns', R.FWD_PARTIAL_NSLICES)
def test_one_lost_slice_moves_the_mean_past_the_tolerance(ns):
    p = R.sliced_stats_partials(ns, 64)
    empty = p[:, 0, 0] == 0
    assert bool(((p[:, :, 0] == 0) == empty.view(-1, 1)).all()) and float(p[empty].abs().max() if bool(empty.any()) else 0.0) == 0
    if ns >= 63:
        assert 0.03 <= float(empty.double().mean()) <= 0.2
    n, mean, m2 = R.combine_fwd_partials(p)
    assert float(n[0]) == 64.0 * int((~empty).sum())
    tol = 1e-6 + 1e-5 * mean.abs()
    if int((~empty).sum()) < 2:
        return
    # without slice i: (n * mean - n_i * mean_i) / (n - n_i)
    ni, mi = p[:, :, 0], p[:, :, 1]
    moved = ((n * mean - ni * mi) / (n - ni) - mean).abs()
    assert bool((moved[~empty] > 10 * tol).all())


@pytest.mark.parametrize('C', [4, 8, 64])
def test_sliced_partials_are_the_partials_of_a_tensor(C):
    """The closed form of sliced_stats_partials against fwd_partials of a tensor with the same slice sums."""
    p = R.sliced_stats_partials(65, C)
    n, mean, m2 = R.combine_fwd_partials(p)
    # rebuild a tensor slice by slice from two-point rows: a slice with mean m and M2 v over 64 rows is matched by
    # 32 rows at m - s and 32 at m + s with 64 s^2 = v
    rows = []
    for i in range(65):
        if float(p[i, 0, 0]) == 0:
            continue
        s = torch.sqrt(p[i, :, 2] / 64)
        rows += [p[i, :, 1] - s] * 32 + [p[i, :, 1] + s] * 32
    x = torch.stack(rows)
    assert torch.allclose(x.mean(0), mean, rtol=1e-12, atol=1e-12)
    assert torch.allclose(((x - x.mean(0)) ** 2).sum(0), m2, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize('shape', R.FP8_SHAPES)
def test_fp8_case_keeps_dx_exact_in_e5m2(shape):
    """Mirrored rows: both sums vanish for the masks that depend on x alone, dx = k0 * g is 1, 2 or 3 times a power of two."""
    rows, C = shape
    c = R.make_case(rows, C, mirror=True)
    for mask in (None, c['ypre'] > 0):
        r = R.check_exact(c, mask, 'bf16')
        assert float(r['s1'].abs().max()) == 0 and float(r['s2'].abs().max()) == 0
        assert torch.equal(r['dx'].float().to(torch.float8_e5m2).double(), r['dx'])
    y = R.fwd_y(c, False, True)
    assert torch.equal(y.float().to(torch.float8_e4m3fn).double(), y)


def test_workspace_size_for_every_case_shape_without_a_gpu():
    """mi355_bn_workspace is host code: it must size every shape of the tables, the fp32-only C = 4 included (where the bf16
    plan it also tries has no chunk per row and once divided by zero)."""
    import mi355
    lib = mi355.load()
    shapes = {(s[0], s[1]) for s in R.BWD_SHAPES + R.RAGGED_SHAPES + R.STATS_SHAPES + R.APPLY_SHAPES + R.MASK_APPLY_SHAPES}
    shapes |= {(16, C) for _, C, _ in R.FWD_PARTIAL_CASES} | set(R.FP8_SHAPES)
    for rows, C in sorted(shapes):
        need = lib.mi355_bn_workspace(rows, C)
        assert need >= (32768 + 4 * C) * 4 and need == lib.mi355_colsum_workspace(rows, C), (rows, C)
