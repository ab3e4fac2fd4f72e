"""Joint feature alignment on the GPU: the jfa_pool / jfa_kl / jfa_scatter launches against the reference's own loss1 / loss3
(tests/golden/g15_jfa.npz) and against the restatement of tests/jfa_ref.py in float64, at the shapes where the tiling can go
wrong and at one workload-shaped case; their bit-level properties on exact operands; the gradient requests; the refused
arguments; the GradFanIn protocol of the pooling's backward in both orders; DAStep's `jfa`.

The tolerance, everywhere (jfa_ref.bounds): a kernel result may be as far from the float64 result as 4 times the distance of a
float32 run of the reference expression from it (the fixture's float32 arrays for the fixture cases, jfa_ref in float32
otherwise), with the floors jfa_ref.py writes down.  A gradient that is STORED in bf16 (bf16 features) may in addition, element by
element, be one bf16 rounding from the value before storage: bf16 keeps 8 significant bits, so round-to-nearest moves a value v
by at most half a unit in the last place, 2^-8 of the power of two below |v|, hence at most 2^-8 |v|; v itself is within the
bound of the float64 value r, so the allowance of an element is 2^-8 (|r| + bound).  The format, not the kernel's arithmetic.

Guards (tests/guarded.py).  The kernel-level tests of section 3 and the KL test of section 4 call the wrappers through _guard:
feature maps, key points, descriptors and gradients are G.place() copies, descriptors, rows and KL gradients the wrappers make
come from torch.empty / torch.empty_like inside the window, a feature gradient that is written (not accumulated) is a G.empty()
buffer, and the row pitch is W * C * esize of the feature map.  The tests through uda.model.loss and autograd (sections 1 and 2,
the two-runs test) go through _run, which keeps one window open over the forward, the backward and the two loss1 calls: the
wrappers allocate every descriptor and gradient there too, so all of them are guarded and must be written completely.  The
GradFanIn test and DAStep are not guarded."""
import numpy as np
import pytest
import torch

from conftest import golden
import guarded as G
import jfa_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()


def _guard(label, fn, *args, **kw):
    """One wrapper call inside a guard window; no flank byte of anything placed or allocated has changed afterwards."""
    from mi355 import ops
    with G.window(ops, label):
        out = fn(*args, **kw)
    torch.cuda.synchronize()
    G.check(label)
    return out


def _gfeat(gpu, a, dtype, name='feature'):
    """_feat inside guards, and the row pitch of the calls that follow: one image row of it."""
    t = _feat(gpu, a, dtype)
    G.row_pitch(t.shape[3] * t.shape[1] * t.element_size())
    return G.place(t, name)


def _gdev(gpu, a, name):
    return G.place(torch.from_numpy(np.ascontiguousarray(a)).to(gpu), name)


def _gout(gpu, B, C, H, W, dtype, name='out'):
    """A channels_last feature gradient with nothing but the fill in it."""
    return G.empty((B, H, W, C), dtype, gpu, name).permute(0, 3, 1, 2)

POISON = -7777.25
KEYS = ('loss', 'grad_f1', 'grad_f2', 'desc1', 'desc2')


def _bits(a):
    if torch.is_tensor(a):
        a = a.detach()
        a = (a.float() if a.dtype == torch.bfloat16 else a).cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def _feat(gpu, a, dtype=torch.float32, grad=False):
    """(B, C, H, W) numpy array as a channels_last device tensor."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu).to(dtype).contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(True) if grad else t


def _nchw(t):
    return t.detach().float().cpu().numpy()


def _check(tag, got, ref32, ref64, stored_bf16=False):
    own, bound = jfa_ref.bounds(ref32, ref64)
    err = jfa_ref.errors(got, ref64)
    for k in err:
        b = bound[k]
        print('%s %s: kernel |err| %.3e; float32 reference %.3e; bound %.3e' % (tag, k, err[k], own[k], b))
        if stored_bf16 and k.startswith('grad'):
            r = np.asarray(ref64[k], np.float64)
            over = np.abs(np.asarray(got[k], np.float64) - r) - (b + 2.0 ** -8 * (np.abs(r) + b))
            print('%s %s: stored in bf16, largest excess over the element-wise allowance %.3e' % (tag, k, float(over.max())))
            assert (over <= 0).all(), (tag, k)
        else:
            assert err[k] <= b, (tag, k)
    assert set(err) == {k for k in ref64 if ref64[k] is not None and got.get(k) is not None}


def _run(gpu, f1, f2, p1, p2, dtype=torch.float32, up=None, **opts):
    """loss3 and loss1 of uda.model.loss through autograd: dict of loss, both feature gradients and both descriptors."""
    from mi355 import ops
    from uda.model.loss import loss1, loss3
    # inside guards: the features and key points are placed; the descriptors, rows, KL gradients and the feature gradients are
    # all made by the wrappers (torch.empty / torch.empty_like) while the window is open, the backward included
    a, b = _gfeat(gpu, f1, dtype, 'f1').requires_grad_(True), _gfeat(gpu, f2, dtype, 'f2').requires_grad_(True)
    x1, x2 = _gdev(gpu, np.asarray(p1, np.float32), 'pre1'), _gdev(gpu, np.asarray(p2, np.float32), 'pre2')
    label = 'loss3 + backward + loss1 %s %s' % (tuple(a.shape), dtype)
    with G.window(ops, label):
        loss = loss3(a, b, x1, x2, **opts)
        (loss if up is None else loss * up).backward()
        kw = {k: v for k, v in opts.items() if k != 'scale'}
        with torch.no_grad():
            d1, d2 = loss1(a, x1, **kw), loss1(b, x2, **kw)
    torch.cuda.synchronize()
    G.check(label)
    assert all(G.unwritten(t) == 0 for t in (a.grad, b.grad, d1, d2, loss.detach()))
    assert a.grad.dtype == dtype and ops_is_nhwc(a.grad) and d1.dtype == torch.float32
    return dict(loss=float(loss.detach()), grad_f1=_nchw(a.grad), grad_f2=_nchw(b.grad), desc1=d1.cpu().numpy(), desc2=d2.cpu().numpy())


def ops_is_nhwc(t):
    from mi355 import ops
    return ops.is_nhwc(t)


# ---------------------------------------------------------------- 1. the fixture
def _gold(g, case, suffix=''):
    sep = '_' if suffix else ''
    return dict(loss=float(g[case + '/loss' + suffix]), grad_f1=g[case + '/grad_f1' + sep + suffix], grad_f2=g[case + '/grad_f2' + sep + suffix],
                desc1=g[case + '/desc1' + sep + suffix], desc2=g[case + '/desc2' + sep + suffix])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', ['a', 'b'])
def test_kernels_against_the_reference(gpu, case, dtype):
    """Through uda.model.loss.loss1 / loss3 and autograd.  The fixture's features are exact in bf16 (multiples of 1/8 below 2), so
    the bf16 copy is the same problem; its gradients come back stored in bf16."""
    g = golden('g15_jfa')
    f1, f2, p1, p2 = (g[case + '/' + k] for k in ('f1', 'f2', 'pre1', 'pre2'))
    assert np.array_equal(jfa_ref.bf16_round(f1), f1) and np.array_equal(jfa_ref.bf16_round(f2), f2)
    got = _run(gpu, f1, f2, p1, p2, dtype)
    _check('fixture %s' % case, got, _gold(g, case), _gold(g, case, '64'), stored_bf16=dtype == torch.bfloat16)
    # a non-unit upstream gradient goes through the scale kernel
    up = _run(gpu, f1, f2, p1, p2, dtype, up=3.0)
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-6
    for k in ('grad_f1', 'grad_f2'):
        assert np.abs(up[k] - 3.0 * got[k]).max() <= tol * np.abs(3.0 * got[k]).max()
    # a plain NCHW fp32 tensor is accepted as the reference's callers would pass it
    from uda.model.loss import loss1
    d = loss1(torch.from_numpy(f1).to(gpu), torch.from_numpy(p1).to(gpu))
    assert _same(d, got['desc1'])                  # (exact operands: the same bits from the fp32 and the bf16 kernel)


# ---------------------------------------------------------------- 2. shapes where the tiling can go wrong
def _points(rng, B, K, H, W, kind='random'):
    """(x, y) key points inside the map, some on the border, some non-integer."""
    p = np.stack([rng.random((B, K)) * (W - 1), rng.random((B, K)) * (H - 1)], -1).astype(np.float32)
    p[:, ::3] = np.round(p[:, ::3])
    if K >= 4:
        p[:, 0], p[:, 1] = (0, 0), (W - 1, H - 1)
        p[:, 2], p[:, 3] = (0, H - 1), (W - 1, 0)
    return p


# jfa_pool / jfa_scatter: channel tiles of 256, 16-byte chunks (8 bf16 / 4 fp32 channels), 256 threads = G pixel groups x chunks,
# strips of 256 pixels; jfa_kl: one wave per row, 4 rows per block, 256 channels per pass of a wave
SHAPES = [
    # name        B  K   C    H   W   radius axes  dtype
    ('C8', 1, 21, 8, 64, 64, 6, 'ref', torch.float32),
    ('C8bf16', 3, 21, 8, 64, 64, 6, 'xy', torch.bfloat16),
    ('C40', 3, 21, 40, 64, 64, 6, 'ref', torch.float32),                   # 5 / 10 chunks: idle threads behind the last group
    ('C40bf16', 1, 1, 40, 64, 64, 6, 'ref', torch.bfloat16),               # K = 1
    ('C256', 1, 32, 256, 64, 64, 6, 'xy', torch.float32),                  # K = 32, 64 chunks a pixel
    ('C256bf16', 3, 21, 256, 64, 64, 1, 'ref', torch.bfloat16),            # radius 1: windows of one pixel
    ('C264', 1, 21, 264, 16, 16, 6, 'xy', torch.bfloat16),                 # a second channel tile of 8 channels
    ('map16', 3, 21, 40, 16, 16, 6, 'ref', torch.float32),                 # the window is larger than half the map
    ('map16r16', 1, 32, 8, 16, 16, 16, 'xy', torch.float32),               # ... larger than the map
    ('r16', 1, 21, 40, 64, 64, 16, 'ref', torch.bfloat16),                 # 32 x 32 windows
    ('m32x48xy', 3, 21, 40, 32, 48, 6, 'xy', torch.float32),               # non-square: a swapped axis or stride shows
    ('m32x48ref', 3, 21, 40, 32, 48, 6, 'ref', torch.float32),
    ('m48x32xy', 1, 21, 8, 48, 32, 6, 'xy', torch.bfloat16),
    ('m19x23', 1, 1, 8, 19, 23, 1, 'ref', torch.float32),                  # odd sides, 437 pixels: a partial second strip
]


@pytest.mark.parametrize('name,B,K,C,H,W,radius,axes,dtype', SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_shapes(gpu, name, B, K, C, H, W, radius, axes, dtype):
    rng = np.random.default_rng(len(name) * 977 + C + H)
    f1 = jfa_ref.bf16_round(rng.random((B, C, H, W)).astype(np.float32) * 2)
    f2 = jfa_ref.bf16_round((rng.random((B, C, H, W)) * (rng.random((B, C, H, W)) < 0.4)).astype(np.float32))     # sparse, as after a ReLU
    p1, p2 = _points(rng, B, K, H, W), _points(rng, B, K, H, W)
    if axes == 'ref':                 # the reference indexes the rows by x: keep the points inside the map under that reading
        p1, p2 = p1[..., ::-1].copy(), p2[..., ::-1].copy()
    scale = 0.3 if name == 'C40' else 1.0
    ref64 = dict(zip(KEYS, jfa_ref.loss3(f1, f2, p1, p2, radius, axes, scale, np.float64)))
    ref32 = dict(zip(KEYS, jfa_ref.loss3(f1, f2, p1, p2, radius, axes, scale, np.float32)))
    got = _run(gpu, f1, f2, p1, p2, dtype, radius=radius, axes=axes, scale=scale)
    _check(name, got, ref32, ref64, stored_bf16=dtype == torch.bfloat16)
    assert np.abs(ref64['grad_f1']).max() > 0 and np.abs(ref64['desc2']).max() > 0


def test_workload_shaped_case(gpu):
    """B = 4, C = 256, 64 x 64, bf16: the neck output's shape, blob-like sparse features."""
    rng = np.random.default_rng(64)
    B, K, C, H, W = 4, 21, 256, 64, 64
    f1 = jfa_ref.bf16_round((rng.random((B, C, H, W)) * (rng.random((B, C, H, W)) < 0.5)).astype(np.float32))
    f2 = jfa_ref.bf16_round((rng.random((B, C, H, W)) * (rng.random((B, C, H, W)) < 0.5)).astype(np.float32))
    p1 = (20 + rng.random((B, K, 2)) * 24).astype(np.float32)               # neighbouring joints: overlapping windows
    p2 = np.round(20 + rng.random((B, K, 2)) * 24).astype(np.float32)
    ref64 = dict(zip(KEYS, jfa_ref.loss3(f1, f2, p1, p2, 6, 'xy', 1.0, np.float64)))
    ref32 = dict(zip(KEYS, jfa_ref.loss3(f1, f2, p1, p2, 6, 'xy', 1.0, np.float32)))
    got = _run(gpu, f1, f2, p1, p2, torch.bfloat16, axes='xy')
    _check('workload', got, ref32, ref64, stored_bf16=True)


def test_empty_windows_and_joints_on_one_pixel(gpu):
    rng = np.random.default_rng(3)
    f1, f2 = rng.random((2, 8, 16, 16)).astype(np.float32), rng.random((2, 8, 16, 16)).astype(np.float32)
    out = np.array([[-7, 3], [3, -7], [40, 3], [3, 40], [1e9, 0], [-1e9, -1e9], [15.5, 22.5], [np.nan, 5], [5, np.nan],
                    [np.inf, 5], [5, -np.inf], [3e38, 3e38]], np.float32)
    p = np.stack([out, out[::-1]])
    got = _run(gpu, f1, f2, p, p, radius=6, axes='xy')
    assert (got['desc1'] == 0).all() and (got['desc2'] == 0).all() and np.isfinite(got['loss']) and abs(got['loss']) < 1e-6
    assert (got['grad_f1'] == 0).all() and (got['grad_f2'] == 0).all()
    assert not jfa_ref.covered(p, 16, 16, 6, 'xy').any() and not jfa_ref.covered(p, 16, 16, 6, 'ref').any()
    got = _run(gpu, f1, f2, p, p, radius=6, axes='ref')
    assert (got['desc1'] == 0).all() and (got['grad_f1'] == 0).all() and abs(got['loss']) < 1e-6
    # mixed: some empty, and all the others on one pixel
    p = np.tile(np.array([7.25, 9.5], np.float32), (2, 21, 1))
    p[:, ::4] = (-30, 5)
    ref64 = dict(zip(KEYS, jfa_ref.loss3(f1, f2, p, p[:, ::-1].copy(), 6, 'xy', 1.0, np.float64)))
    ref32 = dict(zip(KEYS, jfa_ref.loss3(f1, f2, p, p[:, ::-1].copy(), 6, 'xy', 1.0, np.float32)))
    got = _run(gpu, f1, f2, p, p[:, ::-1].copy(), radius=6, axes='xy')
    _check('one pixel', got, ref32, ref64)
    assert (got['desc1'][:, ::4] == 0).all() and _same(got['desc1'][:, 1], got['desc1'][:, 2])


# ---------------------------------------------------------------- 3. exact operands: bits
def _exact(gpu, B=2, K=21, C=40, H=32, W=48, radius=6, axes='xy', seed=8):
    rng = np.random.default_rng(seed)
    f = (rng.integers(0, 16, (B, C, H, W)) / 8).astype(np.float32)         # every window sum is exact in fp32 in any order
    p = _points(rng, B, K, H, W)
    p[:, 5:8] = p[:, 4:5]                                                  # three joints on one pixel
    p[:, 8] = (-40, 3)                                                     # an empty window
    if axes == 'ref':
        p = p[..., ::-1].copy()
    return rng, f, p


@pytest.mark.parametrize('axes', ['xy', 'ref'])
def test_pool_is_bit_identical_on_exact_operands(gpu, axes):
    from mi355 import ops
    rng, f, p = _exact(gpu, axes=axes)
    xy = _gdev(gpu, p, 'xy')
    want = (jfa_ref.pool(f, p, 6, axes, np.float64) * 169).astype(np.float32) / np.float32(169)
    for dtype in (torch.bfloat16, torch.float32):
        d = _guard('joint_pool %s %s' % (axes, dtype), ops.joint_pool, _gfeat(gpu, f, dtype), xy, 6, axes)
        d2 = _guard('joint_pool %s %s again' % (axes, dtype), ops.joint_pool, _gfeat(gpu, f, dtype), xy, 6, axes)
        assert G.unwritten(d) == 0 and G.unwritten(d2) == 0
        assert _same(d, want) and _same(d, d2), dtype
    assert (want[:, 8] == 0).all() and want.max() > 0.5


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('axes', ['xy', 'ref'])
def test_scatter_is_bit_identical_with_the_fixed_order_model(gpu, axes, dtype):
    from mi355 import ops
    B, K, C, H, W = 2, 21, 40, 32, 48
    rng, f, p = _exact(gpu, B, K, C, H, W, axes=axes)
    xy = _gdev(gpu, p, 'xy')
    gd = rng.standard_normal((B, K, C)).astype(np.float32)
    rnd = jfa_ref.bf16_round if dtype == torch.bfloat16 else None
    want, cov = jfa_ref.scatter_model(gd, p, (B, H, W, C), 6, axes, round_to=rnd)
    assert cov.any() and not cov.all()
    gdev = _gdev(gpu, gd, 'gd')
    G.row_pitch(W * C * (2 if dtype == torch.bfloat16 else 4))
    out = _gout(gpu, B, C, H, W, dtype)
    _guard('joint_scatter = %s %s' % (axes, dtype), ops.joint_scatter, gdev, xy, out, False, 6, axes)
    assert G.unwritten(out) == 0
    got = out.permute(0, 2, 3, 1).float().cpu().numpy()
    assert _same(got, want)
    assert (got[~cov] == 0).all() and not np.signbit(got[~cov]).any()                      # +0 outside every window
    # accumulate mode onto a poisoned-then-filled buffer
    base = rng.standard_normal((B, H, W, C)).astype(np.float32)
    base = jfa_ref.bf16_round(base) if dtype == torch.bfloat16 else base
    out.fill_(POISON)
    out.copy_(torch.from_numpy(base).to(gpu).permute(0, 3, 1, 2))
    _guard('joint_scatter += %s %s' % (axes, dtype), ops.joint_scatter, gdev, xy, out, True, 6, axes)
    again = out.clone()
    torch.cuda.synchronize()
    want_acc, _ = jfa_ref.scatter_model(gd, p, (B, H, W, C), 6, axes, onto=base, round_to=rnd)
    got = out.permute(0, 2, 3, 1).float().cpu().numpy()
    assert _same(got, want_acc)
    assert _bits(got[~cov]) == _bits(base[~cov]) and not np.array_equal(got[cov], base[cov])
    # two runs give the same bits
    out.copy_(torch.from_numpy(base).to(gpu).permute(0, 3, 1, 2))
    _guard('joint_scatter += %s %s again' % (axes, dtype), ops.joint_scatter, gdev, xy, out, True, 6, axes)
    assert _same(out, again)


# key points on the four corners of the first and of the last image, windows of one pixel and windows larger than the map
CORNER_C = [8, 264]               # one chunk; a second channel tile of one bf16 chunk / two fp32 chunks behind 256 channels


def _corners(B, K, H, W, axes):
    assert K == 4
    p = np.tile(np.array([[0, 0], [W - 1, H - 1], [0, H - 1], [W - 1, 0]], np.float32), (B, 1, 1))
    return p[..., ::-1].copy() if axes == 'ref' else p


@pytest.mark.parametrize('radius', [1, 16])
@pytest.mark.parametrize('C', CORNER_C)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('axes', ['xy', 'ref'])
def test_pool_and_scatter_at_the_corners_of_the_first_and_last_image(gpu, axes, dtype, C, radius):
    """B = 2, K = 4, a 5 x 7 map: the windows touch the first and the last pixel of the feature map, which sit against the guard
    flanks; with C = 264 the last thread of the second channel tile idles."""
    from mi355 import ops
    B, K, H, W = 2, 4, 5, 7
    rng = np.random.default_rng(C * 10 + radius)
    f = (rng.integers(0, 16, (B, C, H, W)) / 8).astype(np.float32)         # every window sum is exact in fp32 in any order
    p = _corners(B, K, H, W, axes)
    win = jfa_ref.windows(p, H, W, radius, axes)
    assert ((win[..., 1] > win[..., 0]) & (win[..., 3] > win[..., 2])).all() and (win[:, 0, [0, 2]] == 0).all()
    xy = _gdev(gpu, p, 'xy')
    div = (2 * radius + 1) ** 2
    want = (jfa_ref.pool(f, p, radius, axes, np.float64) * div).astype(np.float32) / np.float32(div)
    d = _guard('joint_pool corners', ops.joint_pool, _gfeat(gpu, f, dtype), xy, radius, axes)
    assert G.unwritten(d) == 0 and _same(d, want) and want.max() > 0
    gd = rng.standard_normal((B, K, C)).astype(np.float32)
    rnd = jfa_ref.bf16_round if dtype == torch.bfloat16 else None
    want_g, cov = jfa_ref.scatter_model(gd, p, (B, H, W, C), radius, axes, round_to=rnd)
    assert cov[0, 0, 0] and cov[B - 1].any() and not cov.all()
    gdev = _gdev(gpu, gd, 'gd')
    out = _gout(gpu, B, C, H, W, dtype)
    _guard('joint_scatter = corners', ops.joint_scatter, gdev, xy, out, False, radius, axes)
    assert G.unwritten(out) == 0 and _same(out.permute(0, 2, 3, 1).float().cpu().numpy(), want_g)
    base = rng.standard_normal((B, H, W, C)).astype(np.float32)
    base = jfa_ref.bf16_round(base) if dtype == torch.bfloat16 else base
    acc = G.place(torch.from_numpy(base).to(gpu).to(dtype), 'out +=').permute(0, 3, 1, 2)
    _guard('joint_scatter += corners', ops.joint_scatter, gdev, xy, acc, True, radius, axes)
    want_acc, _ = jfa_ref.scatter_model(gd, p, (B, H, W, C), radius, axes, onto=base, round_to=rnd)
    assert _same(acc.permute(0, 2, 3, 1).float().cpu().numpy(), want_acc)


def test_two_runs_give_the_same_bits(gpu):
    rng = np.random.default_rng(21)
    f1, f2 = rng.random((3, 40, 32, 48)).astype(np.float32), rng.random((3, 40, 32, 48)).astype(np.float32)
    p1, p2 = _points(rng, 3, 21, 32, 48), _points(rng, 3, 21, 32, 48)
    a, b = (_run(gpu, f1, f2, p1, p2, torch.bfloat16, axes='xy') for _ in range(2))
    assert a['loss'] == b['loss'] and all(_same(a[k], b[k]) for k in KEYS[1:])


# ---------------------------------------------------------------- 4. gradient requests
@pytest.mark.parametrize('want', [(True, False), (False, True), (True, True), (False, False)], ids=['a', 'b', 'both', 'neither'])
def test_gradient_requests(gpu, want):
    from mi355 import ops
    rng = np.random.default_rng(5)
    a, b = rng.random((3, 21, 40)).astype(np.float32), rng.random((3, 21, 40)).astype(np.float32)
    ad, bd = _gdev(gpu, a, 'a'), _gdev(gpu, b, 'b')
    # both gradient buffers are handed over whatever is wanted, as neighbours inside one poisoned allocation with guard zones:
    # a side that is not wanted, and everything around a side that is, must keep the poison
    n = ad.numel()
    flat = G.place(torch.full((3 * n + 64,), POISON, device=gpu), 'gradients')
    ga, gb = flat[32:32 + n].view(ad.shape), flat[32 + n:32 + 2 * n].view(bd.shape)
    assert ga.data_ptr() % 16 == 0 and gb.data_ptr() % 16 == 0
    G.row_pitch(a.shape[-1] * 4)
    rows, ra, rb = _guard('joint_kl %s' % (want,), ops.joint_kl, ad, bd, want[0], want[1], 0.5, grad_a=ga, grad_b=gb)
    loss = _guard('reduce_sum', ops.reduce_sum, rows.view(-1), 0.5 / rows.numel())
    assert G.unwritten(rows) == 0 and G.unwritten(loss) == 0
    # ... and with the gradients left to the wrapper (torch.empty_like inside the window): the same bits, all of them written
    rows2, ra2, rb2 = _guard('joint_kl %s, own gradients' % (want,), ops.joint_kl, ad, bd, want[0], want[1], 0.5)
    assert _same(rows2, rows) and G.unwritten(rows2) == 0
    for mine, theirs, w in ((ra2, ga, want[0]), (rb2, gb, want[1])):
        assert (mine is None) == (not w) and (not w or (G.unwritten(mine) == 0 and _same(mine, theirs)))
    assert (ra is None) == (not want[0]) and (rb is None) == (not want[1])
    l64, r64, ga64, gb64 = jfa_ref.kl(a, b, 0.5, np.float64)
    l32, r32, ga32, gb32 = jfa_ref.kl(a, b, 0.5, np.float32)
    got = dict(loss=float(loss), grad_f1=ga.cpu().numpy() if want[0] else None, grad_f2=gb.cpu().numpy() if want[1] else None)
    _check('kl %s' % (want,), got, dict(loss=l32, grad_f1=ga32, grad_f2=gb32),
           dict(loss=l64, grad_f1=ga64 if want[0] else None, grad_f2=gb64 if want[1] else None))
    assert np.allclose(rows.cpu().numpy(), r64, rtol=1e-4, atol=1e-7)
    for g, w in ((ga, want[0]), (gb, want[1])):
        assert (g == POISON).all() if not w else not (g == POISON).any()    # an unwanted buffer keeps its poison, a wanted one none
    assert (flat[:32] == POISON).all() and (flat[32 + 2 * n:] == POISON).all()
    # through autograd: only the side that requires a gradient gets one
    from uda.model.loss import joint_kl_loss
    x, y = ad.clone().requires_grad_(want[0]), bd.clone().requires_grad_(want[1])
    out = joint_kl_loss(x, y, 0.5)
    if any(want):
        out.backward()
        assert (x.grad is not None) == want[0] and (y.grad is not None) == want[1]
        assert not want[0] or _same(x.grad, ga)
        assert not want[1] or _same(y.grad, gb)
    assert float(out.detach()) == float(loss)


# ---------------------------------------------------------------- 5. refused arguments
def test_refused_arguments_launch_nothing(gpu):
    import mi355
    from mi355 import ops
    from uda.model.loss import loss1, loss3
    z = lambda *shape: torch.zeros(shape, device=gpu)
    f = ops.nhwc_empty(2, 16, 8, 8, torch.bfloat16, gpu).zero_()
    xy, d = z(2, 21, 2), z(2, 21, 16)
    flat = torch.zeros(2 * 16 * 8 * 8 + 8, dtype=torch.float32, device=gpu)
    off = flat[1:1 + 2048].view(2, 8, 8, 16).permute(0, 3, 1, 2)               # one element off a 16-byte boundary: refused
    assert ops.is_nhwc(off) and off.data_ptr() % 16 == 4
    doff = torch.zeros(2 * 21 * 16 + 8, device=gpu)[1:1 + 672].view(2, 21, 16)
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    try:
        bad = [
            lambda: ops.joint_pool(off, xy),
            lambda: ops.joint_pool(f, xy, out=doff),
            lambda: ops.joint_scatter(d, xy, off, False),
            lambda: ops.joint_scatter(doff, xy, f, True),
            lambda: ops.joint_kl(doff, d, False, False),
            lambda: ops.joint_kl(d, d, True, False, grad_a=doff),
            lambda: ops.joint_pool(ops.nhwc_empty(2, 12, 8, 8, torch.float32, gpu), xy),       # C not a multiple of 8
            lambda: ops.joint_pool(ops.nhwc_empty(2, 4, 8, 8, torch.float32, gpu), xy),        # C < 8
            lambda: ops.joint_pool(f, z(2, 33, 2)),                                            # K outside 1 .. 32
            lambda: ops.joint_pool(f, z(2, 0, 2)),
            lambda: ops.joint_pool(f, z(3, 21, 2)),                                            # another batch size
            lambda: ops.joint_pool(f, z(2, 21, 3)),
            lambda: ops.joint_pool(f, xy.double()),
            lambda: ops.joint_pool(f, xy, radius=0),
            lambda: ops.joint_pool(f, xy, radius=-6),
            lambda: ops.joint_pool(f, xy, radius=2.5),
            lambda: ops.joint_pool(f, xy, axes='yx'),
            lambda: ops.joint_pool(f, xy, divisor=0.0),
            lambda: ops.joint_pool(f.contiguous(), xy),                                        # NCHW memory
            lambda: ops.joint_pool(f.half(), xy),
            lambda: ops.joint_pool(f, xy, out=z(2, 21, 8)),                                    # a buffer of another shape
            lambda: ops.joint_pool(f.cpu(), xy.cpu()),
            lambda: ops.joint_kl(d, z(2, 21, 8), False, False),
            lambda: ops.joint_kl(z(2, 21, 12), z(2, 21, 12), False, False),
            lambda: ops.joint_kl(d, d, False, False, rows=z(41)),
            lambda: ops.joint_kl(d, d, True, False, grad_a=z(2, 21, 8)),
            lambda: ops.joint_kl(d.cpu(), d.cpu(), False, False),
            lambda: ops.joint_scatter(z(2, 20, 16), xy, f, False),
            lambda: ops.joint_scatter(d, xy, f.contiguous(), False),
            lambda: ops.joint_scatter(d, xy, f, False, radius=0),
            lambda: ops.joint_scatter(d, z(2, 33, 2), f, False),
        ]
        for i, fn in enumerate(bad):
            with pytest.raises(mi355.Mi355Error):
                fn()
                pytest.fail('case %d was accepted' % i)
        with pytest.raises(ValueError):
            loss1(z(2, 16, 8), xy)
        with pytest.raises(ValueError):
            loss3(f, f, xy, z(3, 21, 2))
        torch.cuda.synchronize()
        assert ops.prof_launches() == []
        g = ops.joint_kl(ops.joint_pool(f, xy), d, True, False)[1]
        ops.joint_scatter(g, xy, f, True)
        torch.cuda.synchronize()
        assert [e['label'].split()[0] for e in ops.prof_launches()] == ['jfa_pool', 'jfa_kl', 'jfa_scatter']
    finally:
        ops.prof_enable(0); ops.prof_reset()


# ---------------------------------------------------------------- 6. the gradient fan-in of the neck output
@pytest.mark.parametrize('order', ['pool_first', 'pool_middle', 'pool_last'])
def test_pooling_joins_the_gradient_fan_in(gpu, order):
    """Two mi355.nn.Conv2d heads and the pooling consume one tensor that carries a GradFanIn.  Backward runs in the reverse of the
    recording order, so the three recordings put the pooling's backward last, between the convs' and first.  The tensor's
    gradient is the sum of the three separately computed ones within the bf16 roundings of the buffer; a pooling
    that handed autograd a dense tensor beside an existing buffer would lose a conv's addition."""
    import mi355
    from mi355 import nn as mnn
    from uda.model.loss import loss1
    mi355.set_compute_dtype('bf16')
    rng = np.random.default_rng(11)
    B, C, H, W, K = 2, 64, 16, 16, 21
    torch.manual_seed(5)
    convs = [mnn.Conv2d(C, C, 3, 1, 1, bias=False).to(gpu) for _ in range(2)]
    x0 = _feat(gpu, rng.standard_normal((B, C, H, W)), torch.bfloat16)
    xy = torch.from_numpy(_points(rng, B, K, H, W)).to(gpu)
    wy = [torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32)).to(gpu) for _ in range(2)]
    wd = torch.from_numpy((rng.standard_normal((B, K, C)) * 169).astype(np.float32)).to(gpu)

    def run(which, order='pool_last', fan=True):
        leaf = x0.clone().requires_grad_(True)
        x = leaf * 1.0
        assert ops_is_nhwc(x) and x.dtype == torch.bfloat16
        if fan:
            x._mi_fan = mnn.GradFanIn()
        terms = {}
        seq = {'pool_first': ('p', 0, 1), 'pool_middle': (0, 'p', 1), 'pool_last': (0, 1, 'p')}[order]
        for s in seq:
            if s not in which:
                continue
            if s == 'p':
                terms[s] = (loss1(x, xy, 6, 'xy') * wd).sum()
            else:
                terms[s] = (convs[s](x).float() * wy[s]).sum()
        sum(terms.values()).backward()
        torch.cuda.synchronize()
        return leaf.grad.float().cpu().numpy()

    parts = [run((w,), fan=False) for w in (0, 1, 'p')]
    assert all(np.abs(p).max() > 0 for p in parts)
    mags = [np.abs(p).max() for p in parts]
    assert max(mags) < 30 * min(mags), mags                                 # every consumer matters at the tolerance below
    got = run((0, 1, 'p'), order)
    want = parts[0].astype(np.float64) + parts[1] + parts[2]
    # six bf16 roundings of at most 2^-8 of sum |part| each: one per separately computed part, one per write / addition here
    tol = 6 * 2.0 ** -8 * (np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2])) + 1e-30
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / tol).max())
    for drop in range(3):                                                   # the tolerance does tell a lost consumer
        less = want - parts[drop]
        assert not (np.abs(got - less) <= tol).all()


# ---------------------------------------------------------------- 7. the iteration
W_JFA = 0.5


def _host(module):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in module.state_dict().items()}


def _training(gpu, mode):
    """mode: 'on' (DAStep with the term), 'off' (jfa=None passed explicitly), 'plain' (a DAStep built without the argument)."""
    import mi355
    from mi355.da_step import DAStep, JointFeatureAlign, build_training
    from uda.model.regda_7 import PoseResNetx9
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('bf16')
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=32)
    if mode != 'plain':
        step = DAStep(model, opts, step.crit, step.trade_off, step.skip, step.track_acc,
                      jfa=JointFeatureAlign(weight=W_JFA, radius=3, axes='xy') if mode == 'on' else None)
    assert getattr(step, 'jfa', None) is None or mode == 'on'
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    return model, step, scheds


def _iterate(gpu, mode, iters, capture_at=None):
    from utils.synthetic import make_batch
    from uda.model.loss import joint_kl_loss
    model, step, scheds = _training(gpu, mode)
    batch = make_batch(2, 128, 32, seed=3, device=gpu)
    rec = dict(model=[], loss_gt=[], loss_jfa=[], again=[], desc=[])
    for i in range(iters):
        if capture_at is not None and i == capture_at:
            step.capture(batch, warmup=0)
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        torch.cuda.synchronize()
        rec['model'].append(_host(model))
        rec['loss_gt'].append(float(out['loss_gt']))
        if mode == 'on':
            rec['loss_jfa'].append(float(out['loss_jfa']))
            rec['again'].append(float(joint_kl_loss(out['jfa_desc_t'], out['jfa_desc_s'], W_JFA)))
            rec['desc'].append((out['jfa_desc_t'].cpu().numpy().copy(), out['jfa_desc_s'].cpu().numpy().copy()))
        else:
            assert 'loss_jfa' not in out and 'jfa_desc_s' not in out
    return rec, step, batch


@pytest.fixture(scope='module')
def runs(gpu):
    import mi355
    try:
        eager, _, _ = _iterate(gpu, 'on', 5)
        graph, step, _ = _iterate(gpu, 'on', 5, capture_at=3)
        assert step.graphs is not None and len(step.graphs) == 6
        off, _, _ = _iterate(gpu, 'off', 2)
        plain, _, _ = _iterate(gpu, 'plain', 2)
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(eager=eager, graph=graph, off=off, plain=plain)


def test_step_eager_and_replay_agree_bit_for_bit(runs):
    a, b = runs['eager'], runs['graph']
    assert a['loss_jfa'] == b['loss_jfa'] and a['loss_gt'] == b['loss_gt'] and len(set(a['loss_jfa'])) == 5
    for it in range(5):                                             # iterations 3 and 4 of `graph` are replays
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)


def test_step_off_equals_a_step_built_without_the_argument(runs):
    a, b = runs['off'], runs['plain']
    assert a['loss_gt'] == b['loss_gt']
    for it in range(2):
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)


def test_step_loss_jfa_is_the_recomputed_term(runs):
    for name in ('eager', 'graph'):
        r = runs[name]
        for got, again, (d_t, d_s) in zip(r['loss_jfa'], r['again'], r['desc']):
            assert got == again and got > 0                         # the same kernel on the dumped descriptors outside the step
            assert d_t.shape == d_s.shape == (2, 21, 256) and d_s.min() >= 0 and d_s.max() > 0
            l64 = jfa_ref.kl(d_t, d_s, W_JFA, np.float64)[0]
            l32 = jfa_ref.kl(d_t, d_s, W_JFA, np.float32)[0]
            assert abs(got - float(l64)) <= max(4 * abs(float(l32) - float(l64)), jfa_ref.LOSS_FLOOR * abs(float(l64)))


def test_step_moves_the_feature_extractor_and_nothing_else(runs):
    """After one iteration: the parameters optimizer_f steps (backbone, neck) differ from the off run, the heads' -- which only
    change in steps A and B -- do not."""
    on, off = runs['eager']['model'][0], runs['off']['model'][0]
    assert not _same(on['backbone.layer1.0.conv1.weight'], off['backbone.layer1.0.conv1.weight'])
    assert any(k.startswith('upsampling.') and on[k].dtype.kind == 'f' and not _same(on[k], off[k]) for k in on)
    heads = [k for k in on if k.startswith(('head.', 'head_adv.', 'head_adv2.', 'head_adv3.'))]
    assert len(heads) >= 8
    for k in heads:
        assert _same(on[k], off[k]), k


def test_step_launch_log(gpu):
    """An iteration with `jfa` on holds one jfa_pool in step A (the source descriptors) and one jfa_pool, one jfa_kl (the gradient of
    the target side only) and one jfa_scatter in step C; with `jfa` off an iteration holds none."""
    import mi355
    from mi355 import ops
    from utils.synthetic import make_batch
    try:
        batch = make_batch(2, 128, 32, seed=3, device=gpu)
        logs = {}
        for mode in ('on', 'off'):
            model, step, scheds = _training(gpu, mode)
            step.run(batch)
            inner = step._fwdbwd_C
            seen = {}

            def logged_C(b, inner=inner, seen=seen):
                torch.cuda.synchronize()
                seen['before'] = [e['label'] for e in ops.prof_launches()]
                ops.prof_reset()
                inner(b)
                torch.cuda.synchronize()
                seen['C'] = [e['label'] for e in ops.prof_launches()]
                ops.prof_reset()

            step._fwdbwd_C = logged_C
            torch.cuda.synchronize()
            ops.prof_reset(); ops.prof_enable(2)
            try:
                step.run(batch)
                torch.cuda.synchronize()
                seen['after'] = [e['label'] for e in ops.prof_launches()]
            finally:
                ops.prof_enable(0); ops.prof_reset()
            logs[mode] = seen
        on, off = logs['on'], logs['off']
        assert len(on['C']) > 50 and len(on['before']) > 100
        assert [l.split()[0] for l in on['before'] if l.startswith('jfa_')] == ['jfa_pool']
        assert [l.split()[0] for l in on['C'] if l.startswith('jfa_')] == ['jfa_pool', 'jfa_kl', 'jfa_scatter']
        kl = [l for l in on['C'] if l.startswith('jfa_kl')][0]
        assert kl.split()[1:] == ['rows42', 'C256', 'grads10'], kl
        print([l for l in on['C'] if l.startswith('jfa_scatter')][0])
        assert not any(l.startswith('jfa_') for l in on['after'])
        assert not any(l.startswith('jfa_') for l in off['before'] + off['C'] + off['after'])
        assert len(on['C']) >= len(off['C']) + 3 and len(on['before']) >= len(off['before']) + 1
    finally:
        mi355.set_compute_dtype('bf16')
