"""MMD alignment on the GPU: the mmd_dist / mmd_coef / mmd_grad launches of mi355_mmd_heatmap against the reference's own
MMD_loss3 / MMD_loss (tests/golden/g14_mmd.npz) and against the closed form of tests/mmd_ref.py in float64, at the shapes where
the tiling can go wrong and at the workload's row length; their bit-level properties; the refused arguments; DAStep's `mmd`.

The tolerance, everywhere: a kernel result may be as far from the float64 result as 4 times the distance of a float32 run of the
reference expression from it (the fixture's float32 arrays for the fixture cases, mmd_ref in float32 otherwise), with floors of
5e-7 relative on the loss and 1e-6 of max |grad| on each gradient (mmd_ref.bounds; tests/test_mmd_cpu.py shows the reference's own
float32 run to stay below the floors).

Guards (tests/guarded.py).  Every launch of sections 2 - 4 goes through _kernels: source, target and the gradient buffers of a
side that is not wanted (poisoned, and required to keep the poison) are G.place() copies, the wanted gradients are G.empty()
buffers handed in through grad_source= / grad_target=, rows and the scalar come from torch.empty inside the window, and the
wrapper's workspace cache (ops._mmd_ws) is emptied with monkeypatch for the call, so the (K, n, n) matrices sit in exactly
mi355_mmd_workspace(B, K) bytes between two flanks.  The row pitch is HW * 4.  The fixture test of section 1 goes through the
loss classes and autograd with the window open over forward and backward: the wrapper makes rows, both gradients
(torch.empty_like) and the workspace inside it.  Sections 5 and 6 launch nothing or run DAStep."""
import numpy as np
import pytest
import torch

from conftest import golden
import guarded as G
import mmd_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guards():
    G.reset()
    yield
    G.reset()

POISON = np.float32(-7777.25)


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def _dev(gpu, a, offset=0, name='operand'):
    """`a` on the device; offset 1: as a contiguous view that starts one float behind a 16-byte boundary."""
    a = np.ascontiguousarray(a, np.float32)
    v = G.place(torch.from_numpy(a).to(gpu), name, start=G.START + 4 * offset)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * offset
    return v


def _kernels(gpu, s, t, want=(True, True), offset=0, scale=1.0, own_grads=True, **opts):
    """(loss, rows, grad_source, grad_target) of the launches; the gradient buffers are poisoned first and, when a side is not
    wanted, handed back as they are."""
    import mi355
    from mi355 import ops
    B, K = s.shape[:2]
    G.row_pitch(int(np.prod(s.shape[2:])) * 4)
    sd, td = _dev(gpu, s, offset, 'source'), _dev(gpu, t, offset, 'target')
    gs, gt = [G.empty(x.shape, torch.float32, gpu, n, start=G.START + 4 * offset) if w else _dev(gpu, np.full(x.shape, POISON), offset, n)
              for x, w, n in ((s, want[0], 'grad_source'), (t, want[1], 'grad_target'))]
    label = 'mmd_heatmap B%d K%d %s want %s' % (B, K, s.shape[2:], want)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, '_mmd_ws', {})                   # the workspace is allocated inside the window, at the library's size
        with G.window(ops, label):
            rows, a, b = ops.mmd_heatmap(sd, td, want[0], want[1], scale=scale, grad_source=gs if want[0] and own_grads else None,
                                         grad_target=gt if want[1] and own_grads else None, **opts)
            loss = ops.reduce_sum(rows, float(scale) / rows.numel())
        if not own_grads:                                # the wrapper's own torch.empty_like, made inside the window
            gs, gt = a if want[0] else gs, b if want[1] else gt
        (work,) = ops._mmd_ws.values()
    need = int(mi355.load().mi355_mmd_workspace(B, K))
    assert need == K * 4 * B * B * 4 and work.numel() * 4 == need and G._buf_of(work).n == need      # a guarded buffer of exactly that size
    torch.cuda.synchronize()
    G.check(label)
    assert G.unwritten(work) == 0 and G.unwritten(rows) == 0 and G.unwritten(loss) == 0
    assert all(G.unwritten(g) == 0 for g, w in ((gs, want[0]), (gt, want[1])) if w)
    assert _same(sd, s) and _same(td, t)                                # the inputs are only read
    assert (a is None) == (not want[0]) and (b is None) == (not want[1])
    _kernels.work = work
    return float(loss), rows.cpu().numpy(), gs.cpu().numpy(), gt.cpu().numpy()


def _check(tag, got, ref32, ref64, want=(True, True)):
    loss, _, gs, gt = got
    own, bound = mmd_ref.bounds(ref32[0], ref32[1], ref32[2], ref64[0], ref64[1], ref64[2])
    err = (abs(loss - float(ref64[0])), float(np.abs(gs.astype(np.float64) - ref64[1]).max()) if want[0] else 0.0,
           float(np.abs(gt.astype(np.float64) - ref64[2]).max()) if want[1] else 0.0)
    print('%s: kernel |err| loss %.3e grad_source %.3e grad_target %.3e; float32 reference %.3e %.3e %.3e; bound %.3e %.3e %.3e'
          % ((tag,) + err + own + bound))
    assert all(e <= b for e, b in zip(err, bound)), tag
    return err, bound


# ---------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
def test_kernels_against_the_reference(gpu, case):
    """Through the public classes and autograd: MMD_loss3 (a - c) and MMD_loss (d), loss and both gradients."""
    from uda.model.loss import MMD_loss, MMD_loss3
    g = golden('g14_mmd')
    from mi355 import ops
    G.row_pitch(int(np.prod(g[case + '/source'].shape[2:] if case != 'd' else g[case + '/source'].shape[1:])) * 4)
    s = G.place(torch.from_numpy(g[case + '/source']).to(gpu), 'source').requires_grad_(True)
    t = G.place(torch.from_numpy(g[case + '/target']).to(gpu), 'target').requires_grad_(True)
    crit = MMD_loss() if case == 'd' else MMD_loss3()
    assert (crit.kernel_mul, crit.kernel_num, crit.fix_sigma) == (2.0, 5, None)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, '_mmd_ws', {})                   # rows, both gradients (torch.empty_like) and the workspace: inside the window
        with G.window(ops, 'MMD fixture ' + case):
            loss = crit(s, t)
            loss.backward()
    torch.cuda.synchronize()
    G.check('MMD fixture ' + case)
    assert G.unwritten(s.grad) == 0 and G.unwritten(t.grad) == 0 and G.unwritten(loss.detach()) == 0
    got = (float(loss.detach()), None, s.grad.cpu().numpy(), t.grad.cpu().numpy())
    ref32 = (g[case + '/loss'], g[case + '/grad_source'], g[case + '/grad_target'])
    ref64 = (g[case + '/loss64'], g[case + '/grad_source64'], g[case + '/grad_target64'])
    _check('fixture ' + case, got, ref32, ref64)
    if case == 'd':
        from uda.model.loss import mmd_rbf
        assert float(mmd_rbf(s.detach(), t.detach(), 2.0, 5, None)) == float(loss.detach())
    # a non-unit upstream gradient goes through the scale kernel
    s2 = s.detach().clone().requires_grad_(True)
    (crit(s2, t.detach()) * 3.0).backward()
    assert np.allclose(s2.grad.cpu().numpy(), 3.0 * got[2], rtol=1e-6, atol=0)


# ---------------------------------------------------------------- 2. shapes where the tiling can go wrong
def _operands(seed, B, K, shape):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, K) + shape).astype(np.float32)
    t = (0.8 * rng.standard_normal((B, K) + shape) + 0.25).astype(np.float32)
    return s, t


# mmd_dist: 32 x 32 tiles of row pairs, HW in chunks of 64; mmd_grad: blocks of 16 rows by 1024 columns
SHAPES = [
    ('B1', 1, 21, (8, 8), {}, 0),                                   # n = 2
    ('n14', 7, 3, (4, 4), {}, 0),                                   # one below / above 16 rows (mmd_grad, both sides wanted)
    ('n18', 9, 3, (4, 4), {}, 0),
    ('n30', 15, 2, (4, 4), {}, 0),                                  # one below / above 32 rows (mmd_dist); 15 / 17 rows per side
    ('n34', 17, 2, (4, 4), {}, 0),                                  # ... around mmd_grad's 16 when one side is wanted
    ('n66', 33, 1, (3, 4), {}, 0),                                  # three tiles a side, the last nearly empty
    ('HW35', 2, 21, (5, 7), {}, 0),                                 # scalar path
    ('HW68', 3, 2, (4, 17), {}, 0),                                 # one float4 above the chunk of mmd_dist
    ('HW1028', 2, 2, (4, 257), {}, 0),                              # one float4 above the chunk of mmd_grad
    ('HW1027', 2, 2, (13, 79), {}, 0),                              # the same on the scalar path
    ('unaligned', 3, 21, (8, 8), {}, 1),                            # HW % 4 == 0 but the views start 4 bytes off: scalar path
    ('K1', 4, 1, (8, 8), {}, 0),
    ('kernels1', 2, 21, (8, 8), dict(kernel_num=1), 0),
    ('kernels8', 2, 21, (8, 8), dict(kernel_num=8, kernel_mul=1.5), 0),
    ('fix_sigma', 3, 21, (8, 8), dict(fix_sigma=90.0), 0),
    ('scale', 3, 5, (8, 8), dict(kernel_num=4, kernel_mul=3.0), 0),
]


@pytest.mark.parametrize('name,B,K,shape,opts,offset', SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_shapes(gpu, name, B, K, shape, opts, offset):
    s, t = _operands(len(name) * 131 + B, B, K, shape)
    scale = 0.3 if name == 'scale' else 1.0
    ref64 = mmd_ref.mmd(s, t, scale=scale, dtype=np.float64, **opts)
    ref32 = mmd_ref.mmd(s, t, scale=scale, dtype=np.float32, **opts)
    got = _kernels(gpu, s, t, offset=offset, scale=scale, **opts)
    _check(name, got, (ref32[0], ref32[2], ref32[3]), (ref64[0], ref64[2], ref64[3]))
    assert np.allclose(got[1], ref64[1], rtol=1e-5, atol=1e-6)                  # the per-joint rows
    if offset == 0 and np.prod(shape) % 4 == 0:
        # the scalar path stages the same LDS image and sums in the same order: the same bits as the float4 path
        off1 = _kernels(gpu, s, t, offset=1, scale=scale, **opts)
        assert off1[0] == got[0] and _same(off1[1], got[1]) and _same(off1[2], got[2]) and _same(off1[3], got[3])


@pytest.mark.parametrize('want', [(True, False), (False, True), (True, True), (False, False)], ids=['source', 'target', 'both', 'neither'])
@pytest.mark.parametrize('B', [15, 17])
def test_gradient_requests(gpu, B, want):
    """A side that was not requested is not written (the buffer keeps its poison); a requested side is the same bits whatever
    else was requested; the loss does not depend on the request."""
    s, t = _operands(77 + B, B, 2, (4, 5))
    ref64 = mmd_ref.mmd(s, t, dtype=np.float64)
    ref32 = mmd_ref.mmd(s, t, dtype=np.float32)
    both = _kernels(gpu, s, t)
    got = _kernels(gpu, s, t, want=want)
    assert all(_same(x, y) for x, y in zip(got[1:], _kernels(gpu, s, t, want=want, own_grads=False)[1:]))      # gradients the wrapper allocates
    assert got[0] == both[0] and _same(got[1], both[1])
    for side, g, full in ((0, got[2], both[2]), (1, got[3], both[3])):
        if want[side]:
            assert _same(g, full)
        else:
            assert _same(g, np.full(s.shape, POISON))
    _check('B%d %s' % (B, want), got, (ref32[0], ref32[2], ref32[3]), (ref64[0], ref64[2], ref64[3]), want)


# ---------------------------------------------------------------- 3. the workload's row length
def _blobs(rng, B, K, H, W, jitter):
    cy, cx = rng.random((B, K, 1, 1)) * (H - 1), rng.random((B, K, 1, 1)) * (W - 1)
    yy, xx = np.arange(H).reshape(1, 1, H, 1), np.arange(W).reshape(1, 1, 1, W)
    g = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 8.0) * (1.0 - jitter * rng.random((B, K, 1, 1)))
    return (g + 0.02 * rng.standard_normal((B, K, H, W))).astype(np.float32)


def test_workload_row_length(gpu):
    """B = 64 + 64, K = 3, 64 x 64 heat-maps (Gaussian blobs with noise): mmd_ref evaluates the distances in chunks of HW."""
    rng = np.random.default_rng(64)
    s, t = _blobs(rng, 64, 3, 64, 64, 0.1), _blobs(rng, 64, 3, 64, 64, 0.5)
    ref64 = mmd_ref.mmd(s, t, dtype=np.float64, chunk=128)
    ref32 = mmd_ref.mmd(s, t, dtype=np.float32, chunk=128)
    got = _kernels(gpu, s, t)
    _check('B64 K3 64x64', got, (ref32[0], ref32[2], ref32[3]), (ref64[0], ref64[2], ref64[3]))
    again = _kernels(gpu, s, t)
    assert again[0] == got[0] and _same(again[2], got[2]) and _same(again[3], got[3])


# ---------------------------------------------------------------- 4. bit-level properties
def test_two_runs_give_the_same_bits(gpu):
    s, t = _operands(4, 17, 21, (5, 7))
    a, b = _kernels(gpu, s, t), _kernels(gpu, s, t)
    assert a[0] == b[0] and _same(a[1], b[1]) and _same(a[2], b[2]) and _same(a[3], b[3])


def test_distances_are_symmetric_with_a_zero_diagonal(gpu):
    """The workspace after a launch with one kernel of fixed bandwidth bw = 64 and scale -B^2 K holds c_ij = s_ij exp(-D_ij / bw) / bw:
    the symmetry of D bit for bit shows as c == c^T, its zero diagonal as c_ii = 1 / bw exactly."""
    from mi355 import ops
    B, K = 17, 3
    s, t = _operands(9, B, K, (5, 7))
    _kernels(gpu, s, t, want=(False, False), kernel_num=1, fix_sigma=64.0, scale=-float(B * B * K))
    c = _kernels.work.cpu().numpy().reshape(K, 2 * B, 2 * B)           # (the cache was emptied for the call: its own buffer)
    assert _same(c, np.ascontiguousarray(c.transpose(0, 2, 1)))
    assert _same(np.diagonal(c, axis1=1, axis2=2), np.full((K, 2 * B), 1.0 / 64.0, np.float32))
    assert (c[:, :B, :B] > 0).all() and (c[:, B:, B:] > 0).all() and (c[:, :B, B:] < 0).all() and (c[:, B:, :B] < 0).all()


def test_target_equal_to_source_gives_zero(gpu):
    """With target = source the four distances of every quad are the same bits, so every loss_k is exactly what the symmetric D
    implies: 0.  The tolerance of test 1 around 0 is 4 times the float32 reference's own distance from 0, which is 0 as well
    (tests/test_mmd_cpu.py)."""
    s, _ = _operands(21, 5, 21, (8, 8))
    loss, rows, gs, gt = _kernels(gpu, s, s.copy())
    ref32 = mmd_ref.mmd(s, s, dtype=np.float32)
    print('target = source: loss %.3e, float32 reference %.3e' % (loss, float(ref32[0])))
    assert abs(loss) <= 4 * abs(float(ref32[0])) and not rows.any()
    assert np.isfinite(gs).all() and np.isfinite(gt).all()


def test_zero_bandwidth_joint(gpu):
    """A joint whose 2 B rows are identical, among live ones: exact zeros in its loss_k and gradient rows, the others unchanged
    bit for bit."""
    s, t = _operands(33, 3, 5, (8, 8))
    live = _kernels(gpu, s, t)
    s2, t2 = s.copy(), t.copy()
    s2[:, 2] = t2[:, 2] = s[0, 2]
    loss, rows, gs, gt = _kernels(gpu, s2, t2)
    assert np.isfinite(loss) and _same(rows[2], np.float32(0)) and _same(gs[:, 2], np.zeros_like(gs[:, 2])) and _same(gt[:, 2], np.zeros_like(gt[:, 2]))
    keep = [0, 1, 3, 4]
    assert _same(rows[keep], live[1][keep]) and _same(gs[:, keep], live[2][:, keep]) and _same(gt[:, keep], live[3][:, keep])
    ref64, ref32 = mmd_ref.mmd(s2, t2, dtype=np.float64), mmd_ref.mmd(s2, t2, dtype=np.float32)
    _check('zero-bandwidth joint', (loss, rows, gs, gt), (ref32[0], ref32[2], ref32[3]), (ref64[0], ref64[2], ref64[3]))
    # every joint dead: loss 0
    s3 = np.broadcast_to(s[:1, :, :1, :1], s.shape).copy()
    assert _kernels(gpu, s3, s3.copy())[0] == 0.0


# ---------------------------------------------------------------- 4b. the edges of the row count, inside guards
@pytest.mark.parametrize('B,K,shape', [(1, 1, (3, 5)), (128, 1, (3, 5)), (2, 21, (4, 4))], ids=['n2', 'n256', 'K21-HW16'])
def test_smallest_and_largest_row_counts(gpu, B, K, shape):
    """n = 2 and n = 256 = MMD_MAX_ROWS with one joint and 15 pixels (the scalar path), and K = 21 with one float4 chunk."""
    from mi355 import ops
    assert 2 * 128 == ops.MMD_MAX_ROWS
    s, t = _operands(1000 + B, B, K, shape)
    ref64 = mmd_ref.mmd(s, t, dtype=np.float64)
    ref32 = mmd_ref.mmd(s, t, dtype=np.float32)
    got = _kernels(gpu, s, t)
    _check('B%d K%d %s' % (B, K, shape), got, (ref32[0], ref32[2], ref32[3]), (ref64[0], ref64[2], ref64[3]))
    assert np.allclose(got[1], ref64[1], rtol=1e-5, atol=1e-6)


def test_workspace_one_byte_short_launches_nothing(gpu):
    """mi355_mmd_heatmap refuses a workspace one byte short (MI355_EINVAL, the message names the workspace) ahead of its launches."""
    import mi355
    from mi355 import ops
    B, K, HW = 3, 2, 16
    s, t = _operands(5, B, K, (4, 4))
    sd, td = _dev(gpu, s, 0, 'source'), _dev(gpu, t, 0, 'target')
    need = int(mi355.load().mi355_mmd_workspace(B, K))
    with G.window(ops, 'mmd workspace'):
        work = torch.empty(need // 4, dtype=torch.float32, device=gpu)
    rows, gs, gt = (G.empty(sh, torch.float32, gpu, n) for sh, n in (((K,), 'rows'), (s.shape, 'grad_source'), (t.shape, 'grad_target')))
    ops.prof_reset(); ops.prof_enable(2)
    try:
        rc = mi355.load().mi355_mmd_heatmap(sd.data_ptr(), td.data_ptr(), work.data_ptr(), need - 1, rows.data_ptr(), gs.data_ptr(),
                                            gt.data_ptr(), B, K, HW, 2.0, 5, 0.0, 1.0, mi355.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1 and b'workspace' in mi355.load().mi355_last_error()
        assert ops.prof_launches() == []
    finally:
        ops.prof_enable(0); ops.prof_reset()
    G.check('mmd workspace one byte short')
    assert all(G.unwritten(x) == x.numel() * 4 for x in (work, rows, gs, gt))


# ---------------------------------------------------------------- 5. refused arguments
def test_refused_arguments_launch_nothing(gpu):
    import mi355
    from mi355 import ops
    from uda.model.loss import MMD_loss3
    z = lambda *shape: torch.zeros(shape, device=gpu)
    s, t = z(2, 21, 8, 8), z(2, 21, 8, 8)
    ops.mmd_heatmap(s, t, True, True)                               # (the workspace of this shape exists from here on)
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    try:
        bad = [
            lambda: ops.mmd_heatmap(s, z(3, 21, 8, 8), False, False),              # unequal batch sizes
            lambda: ops.mmd_heatmap(s, z(2, 21, 8, 4), False, False),
            lambda: ops.mmd_heatmap(z(129, 1, 4), z(129, 1, 4), False, False),     # n = 258 rows
            lambda: ops.mmd_heatmap(z(0, 21, 4), z(0, 21, 4), False, False),
            lambda: ops.mmd_heatmap(z(2, 21, 0), z(2, 21, 0), False, False),       # HW = 0
            lambda: ops.mmd_heatmap(s, t, False, False, kernel_num=0),
            lambda: ops.mmd_heatmap(s, t, False, False, kernel_num=9),
            lambda: ops.mmd_heatmap(s, t, False, False, kernel_mul=0.0),
            lambda: ops.mmd_heatmap(s, t, False, False, kernel_mul=-2.0),
            lambda: ops.mmd_heatmap(s, t, False, False, rows=z(20)),               # buffers one element short
            lambda: ops.mmd_heatmap(s, t, True, False, grad_source=z(2 * 21 * 64 - 1)),
            lambda: ops.mmd_heatmap(s, t, False, True, grad_target=z(2 * 21 * 64 - 1)),
            lambda: ops.mmd_heatmap(s.half(), t.half(), False, False),
            lambda: ops.mmd_heatmap(s.transpose(2, 3), t.transpose(2, 3), False, False),
            lambda: ops.mmd_heatmap(s.cpu(), t.cpu(), False, False),
        ]
        for i, fn in enumerate(bad):
            with pytest.raises(mi355.Mi355Error):
                fn()
                pytest.fail('case %d was accepted' % i)
        with pytest.raises(ValueError):
            MMD_loss3()(s, z(3, 21, 8, 8))
        with pytest.raises(ValueError):
            MMD_loss3()(z(2, 64), z(2, 64))
        torch.cuda.synchronize()
        assert ops.prof_launches() == []
        ops.mmd_heatmap(s, t, True, False)
        torch.cuda.synchronize()
        assert [e['label'].split()[0] for e in ops.prof_launches()] == ['mmd_dist', 'mmd_coef', 'mmd_grad']
    finally:
        ops.prof_enable(0); ops.prof_reset()


# ---------------------------------------------------------------- 6. the iteration
W_MMD = 0.5


def _host(module):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in module.state_dict().items()}


def _training(gpu, mode):
    """mode: 'on' (DAStep with the MMD term), 'off' (mmd=None passed explicitly), 'plain' (a DAStep built without the argument)."""
    import mi355
    from mi355.da_step import DAStep, MMDAlign, build_training
    from uda.model.regda_7 import PoseResNetx9
    from test_gpu_ema import _pose
    mi355.set_compute_dtype('bf16')
    model = _pose(gpu, PoseResNetx9, 731)
    step, opts, scheds = build_training(model, heatmap_size=32)
    if mode != 'plain':
        step = DAStep(model, opts, step.crit, step.trade_off, step.skip, step.track_acc,
                      mmd=MMDAlign(weight=W_MMD) if mode == 'on' else None)
    assert getattr(step, 'mmd', None) is None or mode == 'on'
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    return model, step, scheds


def _run(gpu, mode, iters, capture_at=None):
    from utils.synthetic import make_batch
    from uda.model.loss import MMD_loss3
    model, step, scheds = _training(gpu, mode)
    batch = make_batch(2, 128, 32, seed=3, device=gpu)
    rec = dict(model=[], loss_gt=[], loss_mmd=[], again=[], y=[])
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
            rec['loss_mmd'].append(float(out['loss_mmd']))
            rec['again'].append(float(MMD_loss3()(out['y_s'], out['y_t'], scale=W_MMD)))
            rec['y'].append((out['y_s'].cpu().numpy().copy(), out['y_t'].cpu().numpy().copy()))
        else:
            assert 'loss_mmd' not in out
    return rec, step, batch


@pytest.fixture(scope='module')
def runs(gpu):
    import mi355
    try:
        eager, _, _ = _run(gpu, 'on', 5)
        graph, step, _ = _run(gpu, 'on', 5, capture_at=3)
        assert step.graphs is not None and len(step.graphs) == 6
        off, _, _ = _run(gpu, 'off', 2)
        plain, _, _ = _run(gpu, 'plain', 2)
    finally:
        mi355.set_compute_dtype('bf16')
    return dict(eager=eager, graph=graph, off=off, plain=plain)


def test_step_eager_and_replay_agree_bit_for_bit(runs):
    a, b = runs['eager'], runs['graph']
    assert a['loss_mmd'] == b['loss_mmd'] and a['loss_gt'] == b['loss_gt'] and len(set(a['loss_mmd'])) == 5
    for it in range(5):                                             # iterations 3 and 4 of `graph` are replays
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)


def test_step_off_equals_a_step_built_without_the_argument(runs):
    a, b = runs['off'], runs['plain']
    assert a['loss_gt'] == b['loss_gt']
    for it in range(2):
        for k in a['model'][it]:
            assert _same(a['model'][it][k], b['model'][it][k]), (it, k)


def test_step_loss_mmd_is_the_recomputed_term(runs):
    for name in ('eager', 'graph'):
        r = runs[name]
        for got, again, (y_s, y_t) in zip(r['loss_mmd'], r['again'], r['y']):
            assert got == again and got > 0                         # the same kernels on the dumped y_s, y_t outside the step
            ref64 = mmd_ref.mmd(y_s, y_t, scale=W_MMD, dtype=np.float64)
            ref32 = mmd_ref.mmd(y_s, y_t, scale=W_MMD, dtype=np.float32)
            assert abs(got - float(ref64[0])) <= max(4 * abs(float(ref32[0]) - float(ref64[0])), 5e-7 * abs(float(ref64[0])))


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
    """Step C of an iteration with `mmd` on holds each of the three mmd_ launches exactly once, for the target side only; with
    `mmd` off an iteration holds none."""
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
        for kernel in ('mmd_dist', 'mmd_coef', 'mmd_grad'):
            assert sum(l.startswith(kernel) for l in on['C']) == 1, kernel
        assert sum(l.startswith('mmd_') for l in on['C']) == 3
        assert [l for l in on['C'] if l.startswith('mmd_grad')][0].split()[4] == 'rows2+2'        # the target rows only
        assert not any(l.startswith('mmd_') for l in on['before'] + on['after'])
        assert not any(l.startswith('mmd_') for l in off['before'] + off['C'] + off['after'])
        assert len(on['C']) >= len(off['C']) + 3 and len(on['before']) == len(off['before'])
    finally:
        mi355.set_compute_dtype('bf16')
