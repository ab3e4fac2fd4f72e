"""The in-launch exchange of the one-launch BatchNorm backward (csrc/bn.hip, bn_bwd_resident_kernel): data-tagged granules
in a buffer of the library's own, the tag derived from a per-(kind, grid size) completion count on the device.

What can go wrong with such a tag is reuse: launches of different grid sizes share the granule slots, a replayed graph cannot
be handed a fresh tag from the host, and a reset must not leave a slot that a later launch would take for its own.  These
tests run many launches of many grids back to back -- eagerly, from a replayed graph, and across a reset -- and ask for
the same bits every time and for no give-up.  None of them provokes a give-up."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, C, H, W, dtype): C = 64 G channels in bf16 (32 G in fp32) -> G = 1, 2, 4, 8, 16, 32 channel groups; row counts that do not
# divide by the 256 / G row blocks (ragged last tile), one that gives fewer blocks than CUs, and both granule kinds
GEOMS = [
    (3, 64, 37, 41, torch.bfloat16),        # G = 1, 4551 rows
    (2, 128, 33, 29, torch.bfloat16),       # G = 2
    (5, 256, 17, 19, torch.bfloat16),       # G = 4
    (16, 256, 32, 32, torch.bfloat16),      # G = 4, whole tiles (the benchmark's 16384 x 256)
    (3, 512, 13, 11, torch.bfloat16),       # G = 8
    (2, 1024, 9, 7, torch.bfloat16),        # G = 16
    (1, 2048, 5, 5, torch.bfloat16),        # G = 32, 25 rows over 8 row blocks
    (1, 2048, 1, 3, torch.bfloat16),        # G = 32, 3 rows: 96 blocks
    (2, 64, 21, 23, torch.float32),         # fp32: G = 2, 64 granules per block
    (3, 256, 11, 13, torch.float32),        # fp32: G = 8
]


def _ops():
    import mi355
    from mi355 import ops
    mi355.load()
    return ops


def _inputs(gpu, seed, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    out = []
    for N, C, H, W, dt in GEOMS:
        nhwc = lambda t: t.to(gpu).to(dt).contiguous(memory_format=torch.channels_last)
        x = nhwc(torch.randn(N, C, H, W, generator=g))
        dy = nhwc(scale * torch.randn(N, C, H, W, generator=g))
        gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(gpu)
        beta = (0.1 * torch.randn(C, generator=g)).to(gpu)
        mean = (0.1 * torch.randn(C, generator=g)).to(gpu)
        invstd = (1 + 0.1 * torch.rand(C, generator=g)).to(gpu)
        out.append(dict(x=x, dy=dy, gamma=gamma, beta=beta, mean=mean, invstd=invstd))
    return out


def _bwd(ops, a):
    """One backward in the form the one-launch kernel takes (ReLU mask recomputed from x): (dx, dres, dgamma, dbeta)."""
    C = a['x'].shape[1]
    dg, db = torch.zeros(C, device=a['x'].device), torch.zeros(C, device=a['x'].device)
    dx, dres = ops.bn_bwd(a['dy'], a['x'], None, a['gamma'], a['mean'], a['invstd'], dg, db, False, True, True, beta=a['beta'])
    return dx, dres, dg, db


def _sequence(ops, args, rounds):
    """`rounds` passes over all geometries, the grids interleaved; asserts every result equal to that geometry's first."""
    first = [None] * len(args)
    for rnd in range(rounds):
        order = range(len(args)) if rnd % 2 == 0 else reversed(range(len(args)))
        for i in order:
            res = _bwd(ops, args[i])
            if first[i] is None:
                first[i] = res
                assert all(bool(torch.isfinite(t.float()).all()) for t in res), 'geometry %d' % i
            else:
                for a, b in zip(res, first[i]):
                    assert torch.equal(a, b), 'geometry %d differs from its first result in round %d' % (i, rnd)
    return first


@pytest.fixture()
def resident(gpu):
    """The one-launch form switched on for the test (and the previous setting restored), counters clean before and after."""
    import mi355
    ops = _ops()
    assert ops.bn_resident_timeouts() == 0
    prev = mi355.load().mi355_bn_set_resident(1)
    yield ops
    mi355.load().mi355_bn_set_resident(prev)
    assert ops.bn_resident_timeouts() == 0


def test_interleaved_grids_repeat_their_bits(gpu, resident):
    ops = resident
    _sequence(ops, _inputs(gpu, 11), 50)
    assert ops.bn_resident_timeouts() == 0


def test_replayed_graph_equals_eager_on_changed_inputs(gpu, resident):
    ops = resident
    args = _inputs(gpu, 12)
    for a in args:                      # warm up outside the capture: workspace, first-launch attributes
        _bwd(ops, a)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = [_bwd(ops, a) for a in args]
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(24):
        fresh = _inputs(gpu, 100 + rep, scale=1.0 + 0.25 * rep)
        for a, f in zip(args, fresh):
            for k in a:
                a[k].copy_(f[k])
        graph.replay()
        torch.cuda.synchronize()
        replayed = [[t.clone() for t in res] for res in captured]
        for i, a in enumerate(args):
            eager = _bwd(ops, a)        # eager launches between the replays: the graph's tags must not depend on a host count
            for r, e in zip(replayed[i], eager):
                assert torch.equal(r, e), 'geometry %d, replay %d' % (i, rep)
    assert ops.bn_resident_timeouts() == 0


def test_reset_between_two_runs(gpu, resident):
    ops = resident
    args = _inputs(gpu, 13)
    one = _sequence(ops, args, 3)
    torch.cuda.synchronize()
    ops.bn_resident_reset()             # counts back to 0: the tags of the first run come round again
    two = _sequence(ops, args, 3)
    for i, (r1, r2) in enumerate(zip(one, two)):
        for a, b in zip(r1, r2):
            assert torch.equal(a, b), 'geometry %d differs after the reset' % i
    assert ops.bn_resident_timeouts() == 0
