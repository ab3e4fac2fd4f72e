"""mi355_render_hands (csrc/render.hip) on the GPU: out, out_ema and ids bit for bit against the numpy restatement of
tests/render_ref.py, inside the poisoned guard buffers of tests/guarded.py -- every output element written, no flank byte changed,
the records unchanged -- for both domains and the degenerate records, with each nullable output absent in turn, twice, and under
graph replay; and the refusals of the Python wrapper, which come before any launch."""
import functools

import numpy as np
import pytest
import torch

import guarded
import render_ref as R

pytestmark = pytest.mark.gpu

SIDES = (16, 32, 48, 64)          # 48: tile edges that are no power of two; 64: more than one 32-wide tile in each direction
CHUNKS = ((0, 1, 2), (3, 4, 5), (4, 5, 6))        # the seven records of render_ref.case_records as launches of B = 3


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


@functools.lru_cache(maxsize=None)
def _case(S):
    """(records, (out, out_ema, ids)) at side S: computed once, shared, never changed."""
    from mi355.ops import HAND_REC_DTYPE
    from utils.rendered_dataset import RenderedHand21
    recs = R.case_records(S, HAND_REC_DTYPE, RenderedHand21)
    want = R.render(recs, S, *R.norm())
    for a in (recs,) + want:
        a.setflags(write=False)
    return recs, want


def _launch(gpu, recs, S, ema=True, ids=True):
    from mi355 import ops
    B = len(recs)
    r_d = guarded.place(torch.from_numpy(recs.view(np.uint8).reshape(B, -1).copy()).to(gpu), 'recs')
    out = guarded.empty((B, 3, S, S), torch.float32, gpu, 'out')
    o_e = guarded.empty((B, 3, S, S), torch.float32, gpu, 'out_ema') if ema else None
    o_i = guarded.empty((B, S, S), torch.uint8, gpu, 'ids') if ids else None
    got = ops.render_hands(r_d, S, out=out, out_ema=o_e, ids=o_i)
    torch.cuda.synchronize()
    guarded.check('render_hands B=%d S=%d' % (B, S))
    assert got.data_ptr() == out.data_ptr()
    assert _same(r_d, recs.view(np.uint8).reshape(B, -1))            # the records are only read
    for t in (out, o_e, o_i):
        assert t is None or guarded.unwritten(t) == 0
    return out, o_e, o_i


def test_record_size_matches_the_dtype():
    import mi355
    from mi355.ops import HAND_REC_DTYPE
    assert mi355.load().mi355_hand_rec_size() == HAND_REC_DTYPE.itemsize == 480


@pytest.mark.parametrize('S', SIDES)
def test_render_bit_exact_inside_guard_buffers(gpu, S):
    recs, want = _case(S)
    try:
        for chunk in CHUNKS:
            sel = list(chunk)
            got = _launch(gpu, recs[sel], S)
            for name, g, w in zip(('out', 'out_ema', 'ids'), got, want):
                w = w[sel]
                if not _same(g, w):
                    g = g.cpu().numpy()
                    bad = np.argwhere(g.view(np.uint32 if g.dtype == np.float32 else np.uint8) != w.view(np.uint32 if w.dtype == np.float32 else np.uint8))
                    raise AssertionError('%s differs at S=%d records %s: %d elements, first %s got %r want %r' % (
                        name, S, sel, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))
    finally:
        guarded.reset()
    ids = want[2]
    assert not ids[5].any() and (ids[6] == 21).all()                 # the hand outside the frame; the occluder in front of everything
    assert np.isfinite(want[0]).all() and len(np.unique(ids[0])) > 10


@pytest.mark.parametrize('S', (16, 48))
def test_each_nullable_output_absent_in_turn_keeps_the_other_bits(gpu, S):
    recs, want = _case(S)
    sel = [1, 3, 4]
    try:
        for ema, ids in ((False, True), (True, False), (False, False)):
            out, o_e, o_i = _launch(gpu, recs[sel], S, ema=ema, ids=ids)
            assert _same(out, want[0][sel])
            assert o_e is None or _same(o_e, want[1][sel])
            assert o_i is None or _same(o_i, want[2][sel])
    finally:
        guarded.reset()


def test_two_runs_and_graph_replay_are_identical(gpu):
    from mi355 import ops
    S = 64
    recs, want = _case(S)
    sel = [1, 2, 4]
    try:
        first = _launch(gpu, recs[sel], S)
        second = _launch(gpu, recs[sel], S)
        assert all(_same(a, b) for a, b in zip(first, second))
        r_d = torch.from_numpy(recs[sel].view(np.uint8).reshape(3, -1).copy()).to(gpu)
        out, o_e = torch.zeros((3, 3, S, S), device=gpu), torch.zeros((3, 3, S, S), device=gpu)
        o_i = torch.zeros((3, S, S), dtype=torch.uint8, device=gpu)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.render_hands(r_d, S, out=out, out_ema=o_e, ids=o_i)       # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.render_hands(r_d, S, out=out, out_ema=o_e, ids=o_i)
        for t in (out, o_e, o_i):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(first, (out, o_e, o_i)))
        assert all(_same(a, w[sel]) for a, w in zip((out, o_e, o_i), want))
    finally:
        guarded.reset()


def test_wrapper_refuses_bad_arguments_before_any_launch(gpu):
    import mi355
    from mi355 import ops
    S = 32
    recs, _ = _case(S)
    B = 3
    try:
        r_d = guarded.place(torch.from_numpy(recs[:B].view(np.uint8).reshape(B, -1).copy()).to(gpu), 'recs')
        out = guarded.empty((B, 3, S, S), torch.float32, gpu, 'out')
        o_e = guarded.empty((B, 3, S, S), torch.float32, gpu, 'out_ema')
        o_i = guarded.empty((B, S, S), torch.uint8, gpu, 'ids')
        big = guarded.empty((2 * B * 3 * S * S + 8,), torch.float32, gpu, 'big')
        flat = big.view(torch.uint8)
        bad = [
            dict(image_size=24), dict(image_size=0), dict(image_size=528), dict(image_size=32.5),
            dict(recs=r_d.view(-1)[:-1]), dict(recs=r_d.view(-1)[:0]), dict(recs=r_d[:, ::2]), dict(recs=r_d.cpu()),
            dict(recs=flat[4:4 + B * 480]),                                                      # recs off a 16-byte boundary
            dict(out=out[:2]), dict(out=out.to(torch.float64)), dict(out=out.transpose(2, 3)), dict(out=out.cpu()),
            dict(out=big[1:1 + B * 3 * S * S].view(B, 3, S, S)),                                 # out 4 bytes off
            dict(out_ema=o_e[:, :2]), dict(out_ema=big[2:2 + B * 3 * S * S].view(B, 3, S, S)),
            dict(ids=o_i.to(torch.int32)), dict(ids=o_i[:, :, :16]), dict(ids=flat[1:1 + B * S * S].view(B, S, S)),
            dict(out_ema=out),                                                                   # the same buffer twice
            dict(out=big[:B * 3 * S * S].view(B, 3, S, S), out_ema=big[B * 3 * S * S - 4:2 * B * 3 * S * S - 4].view(B, 3, S, S)),
            dict(out=big[:B * 3 * S * S].view(B, 3, S, S), ids=flat[B * 3 * S * S * 4 - 4:B * 3 * S * S * 4 - 4 + B * S * S].view(B, S, S)),
            dict(recs=flat[:B * 480], out=big[:B * 3 * S * S].view(B, 3, S, S)),                 # out on top of the records
            dict(mean=(0.5, 0.5)), dict(std=(0.2, 0.0, 0.2)), dict(std=(0.2, float('nan'), 0.2)),
        ]
        for change in bad:
            args = dict(dict(recs=r_d, image_size=S, out=out, out_ema=o_e, ids=o_i), **change)
            with pytest.raises(mi355.Mi355Error):
                ops.render_hands(**args)
        torch.cuda.synchronize()
        guarded.check('render_hands refusals')
        for t in (out, o_e, o_i, big):
            assert guarded.unwritten(t) == t.numel() * t.element_size()                          # nothing was launched
    finally:
        guarded.reset()
