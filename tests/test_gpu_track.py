"""mi355_roi_crop_normalize and mi355_track_update (csrc/track.hip) on the GPU: bit for bit against the numpy restatement of
tests/track_ref.py, inside the poisoned guard buffers of tests/guarded.py -- every output element written, no flank byte changed,
the inputs unchanged -- eagerly and under graph replay.  The records cover every usable and unusable form the header names: an
unusable record must give exact zeros with the guards untouched (the frames are placed between poisoned flanks, so a read outside
them returns NaN bytes, not pixels).  Then the identity crop against mi355_resize_normalize, and the refusals of both wrappers,
which come before any launch."""
import functools

import numpy as np
import pytest
import torch

import guarded
import track_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
F, K = 2, 21
FRAMES = ((40, 56), (33, 57))                # (Hf, Wf); 33 x 57: a row pitch of 171 bytes
SIDES = (16, 32, 64)
LAUNCHES = (1, 3, 5)                         # records per launch, cycled over the list of box_records


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def _up(v):
    return np.nextafter(f32(v), f32(np.inf))


def box_records(S, Hf, Wf):
    """Every box the kernels must get right, as one list of records; `usable` of each is the header's rule."""
    rows = [
        dict(x0=3, y0=2, side=S),                                     # integer copy (crosses the lower / right edge where S is large)
        dict(x0=0, y0=0, side=S, frame=1),
        dict(x0=2.37, y0=1.61, side=0.83 * S),                        # fractional, n = 1
        dict(x0=1.5, y0=0.25, side=1.5 * S), dict(x0=-3.0, y0=1.0, side=2.5 * S, frame=1), dict(x0=-9.75, y0=-20.5, side=3.7 * S),    # n = 2, 3, 4
        dict(x0=1, y0=1, side=_up(S)), dict(x0=1, y0=1, side=2 * S), dict(x0=1, y0=1, side=_up(2 * S)),              # the thresholds of n
        dict(x0=1, y0=1, side=3 * S), dict(x0=1, y0=1, side=_up(3 * S)),
        dict(x0=-5.5, y0=4, side=S), dict(x0=6, y0=-7.25, side=S),    # across the left, upper,
        dict(x0=Wf - S / 2, y0=3.5, side=S), dict(x0=2.25, y0=Hf - S / 4, side=S, frame=1),                          # right and lower edge
        dict(x0=Wf + 10, y0=5, side=S), dict(x0=4, y0=-2 * S - 10, side=1.2 * S), dict(x0=-1.0 - S, y0=0, side=S),   # wholly outside
        dict(x0=Wf, y0=Hf, side=S), dict(x0=1048576.0, y0=-1048576.0, side=4 * S),                                   # the coordinate bound itself
        dict(x0=-0.5 * S, y0=-0.25 * S, side=4 * S), dict(x0=0, y0=0, side=_up(4 * S)),                              # side = 4 S, and just above
        dict(x0=5, y0=5, side=0.99), dict(x0=5.3, y0=5.6, side=1.0), dict(x0=5, y0=5, side=-4.0), dict(x0=5, y0=5, side=np.nan),
        dict(x0=3, y0=2, side=S, live=0), dict(x0=3, y0=2, side=S, frame=-1), dict(x0=3, y0=2, side=S, frame=F),
        dict(x0=3, y0=2, side=S, frame=0x7fffffff), dict(x0=3, y0=2, side=S, frame=-0x80000000),
        dict(x0=np.nan, y0=2, side=S), dict(x0=np.inf, y0=2, side=S), dict(x0=1e30, y0=2, side=S), dict(x0=3, y0=-np.inf, side=S),
        dict(x0=3, y0=-1e30, side=S), dict(x0=_up(1048576.0), y0=0, side=S),
        dict(x0=3, y0=2, side=S, mirror=1), dict(x0=2.37, y0=1.61, side=0.83 * S, mirror=1, frame=1),                # mirror
        dict(x0=-4.5, y0=3.25, side=2.2 * S, mirror=-1), dict(x0=7.5, y0=0.5, side=1.3 * S, live=-0x80000000, mirror=0x7fffffff),
    ]
    rec = R.records(len(rows), live=1)
    for i, row in enumerate(rows):
        for k, v in row.items():
            rec[k][i] = v
    return rec


@functools.lru_cache(maxsize=None)
def _case(S, Hf, Wf):
    """(frames, records, expected crops): computed once, shared, never changed."""
    rng = np.random.default_rng(1000 * S + Hf)
    frames = rng.integers(0, 256, (F, Hf, Wf, 3), dtype=np.uint8)
    frames[0, :2, :3] = (0, 255, 124)                            # the extremes of the table, and the byte nearest the mean
    recs = box_records(S, Hf, Wf)
    want = R.roi_crop_normalize(frames, recs, S)
    for a in (frames, recs, want):
        a.setflags(write=False)
    return frames, recs, want


def _rec_tensor(recs, gpu, name='recs'):
    return guarded.place(torch.from_numpy(recs.view(np.int32).reshape(-1, 8).copy()).to(gpu), name)


def _crop(gpu, frames, recs, S, start=guarded.START):
    from mi355 import ops
    N = len(recs)
    f_d = guarded.place(torch.from_numpy(frames.copy()).to(gpu), 'frames', start=start + 1)       # frames: no alignment at all
    r_d = _rec_tensor(recs, gpu)
    out = guarded.empty((N, 3, S, S), torch.float32, gpu, 'out', start=start)
    assert out.data_ptr() % 16 == start % 16
    got = ops.roi_crop_normalize(f_d, r_d, S, out=out)
    torch.cuda.synchronize()
    guarded.check('roi_crop_normalize N=%d S=%d' % (N, S))
    assert got.data_ptr() == out.data_ptr() and guarded.unwritten(out) == 0
    assert _same(f_d, frames) and _same(r_d, recs.view(np.int32).reshape(-1, 8))                # the inputs are only read
    return out


def _explain(name, got, want):
    g = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    bad = np.argwhere(g.view(np.uint32) != want.view(np.uint32))
    return '%s differs in %d elements, first %s got %r want %r' % (name, len(bad), bad[0].tolist(), g[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize('Hf,Wf', FRAMES)
@pytest.mark.parametrize('S', SIDES)
def test_crop_bit_exact_inside_guard_buffers(gpu, S, Hf, Wf):
    frames, recs, want = _case(S, Hf, Wf)
    usable = np.array([R.usable(r, S, F) for r in recs])
    assert usable.sum() >= 24 and (~usable).sum() >= 14
    assert not want[~usable].any() and all(w.any() for w in want[usable][:11])
    try:
        at, turn = 0, 0
        while at < len(recs):
            n = min(LAUNCHES[turn % 3], len(recs) - at)
            sel = slice(at, at + n)
            out = _crop(gpu, frames, recs[sel], S, start=guarded.START + 4 * (turn % 2))           # 16-byte aligned, and off by 4 bytes
            assert _same(out, want[sel]), _explain('S=%d records %d..%d' % (S, at, at + n - 1), out, want[sel])
            for i in np.flatnonzero(~usable[sel]):
                assert _bits(out[i])[2] == bytes(3 * S * S * 4)                                    # +0.0 everywhere: no sign bit either
            at, turn = at + n, turn + 1
    finally:
        guarded.reset()


def test_identity_crop_equals_resize_normalize(gpu):
    from mi355 import augment, ops
    S, (Hf, Wf) = 32, FRAMES[1]
    frames, _, _ = _case(S, Hf, Wf)
    boxes = [(0, 0, 0), (1, 25, 1), (0, 7, 0), (1, 13, 1)]                    # (frame, x0, y0): squares inside the 33 x 57 frame
    recs = R.records(len(boxes), live=1, side=S)
    squares = []
    for i, (f, x0, y0) in enumerate(boxes):
        recs['frame'][i], recs['x0'][i], recs['y0'][i] = f, x0, y0
        squares.append(np.ascontiguousarray(frames[f, y0:y0 + S, x0:x0 + S]))
    try:
        out = _crop(gpu, frames, recs, S)
        packed = torch.from_numpy(np.concatenate([s.reshape(-1) for s in squares])).to(gpu)
        table = np.array([[i * S * S * 3, S, S] for i in range(len(boxes))], dtype=np.int64)
        params = np.tile(np.array([0.0, 0, 0, S, 0.0, 0.0, 0.0, -1, -1, -1, 0.0]), (len(boxes), 1))
        ref = augment.resize_normalize(packed, table, params, size=S)
        torch.cuda.synchronize()
        assert _same(out, ref)
        recs['mirror'] = 1
        flipped = _crop(gpu, frames, recs, S)
        assert _same(flipped, torch.flip(ref, dims=(3,)))
    finally:
        guarded.reset()


# ---------------------------------------------------------------- track_update
def update_case(S, Hf, Wf, seed=0):
    """Records, key points and confidences that reach every branch of the box rule, with the parameters they are run under."""
    rng = np.random.default_rng(seed)
    P = dict(tau=0.1, min_joints=8, scale=1.5, alpha=0.75, grow=1.5, max_lost=3, min_side=8.0)
    rows, xy, conf = [], [], []

    def add(rec, pts=None, c=None):
        rows.append(rec)
        xy.append(rng.uniform(0.2 * S, 0.8 * S, (K, 2)).astype(f32) if pts is None else np.asarray(pts, dtype=f32))
        conf.append(rng.uniform(0.2, 0.9, K).astype(f32) if c is None else np.asarray(c, dtype=f32))

    few = lambda m: np.where(np.arange(K) < m, 0.5, 0.05)        # m joints at or above tau
    add(dict(x0=10.25, y0=4.5, side=1.1 * S))                                        # seen, in the middle
    add(dict(x0=10.25, y0=4.5, side=1.1 * S, mirror=1, frame=1))
    add(dict(x0=2, y0=3, side=S), c=few(8))                                          # m at min_joints
    add(dict(x0=2, y0=3, side=S, lost=2), c=few(8))
    add(dict(x0=2, y0=3, side=S), c=few(7))                                          # m just below: lost 0 -> 1, the box grows
    add(dict(x0=2, y0=3, side=S, lost=2), c=few(7))                                  # lost reaches max_lost: still alive
    add(dict(x0=2, y0=3, side=S, lost=3), c=few(7))                                  # beyond: dead, the box kept
    add(dict(x0=2, y0=3, side=S, lost=-5), c=few(0))
    add(dict(x0=2, y0=3, side=S, lost=0x7fffffff), c=few(0))
    add(dict(x0=2, y0=3, side=S), c=np.where(np.arange(K) == 7, 0.1, few(7)))        # conf == tau counts
    nan_c = rng.uniform(0.2, 0.9, K).astype(f32); nan_c[[0, 5, 20]] = np.nan
    add(dict(x0=6, y0=1, side=S), c=nan_c)                                           # NaN conf: not visible, not in the score
    add(dict(x0=6, y0=1, side=S), c=np.full(K, np.nan))
    nan_p = rng.uniform(0.2 * S, 0.8 * S, (K, 2)).astype(f32); nan_p[1, 0] = np.nan; nan_p[2, 1] = np.inf; nan_p[3] = (-np.inf, np.nan)
    add(dict(x0=6, y0=1, side=S, mirror=1), pts=nan_p)                               # NaN / inf xy: kp 0, not visible
    add(dict(x0=6, y0=1, side=S), pts=np.full((K, 2), np.nan))
    add(dict(x0=6, y0=1, side=S), pts=np.full((K, 2), 3.0e38))                       # overflows to inf in the map-back
    for dx, dy in ((-0.9 * S, 0), (0, -0.9 * S), (Wf, 0), (0, Hf), (-2.0 * S, -2.0 * S), (Wf + S, Hf + S)):
        add(dict(x0=4 + dx, y0=2 + dy, side=S))                                      # the new box clamps at every frame edge
    add(dict(x0=Wf - S / 2, y0=Hf - S / 2, side=S), c=few(3))                        # the grown box clamps as well
    add(dict(x0=-S / 2, y0=-S / 2, side=S), c=few(3))
    add(dict(x0=1, y0=1, side=4 * S), c=few(2))                                      # grow stops at the cap
    add(dict(x0=1, y0=1, side=1.0), pts=np.full((K, 2), 0.5 * S))                    # a point set: side rises to min_side
    add(dict(x0=1, y0=1, side=4 * S), pts=rng.uniform(0, S, (K, 2)))                 # a hand as large as the frame: side falls to the cap
    for bad in (dict(live=0), dict(side=0.5), dict(side=_up(4 * S)), dict(side=np.nan), dict(x0=np.nan), dict(y0=np.inf), dict(x0=-1e30),
                dict(live=0, lost=9, mirror=3, reserved=77)):
        add(dict(dict(x0=3, y0=2, side=S), **bad))                                   # unusable: zeros, live = 0, the rest kept
    add(dict(x0=3, y0=2, side=S, frame=-7, reserved=5, live=-2))                     # frame is not tested here; reserved -> 0
    rec = R.records(len(rows), live=1)
    for i, row in enumerate(rows):
        for k, v in row.items():
            rec[k][i] = v
    return rec, np.stack(xy), np.stack(conf), P


@functools.lru_cache(maxsize=None)
def _ucase(S, Hf, Wf):
    rec, xy, conf, P = update_case(S, Hf, Wf)
    want = R.track_update(rec, xy, conf, Hf, Wf, S, **P)
    for a in (rec, xy, conf) + want:
        a.setflags(write=False)
    return rec, xy, conf, P, want


def _update(gpu, rec, xy, conf, P, S, Hf, Wf, in_place):
    from mi355 import ops
    N = len(rec)
    r_d = _rec_tensor(rec, gpu, 'rec_in')
    xy_d, c_d = guarded.place(torch.from_numpy(xy.copy()).to(gpu), 'xy'), guarded.place(torch.from_numpy(conf.copy()).to(gpu), 'conf')
    out = (guarded.empty((N, K, 2), torch.float32, gpu, 'kp'), guarded.empty((N, K), torch.float32, gpu, 'vis'),
           guarded.empty((N,), torch.float32, gpu, 'score'))
    r_o = r_d if in_place else guarded.empty((N, 8), torch.int32, gpu, 'rec_out')
    kp, vis, score, r_got = ops.track_update(r_d, xy_d, c_d, ops.track_params((Hf, Wf), S, **P), out=out, rec_out=None if in_place else r_o)
    torch.cuda.synchronize()
    guarded.check('track_update N=%d' % N)
    assert r_got.data_ptr() == r_o.data_ptr() and all(guarded.unwritten(t) == 0 for t in out)
    assert _same(xy_d, xy) and _same(c_d, conf) and (in_place or _same(r_d, rec.view(np.int32).reshape(-1, 8)))
    return kp, vis, score, r_o


@pytest.mark.parametrize('in_place', (True, False))
@pytest.mark.parametrize('S,Hf,Wf', ((32, 40, 56), (16, 33, 57), (64, 33, 57)))
def test_update_bit_exact_inside_guard_buffers(gpu, S, Hf, Wf, in_place):
    rec, xy, conf, P, want = _ucase(S, Hf, Wf)
    w_kp, w_vis, w_score, w_rec = want
    live = w_rec['live']
    assert (live == 0).sum() >= 10 and (w_rec['lost'][live != 0] > 0).sum() >= 4 and w_vis.min() == 0 and w_vis.max() == 1
    try:
        at, turn = 0, 0
        while at < len(rec):
            n = min(LAUNCHES[turn % 3], len(rec) - at)
            sel = slice(at, at + n)
            kp, vis, score, r_o = _update(gpu, rec[sel], xy[sel], conf[sel], P, S, Hf, Wf, in_place)
            for name, g, w in (('kp', kp, w_kp[sel]), ('vis', vis, w_vis[sel]), ('score', score, w_score[sel])):
                assert _same(g, w), _explain('%s of records %d..%d' % (name, at, at + n - 1), g, w)
            got = r_o.cpu().numpy().view(R.REC).reshape(-1)
            assert got.tobytes() == w_rec[sel].tobytes(), 'records %d..%d: got %r want %r' % (at, at + n - 1, got, w_rec[sel])
            at, turn = at + n, turn + 1
    finally:
        guarded.reset()


def test_two_runs_and_graph_replay_are_identical(gpu):
    from mi355 import ops
    S, (Hf, Wf) = 32, FRAMES[1]
    frames, recs, want = _case(S, Hf, Wf)
    rec, xy, conf, P, (w_kp, w_vis, w_score, w_rec) = _ucase(S, Hf, Wf)
    sel = [2, 5, 12, 21, 37]
    try:
        first = _crop(gpu, frames, recs[sel], S)
        second = _crop(gpu, frames, recs[sel], S, start=guarded.START + 4)
        assert _same(first, second) and _same(first, want[sel])
        f_d = guarded.place(torch.from_numpy(frames.copy()).to(gpu), 'frames', start=guarded.START + 1)
        r_c = _rec_tensor(recs[sel], gpu)
        n = len(rec)
        r_u0 = torch.from_numpy(rec.view(np.int32).reshape(-1, 8).copy()).to(gpu)
        r_u = guarded.place(r_u0, 'rec_in')
        xy_d, c_d = guarded.place(torch.from_numpy(xy.copy()).to(gpu), 'xy'), guarded.place(torch.from_numpy(conf.copy()).to(gpu), 'conf')
        out = guarded.empty((len(sel), 3, S, S), torch.float32, gpu, 'out')
        outs = (guarded.empty((n, K, 2), torch.float32, gpu, 'kp'), guarded.empty((n, K), torch.float32, gpu, 'vis'),
                guarded.empty((n,), torch.float32, gpu, 'score'))
        params = ops.track_params((Hf, Wf), S, **P)

        def chain():
            ops.roi_crop_normalize(f_d, r_c, S, out=out)
            ops.track_update(r_u, xy_d, c_d, params, out=outs)                   # in place
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            chain()                                                              # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        for t in (out,) + outs:
            t.view(torch.uint8).fill_(guarded.FILL)                              # unwritten again: the replay must write every element
        r_u.copy_(r_u0)
        graph.replay()
        torch.cuda.synchronize()
        guarded.check('replay of roi_crop_normalize + track_update')
        assert all(guarded.unwritten(t) == 0 for t in (out,) + outs)
        assert _same(out, want[sel])
        assert _same(outs[0], w_kp) and _same(outs[1], w_vis) and _same(outs[2], w_score)
        assert r_u.cpu().numpy().view(R.REC).reshape(-1).tobytes() == w_rec.tobytes()
    finally:
        guarded.reset()


def test_record_helpers_round_trip(gpu):
    from mi355 import ops
    assert ops.TRACK_REC_DTYPE == R.REC
    recs = box_records(32, 40, 56)
    t = ops.pack_track_records(recs, gpu)
    assert t.dtype == torch.int32 and tuple(t.shape) == (len(recs), 8)
    assert ops.unpack_track_records(t).tobytes() == recs.tobytes()
    ops.pack_track_records(recs[::-1], out=t)
    assert ops.unpack_track_records(t).tobytes() == recs[::-1].tobytes()


def test_wrappers_refuse_bad_arguments_before_any_launch(gpu):
    import mi355
    from mi355 import ops
    S, (Hf, Wf), N = 32, FRAMES[0], 3
    frames, recs, _ = _case(S, Hf, Wf)
    rec, xy, conf, P, _ = _ucase(S, Hf, Wf)
    try:
        f_d = guarded.place(torch.from_numpy(frames.copy()).to(gpu), 'frames')
        r_d = _rec_tensor(recs[:N], gpu)
        out = guarded.empty((N, 3, S, S), torch.float32, gpu, 'out')
        big = guarded.empty((N * 3 * S * S + 64,), torch.float32, gpu, 'big')
        crop_ok = dict(frames=f_d, recs=r_d, S=S, out=out)
        bad_crop = [
            (dict(S=24), 'S=24'), (dict(S=0), 'S=0'), (dict(S=528), 'S=528'), (dict(S=32.5), 'S=32.5'),
            (dict(frames=f_d.to(torch.float32)), 'frames must be'), (dict(frames=f_d[:, :, :, :2]), 'frames must be'), (dict(frames=f_d[:, ::2]), 'frames must be'),
            (dict(frames=f_d.cpu()), 'no CPU fallback'), (dict(frames=f_d[:0]), 'frames must be'),
            (dict(recs=r_d.view(-1)), 'recs must be'), (dict(recs=r_d[:, :7]), 'recs must be'), (dict(recs=r_d.to(torch.int64)), 'recs must be'),
            (dict(recs=r_d[:0]), 'recs must be'), (dict(recs=r_d.cpu()), 'no CPU fallback'),
            (dict(out=out[:2]), 'out must be'), (dict(out=out.to(torch.float64)), 'out must be'), (dict(out=out.transpose(2, 3)), 'out must be'),
            (dict(std=(0.2, 0.0, 0.2)), 'norm std[1]'), (dict(std=(0.2, 0.2, float('nan'))), 'norm std[2]'), (dict(mean=(float('inf'), 0, 0)), 'norm mean[0]'),
            (dict(recs=big.view(torch.int32)[8:8 + 8 * N].view(N, 8), out=big[:N * 3 * S * S].view(N, 3, S, S)), 'out and recs overlap'),
            (dict(frames=big.view(torch.uint8)[64:64 + frames.size].view(F, Hf, Wf, 3), out=big[:N * 3 * S * S].view(N, 3, S, S)), 'out and frames overlap'),
        ]
        for change, msg in bad_crop:
            with pytest.raises(mi355.Mi355Error) as e:
                ops.roi_crop_normalize(**dict(crop_ok, **change))
            assert msg in str(e.value), (change.keys(), str(e.value))
        u_r = _rec_tensor(rec[:N], gpu, 'rec_in')
        xy_d, c_d = guarded.place(torch.from_numpy(xy[:N].copy()).to(gpu), 'xy'), guarded.place(torch.from_numpy(conf[:N].copy()).to(gpu), 'conf')
        outs = (guarded.empty((N, K, 2), torch.float32, gpu, 'kp'), guarded.empty((N, K), torch.float32, gpu, 'vis'),
                guarded.empty((N,), torch.float32, gpu, 'score'))
        r_o = guarded.empty((N, 8), torch.int32, gpu, 'rec_out')
        upd_ok = dict(recs=u_r, xy=xy_d, conf=c_d, out=outs, rec_out=r_o)
        par = lambda **kw: ops.track_params((Hf, Wf), S, **dict(P, **kw))
        bad_upd = [
            (dict(xy=xy_d[:2]), None, 'xy must be'), (dict(xy=xy_d[:, :, :1]), None, 'xy must be'), (dict(xy=xy_d.to(torch.float64)), None, 'xy must be'),
            (dict(conf=c_d[:, :20]), None, 'conf'), (dict(conf=c_d.cpu()), None, 'no CPU fallback'),
            (dict(recs=u_r[:2]), None, 'xy must be (2, K, 2)'), (dict(rec_out=r_o[:2]), None, 'rec_out holds'), (dict(rec_out=r_o.view(-1)), None, 'rec_out must be'),
            (dict(out=outs[:2]), None, 'out must hold'), (dict(out=(outs[0], outs[1].view(-1), outs[2])), None, 'vis must be'),
            (dict(out=(outs[0], outs[0].view(-1)[:N * K].view(N, K), outs[2])), None, 'kp and vis overlap'),
            (dict(rec_out=big.view(torch.int32)[:8 * N].view(N, 8), out=(outs[0], outs[1], big[4:4 + N])), None, 'score and rec_out overlap'),
            (dict(rec_out=u_r.view(-1)[8:].view(N - 1, 8), recs=u_r[:N - 1], xy=xy_d[:N - 1], conf=c_d[:N - 1],
                  out=tuple(t[:N - 1] for t in outs)), None, 'rec_out and rec_in overlap'),
            ({}, par(tau=float('nan')), 'tau='), ({}, par(min_joints=0), 'min_joints=0'), ({}, par(min_joints=K + 1), 'min_joints=22'),
            ({}, par(scale=0.0), 'scale='), ({}, par(alpha=1.5), 'alpha='), ({}, par(alpha=float('nan')), 'alpha='), ({}, par(grow=0.9), 'grow='),
            ({}, par(max_lost=-1), 'max_lost=-1'), ({}, par(min_side=0.5), 'min_side='), ({}, ops.track_params((Hf, Wf), 24, **P), 'S=24'),
            ({}, ops.track_params((0, Wf), S, **P), 'Hf=0'), ({}, ops.track_params((Hf, 4097), S, **P), 'Wf=4097'),
        ]
        for change, params, msg in bad_upd:
            with pytest.raises(mi355.Mi355Error) as e:
                ops.track_update(params=params or par(), **dict(upd_ok, **change))
            assert msg in str(e.value), (change.keys(), str(e.value))
        with pytest.raises(mi355.Mi355Error):
            ops.track_params((Hf, Wf), S, speed=3)
        kbig = torch.zeros((N, 65, 2), device=gpu)
        with pytest.raises(mi355.Mi355Error) as e:
            ops.track_update(u_r, kbig, torch.zeros((N, 65), device=gpu), par())
        assert 'K=65' in str(e.value)
        torch.cuda.synchronize()
        guarded.check('track refusals')
        for t in (out, big, r_o) + outs:
            assert guarded.unwritten(t) == t.numel() * t.element_size()                          # nothing was launched
        assert _same(u_r, rec[:N].view(np.int32).reshape(-1, 8))
    finally:
        guarded.reset()
