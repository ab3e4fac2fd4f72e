"""mi355.infer.HandTracker on the GPU.  Closed loop on a moving target: an oracle head stands in for the network -- a module that
writes a peak at every known key point as seen through the tracker's CURRENT device records -- so the whole loop (crop, forward,
decode, confidence, map-back, next box) can be restated in numpy with tests/track_ref.py and compared bit for bit, eagerly and
under graph replay, through a hand that is hidden and found again and one that is lost for good.  Then a randomly initialised
ResNet-18: the key points inside step() are PosePredictor's on the same crops, replay equals eager, predict() moves nothing."""
import numpy as np
import pytest
import torch

import track_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
S, HM, HF, WF, T, N, K = 32, 8, 96, 128, 12, 2, 21
P = dict(tau=0.1, min_joints=8, scale=1.5, alpha=1.0, grow=1.25, max_lost=3, min_side=8.0)
PEAK = 8.0                                    # a visible map: p = 1 / (1 + 63 e^-8) = 0.98; a hidden one is flat: p = 1 / 64 < tau


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    return _bits(a) == _bits(b)


def scene():
    """Key points of two hands over T frames (T, N, K, 2), frame pixels, and which hand is hidden in which frame (T, N)."""
    rng = np.random.default_rng(11)
    shape = rng.uniform(-11, 11, (N, K, 2))
    start, vel = np.array([[30.0, 30.0], [95.0, 60.0]]), np.array([[3.1, 1.7], [-2.6, -1.2]])
    gt = start[None, :, None] + vel[None, :, None] * np.arange(T)[:, None, None, None] + shape[None]
    hidden = np.zeros((T, N), bool)
    hidden[3:6, 0] = True                     # max_lost frames: found again
    hidden[4:8, 1] = True                     # max_lost + 1 frames: lost for good
    return gt, hidden


def start_boxes(gt):
    return np.stack([np.concatenate([gt[0, n].min(0), gt[0, n].max(0)]) for n in range(N)])


def peak_pixels(rec, pts):
    """Heat-map pixel (hx, hy) of every key point `pts` (K, 2; frame pixels, float64) seen through one record: the crop
    coordinate (mirrored where the record says so) over the stride, rounded, clamped to the map.  float64 on both sides."""
    st = float(rec['side']) / S
    cx, cy = (pts[:, 0] - float(rec['x0'])) / st, (pts[:, 1] - float(rec['y0'])) / st
    if rec['mirror'] != 0:
        cx = (S - 1) - cx
    stride = S / HM
    return np.clip(np.rint(cx / stride), 0, HM - 1), np.clip(np.rint(cy / stride), 0, HM - 1)


class Oracle(torch.nn.Module):
    """(B, 3, S, S) -> (B, K, HM, HM): PEAK at peak_pixels of self.gt through tracker.recs, zeros elsewhere; a hidden hand's maps are
    flat.  Everything is a device operation on tensors at fixed addresses, so the module can be captured."""

    def __init__(self, gpu):
        super().__init__()
        self.gt = torch.zeros((N, K, 2), dtype=torch.float64, device=gpu)
        self.hidden = torch.zeros((N,), dtype=torch.float32, device=gpu)
        self.tracker = None

    def forward(self, x):
        r = self.tracker.recs
        geo = r[:, 1:4].view(torch.float32).double()
        st = geo[:, 2] / S
        cx = (self.gt[:, :, 0] - geo[:, 0:1]) / st[:, None]
        cy = (self.gt[:, :, 1] - geo[:, 1:2]) / st[:, None]
        cx = torch.where((r[:, 4] != 0)[:, None], (S - 1) - cx, cx)
        stride = S / HM
        hx = torch.nan_to_num(torch.round(cx / stride), 0.0, 0.0, 0.0).clamp(0, HM - 1).long()
        hy = torch.nan_to_num(torch.round(cy / stride), 0.0, 0.0, 0.0).clamp(0, HM - 1).long()
        y = torch.zeros((N, K, HM * HM), dtype=torch.float32, device=x.device)
        y.scatter_(2, (hy * HM + hx)[:, :, None], PEAK)
        return (y * (1.0 - self.hidden)[:, None, None]).view(N, K, HM, HM)


def closed_loop_reference(gt, hidden, rec):
    out = []
    for t in range(T):
        xy, conf = np.zeros((N, K, 2), f32), np.zeros((N, K), f32)
        for n in range(N):
            if hidden[t, n]:
                conf[n] = 1.0 / (HM * HM)                     # argmax of a flat map: xy = 0
                continue
            hx, hy = peak_pixels(rec[n], gt[t, n])
            xy[n, :, 0], xy[n, :, 1] = hx * (S / HM), hy * (S / HM)
            conf[n] = 0.98
        kp, vis, _, rec = R.track_update(rec, xy, conf, HF, WF, S, **P)
        out.append((kp, vis, rec))
    return out


def run_tracker(gpu, gt, hidden, graph):
    from mi355 import ops
    from mi355.infer import HandTracker
    oracle = Oracle(gpu)
    tracker = HandTracker(oracle, S, (HF, WF), N, decode='argmax', flip_test=False, graph=graph, warmup=2, **P)
    oracle.tracker = tracker
    tracker.reset(start_boxes(gt), mirror=[0, 1])
    frames = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (1, HF, WF, 3), dtype=np.uint8)).to(gpu)
    out = []
    for t in range(T):
        oracle.gt.copy_(torch.from_numpy(gt[t]))
        oracle.hidden.copy_(torch.from_numpy(hidden[t].astype(f32)))
        kp, vis, score, live, boxes = tracker.step(frames)
        rec = ops.unpack_track_records(tracker.recs)
        assert live.cpu().numpy().tolist() == (rec['live'] != 0).tolist()
        assert _same(boxes, np.stack([rec['x0'], rec['y0'], rec['x0'] + rec['side'], rec['y0'] + rec['side']], 1))
        out.append((kp.cpu().numpy(), vis.cpu().numpy(), rec, score.cpu().numpy()))
    return tracker, out


def test_closed_loop_equals_the_numpy_restatement_eagerly_and_replayed(gpu):
    from mi355 import ops
    from mi355.infer import HandTracker
    gt, hidden = scene()
    first = ops.unpack_track_records(ops.pack_track_records(HandTracker(None, S, (HF, WF), N, **P)._records(start_boxes(gt), [0, 1], None)))
    want = closed_loop_reference(gt, hidden, first.copy())
    # the scene does what the issue asks of it: hand 0 is found again, hand 1 is lost for good
    assert [int(w[2]['live'][0]) for w in want] == [1] * T and [int(w[2]['lost'][0]) for w in want][2:7] == [0, 1, 2, 3, 0]
    assert want[6][1][0].all() and want[T - 1][1][0].all()
    assert [int(w[2]['live'][1]) for w in want] == [1] * 7 + [0] * 5
    assert all(not w[0][1].any() and not w[1][1].any() for w in want[8:])
    err = np.abs(want[T - 1][0][0] - gt[T - 1, 0]).max()
    assert err < 8.0, err                                                     # the box still holds the hand: within two heat-map pixels (4 crop pixels each)
    eager_tracker, eager = run_tracker(gpu, gt, hidden, graph=False)
    graph_tracker, replay = run_tracker(gpu, gt, hidden, graph=True)
    assert not eager_tracker._graphs and len(graph_tracker._graphs) == 1
    for t in range(T):
        for name, i in (('kp', 0), ('vis', 1)):
            assert _same(eager[t][i], want[t][i]), '%s differs from the restatement at frame %d:\n%r\n%r' % (name, t, eager[t][i], want[t][i])
            assert _same(replay[t][i], eager[t][i]), '%s: replay differs from eager at frame %d' % (name, t)
        assert eager[t][2].tobytes() == want[t][2].tobytes(), 'records differ at frame %d: %r vs %r' % (t, eager[t][2], want[t][2])
        assert replay[t][2].tobytes() == eager[t][2].tobytes() and _same(replay[t][3], eager[t][3])
        assert abs(float(eager[t][3][0]) - (0.0 if hidden[t, 0] else 1.0 / (1.0 + 63.0 * np.exp(-PEAK)))) < 1e-6       # the confidence


@pytest.fixture(scope='module')
def resnet18(gpu):
    import mi355
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling, PoseResNet
    mi355.load()
    torch.manual_seed(3)
    bb = models.resnet18(pretrained=False)
    return PoseResNet(bb, Upsampling(bb.out_features), 256, 21, finetune=True).to(gpu).eval()


def test_resnet18_step_is_pose_predictor_on_the_crops(gpu, resnet18):
    from mi355 import ops
    from mi355.infer import HandTracker, PosePredictor
    S2, Hf, Wf = 64, 120, 160
    rng = np.random.default_rng(4)
    frames = [torch.from_numpy(rng.integers(0, 256, (1, Hf, Wf, 3), dtype=np.uint8)).to(gpu) for _ in range(3)]
    boxes = np.array([[20, 30, 70, 90], [90, 10, 150, 60]], dtype=np.float64)
    predictor = PosePredictor(resnet18, S2)
    results = {}
    for graph in (False, True):
        tracker = HandTracker(resnet18, S2, (Hf, Wf), 2, graph=graph, warmup=2).reset(boxes, mirror=[0, 1])
        rows = []
        for f in frames:
            before = tracker.recs.clone()
            out = tracker.step(f)
            crops = ops.roi_crop_normalize(f, before, S2)
            xy, _ = predictor(crops)
            assert _same(tracker.crop_xy, xy)
            rows.append(tuple(t.clone() for t in out) + (tracker.recs.clone(),))
        results[graph] = rows
        assert bool(tracker._graphs) == graph
        kept = tracker.recs.clone()
        kp, vis, score, live, bx = tracker.predict(frames[0], boxes, mirror=[0, 1])
        again = [tracker.predict(frames[0], boxes, mirror=[0, 1])[0] for _ in range(2)]         # the third call is replayed
        assert _same(tracker.recs, kept) and all(_same(kp, k) for k in again)
        assert len(tracker._graphs) == (2 if graph else 0)
        assert _same(kp, results[graph][0][0]) and live.all() and tuple(bx.shape) == (2, 4)      # the first step saw the same boxes
    for a, b in zip(results[False], results[True]):
        assert all(_same(u, v) for u, v in zip(a, b))
