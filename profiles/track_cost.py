"""Cost of the hand-tracking loop (DESIGN.md section 7 "Hand tracking"), on rendered frames (utils.rendered_dataset.hand_sequence):

  * mi355.infer.HandTracker.step per frame under graph replay and eagerly, at N = 1, 2, 8 hands, ResNet-50, 256 x 256 crops, and
    the frames per second of either; the split crop / forward / decode / confidence / update of one eager step between device events;
  * the same loop written with what the parent commit offers: PIL crop and resize on the host, ToTensor + Normalize, upload,
    mi355.infer.PosePredictor, read the key points back, next box on the host (uda.dataset.util.scale_box);
  * mi355_roi_crop_normalize at 64 hands, 256 x 256, beside mi355_resize_normalize on the pre-cropped squares and
    mi355_affine_warp_images on an output of the same size;
  * the mean and maximum absolute difference between the crop kernel and the Pillow chain (resize_normalize on the pre-cropped
    square) at side / S = 1, 1.5, 2 and 3: the two filters differ by design above 1; at 1 on an integer box they are equal.

Every figure is measured where it runs; nothing is asserted.  Prints one line per figure and, last, one JSON line with all.

    python profiles/track_cost.py [--arch resnet50] [--image-size 256] [--frame 512] [--frames 60] [--rounds 3] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd'))

import numpy as np
import torch

import mi355
from mi355 import augment, ops
from mi355.infer import HandTracker, PosePredictor
from utils.rendered_dataset import hand_sequence, render_sequence


def timed(fn, reps, warm=5):
    """Mean GPU time per call in ms: `reps` calls back to back between two events, after `warm` unmeasured ones."""
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def build_model(arch, device):
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    torch.manual_seed(0)
    bb = models.__dict__[arch](pretrained=False)
    return PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(device).eval()


def gt_boxes(gt, n):
    b = np.array([gt[0, :, 0].min(), gt[0, :, 1].min(), gt[0, :, 0].max(), gt[0, :, 1].max()])
    return np.tile(b, (n, 1))


def loop_wall(step, frames, rounds):
    """Median wall time per frame in ms of `step(frame)` over the sequence, the device drained at the end of every round."""
    per = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(len(frames)):
            step(frames[t:t + 1])
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3 / len(frames))
    return statistics.median(per), per


def stage_split(tracker, frame, reps=20):
    """ms per stage of one eager step, each between device events with the others' inputs held fixed."""
    from utils.keypoint_detection import decode_keypoints
    N, S = tracker.max_hands, tracker.image_size
    recs = tracker.recs.clone()
    x = ops.roi_crop_normalize(frame, recs, S)
    with torch.no_grad():
        y2 = tracker.model(ops.mirror_batch(x))
    y, yf = y2[:N], y2[N:]
    xy, _, avg = decode_keypoints(y, S, tracker.decode, with_maxval=True, y_flip=yf, flip_shift=1, sigma=2.0, return_avg=True)
    pk = ops.peak_prob(avg, 1.0)
    outs = (torch.empty_like(xy), torch.empty_like(pk[2]), torch.empty((N,), device=xy.device))
    scratch = recs.clone()
    with torch.no_grad():
        return {
            'crop': timed(lambda: ops.roi_crop_normalize(frame, recs, S, out=x), reps),
            'forward': timed(lambda: tracker.model(ops.mirror_batch(x)), reps),
            'decode': timed(lambda: decode_keypoints(y, S, tracker.decode, with_maxval=True, y_flip=yf, flip_shift=1, sigma=2.0, return_avg=True), reps),
            'confidence': timed(lambda: ops.peak_prob(avg, 1.0, out=pk), reps),
            'update': timed(lambda: ops.track_update(recs, xy, pk[2], tracker.params, out=outs, rec_out=scratch), reps),
        }


def host_loop(model, S, host_frames, box, n_hands, device):
    """The loop the parent commit allows: per frame and hand PIL crop + resize, ToTensor + Normalize on the host, one upload, PosePredictor,
    the key points read back, the next box from scale_box."""
    from PIL import Image
    from uda.dataset.util import get_bounding_box, scale_box
    predictor = PosePredictor(model, S)
    mean, std = np.array(augment.MEAN, np.float32)[:, None, None], np.array(augment.STD, np.float32)[:, None, None]
    Hf, Wf = host_frames.shape[1:3]
    images = [Image.fromarray(f) for f in host_frames]
    boxes = [scale_box(box, Wf, Hf, 1.5)] * n_hands

    def step(t):
        crops = []
        for l, u, r, d in boxes:
            im = images[t].crop((l, u, r + 1, d + 1)).resize((S, S), Image.BILINEAR)
            crops.append((np.asarray(im, np.float32).transpose(2, 0, 1) / 255.0 - mean) / std)
        xy, _ = predictor(torch.from_numpy(np.stack(crops)).to(device))
        xy = xy.cpu().numpy()
        for n, (l, u, r, d) in enumerate(boxes):
            kp = xy[n] * ((r - l + 1) / S) + (l, u)
            boxes[n] = scale_box(get_bounding_box(kp), Wf, Hf, 1.5) if np.isfinite(kp).all() and np.ptp(kp, axis=0).max() >= 8 else boxes[n]
    return step


def crop_kernels(device, frames, S=256, B=64, reps=50):
    Hf, Wf = frames.shape[1:3]
    rng = np.random.default_rng(0)
    rec = ops.track_records(B, live=1, side=S, frame=rng.integers(0, len(frames), B), x0=rng.integers(0, Wf - S + 1, B), y0=rng.integers(0, Hf - S + 1, B))
    r_d = ops.pack_track_records(rec, device)
    out = torch.empty((B, 3, S, S), device=device)
    host = frames.cpu().numpy()
    squares = [np.ascontiguousarray(host[r['frame'], int(r['y0']):int(r['y0']) + S, int(r['x0']):int(r['x0']) + S]) for r in rec]
    packed = torch.from_numpy(np.concatenate([s.reshape(-1) for s in squares])).to(device)
    table = np.array([[i * S * S * 3, S, S] for i in range(B)], dtype=np.int64)
    params = np.tile(np.array([0.0, 0, 0, S, 0.0, 0.0, 0.0, -1, -1, -1, 0.0]), (B, 1))
    ref = augment.resize_normalize(packed, table, params, size=S)
    got = ops.roi_crop_normalize(frames, r_d, S, out=out)
    equal = bool(torch.equal(got, ref))
    views = torch.from_numpy(ops.view_records(rng.uniform(-30, 30, B), rng.uniform(0.8, 1.2, B), rng.uniform(-20, 20, (B, 2)), S, S // 4)).to(device)
    warped = torch.empty_like(out)
    res = {'identity_equals_resize_normalize': equal, 'B': B, 'S': S}
    for _ in range(3):                                                                             # alternating rounds
        for name, fn in (('roi_crop_normalize_us', lambda: ops.roi_crop_normalize(frames, r_d, S, out=out)),
                         ('resize_normalize_us', lambda: augment.resize_normalize(packed, table, params, out=ref, size=S)),
                         ('affine_warp_images_us', lambda: ops.affine_warp_images(ref, views, out=warped))):
            res.setdefault(name, []).append(1e3 * timed(fn, reps))
    rec2 = ops.track_records(B, live=1, side=2 * S, frame=0, x0=0, y0=0)
    r2 = ops.pack_track_records(rec2, device)
    if min(Hf, Wf) >= 2 * S:
        res['roi_crop_normalize_side_2S_us'] = [1e3 * timed(lambda: ops.roi_crop_normalize(frames, r2, S, out=out), reps) for _ in range(3)]
    return res


def filter_difference(device, frames, S=256):
    """|crop kernel - Pillow chain| on the rendered frames at side / S = 1, 1.5, 2, 3 (integer boxes, centred)."""
    Hf, Wf = frames.shape[1:3]
    host = frames.cpu().numpy()
    out = {}
    for ratio in (1.0, 1.5, 2.0, 3.0):
        side = int(round(ratio * S))
        if side > min(Hf, Wf):
            out['%g' % ratio] = 'not measured: the frame is smaller than the box'
            continue
        x0, y0 = (Wf - side) // 2, (Hf - side) // 2
        n = len(host)
        r_d = ops.pack_track_records(ops.track_records(n, live=1, side=side, frame=np.arange(n), x0=x0, y0=y0), device)
        got = ops.roi_crop_normalize(frames, r_d, S)
        squares = [np.ascontiguousarray(f[y0:y0 + side, x0:x0 + side]) for f in host]
        packed = torch.from_numpy(np.concatenate([s.reshape(-1) for s in squares])).to(device)
        table = np.array([[i * side * side * 3, side, side] for i in range(n)], dtype=np.int64)
        params = np.tile(np.array([0.0, 0, 0, side, 0.0, 0.0, 0.0, -1, -1, -1, 0.0]), (n, 1))
        ref = augment.resize_normalize(packed, table, params, size=S)
        d = (got - ref).abs()
        out['%g' % ratio] = {'mean_abs': float(d.mean()), 'max_abs': float(d.max()), 'equal': bool(torch.equal(got, ref))}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('--image-size', type=int, default=256)
    ap.add_argument('--frame', type=int, default=512, help='side of the rendered frames')
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--hands', type=int, nargs='+', default=[1, 2, 8])
    ap.add_argument('--host-frames', type=int, default=20, help='frames of the host baseline loop per round')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('track_cost.py measures on an MI355X: no GPU here, nothing measured')
    device = torch.device('cuda:0')
    mi355.load()
    S = args.image_size
    recs, gt = hand_sequence(args.frames, args.frame, seed=1)
    frames = render_sequence(recs, args.frame, device)
    host_frames = frames.cpu().numpy()
    model = build_model(args.arch, device)
    res = {'arch': args.arch, 'image_size': S, 'frame': args.frame, 'frames': args.frames, 'device': torch.cuda.get_device_name(0), 'loop': {}}
    for n in args.hands:
        row = {}
        for mode, graph in (('replay', True), ('eager', False)):
            tracker = HandTracker(model, S, (args.frame, args.frame), n, graph=graph).reset(gt_boxes(gt, n))
            for t in range(4):                                                                    # warm-up, capture
                tracker.step(frames[t:t + 1])
            tracker.reset(gt_boxes(gt, n))
            ms, per = loop_wall(tracker.step, frames, args.rounds)
            row[mode + '_ms_per_frame'], row[mode + '_rounds_ms'], row[mode + '_fps'] = ms, per, 1e3 / ms
            if not graph:
                tracker.reset(gt_boxes(gt, n))
                row['eager_split_ms'] = stage_split(tracker, frames[:1])
        step = host_loop(model, S, host_frames, gt_boxes(gt, 1)[0], n, device)
        for t in range(3):
            step(t)
        per = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(args.host_frames):
                step(t % len(host_frames))
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3 / args.host_frames)
        row['host_loop_ms_per_frame'], row['host_loop_rounds_ms'], row['host_loop_fps'] = statistics.median(per), per, 1e3 / statistics.median(per)
        res['loop']['N=%d' % n] = row
        print('N=%d  replay %.3f ms/frame (%.0f fps)  eager %.3f ms/frame (%.0f fps)  host loop %.3f ms/frame (%.0f fps)  split %s' % (
            n, row['replay_ms_per_frame'], row['replay_fps'], row['eager_ms_per_frame'], row['eager_fps'], row['host_loop_ms_per_frame'],
            row['host_loop_fps'], {k: round(v, 4) for k, v in row['eager_split_ms'].items()}))
    res['crop_kernels'] = crop_kernels(device, frames, S)
    print('crop kernels (us, three alternating rounds):', res['crop_kernels'])
    res['filter_difference_vs_pillow'] = filter_difference(device, frames, min(S, 128) if args.frame < 3 * S else S)
    print('crop kernel vs Pillow chain:', res['filter_difference_vs_pillow'])
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
