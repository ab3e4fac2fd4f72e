#!/usr/bin/env python
"""Key points of the hands in an image sequence, from a trained checkpoint and one rough box per hand (mi355.infer.HandTracker).

    python predict.py -a resnet101 --resume logs/checkpoints/latest.pth --frames DIR --init-box 210 140 330 300 --out hands.npz
    python predict.py -a resnet18 --resume ... --image-size 64 --heatmap-size 16 --synthetic-hands-video 24

Every frame is one graph launch on the GPU: crop, resize, mirror and normalise from the uint8 frame, the forward (with
``--flip-test``), the sub-pixel decode, the confidence, the key points mapped back to the frame and the next box -- no host round trip.
``--track`` (the default) follows the boxes from frame to frame; ``--no-track`` crops every frame by the boxes given.

``--frames DIR``: the images of DIR in sorted order, all of one size, read with PIL.  ``--init-box X0 Y0 X1 Y1`` once per hand, in frame
pixels; ``--left`` after a box marks a left hand, which the network is shown mirrored.  ``--synthetic-hands-video N`` needs no files:
two drawn hands of utils.rendered_dataset interpolated over N frames and rendered on the GPU, so the key points of every frame are
exact and the script prints the end-point error per frame.  ``--out PATH.npz`` holds kp (T, N, K, 2), vis (T, N, K), score (T, N), live
(T, N) and boxes (T, N, 4) (the squares the NEXT frame is cropped by); ``--overlay DIR`` writes every frame with the skeletons drawn.

The tracking constants --tau, --min-joints, --alpha, --grow, --max-lost and --min-side are placeholders: their effect has not been
measured.  --scale 1.5 is the crop of the data sets."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

ARCHS = ('resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152')
IMAGE_TYPES = ('.png', '.jpg', '.jpeg', '.bmp', '.ppm', '.tif', '.tiff', '.webp')
PLACEHOLDER = ' (placeholder: its effect has not been measured)'


class _Box(argparse.Action):
    def __call__(self, parser, ns, values, option_string=None):
        x0, y0, x1, y1 = values
        if not (x1 > x0 and y1 > y0):
            parser.error('--init-box %g %g %g %g has a non-positive extent: give X0 Y0 X1 Y1 with X1 > X0 and Y1 > Y0' % (x0, y0, x1, y1))
        ns.init_box = (ns.init_box or []) + [[x0, y0, x1, y1]]
        ns.left = (ns.left or []) + [False]


class _Left(argparse.Action):
    def __call__(self, parser, ns, values, option_string=None):
        if not ns.left:
            parser.error('--left marks the hand of the --init-box in front of it: there is none')
        ns.left = ns.left[:-1] + [True]


def build_parser():
    from mi355.ops import TRACK_DEFAULTS as D
    p = argparse.ArgumentParser(description='Track hands through an image sequence on the GPU: crop, pose and next box per frame',
                                formatter_class=argparse.RawDescriptionHelpFormatter, epilog=__doc__)
    p.add_argument('-a', '--arch', default='resnet101', choices=ARCHS, help=' | '.join(ARCHS))
    p.add_argument('--resume', default=None, metavar='PATH', help='checkpoint of train1.py (its `model` key); without one the weights are random')
    p.add_argument('--ema_model', default=None, metavar='PATH', help='checkpoint whose `model_ema` key holds the EMA teacher: predicts with it instead')
    p.add_argument('--image-size', type=int, default=256, help='network input side')
    p.add_argument('--heatmap-size', type=int, default=64, help='heat-map side of the main head (informative: the network decides)')
    p.add_argument('--num-head-layers', type=int, default=2)
    p.add_argument('--dtype', default='bf16', choices=['bf16', 'f32', 'fp8', 'mxfp8'], help='compute dtype of activations / packed weights')
    p.add_argument('--decode', default='taylor', choices=['argmax', 'upsample', 'quarter', 'taylor'], help='key-point decode (test.py --decode)')
    p.add_argument('--flip-test', action='store_true', help='average the heat-maps of every crop with those of its mirror image')
    p.add_argument('--flip-shift', default=1, type=int, choices=[0, 1])
    p.add_argument('--conf-beta', default=1.0, type=float, help='the confidence of a joint is the peak of softmax(conf_beta * y), as --teacher-conf defines it')
    p.add_argument('--frames', default=None, metavar='DIR', help='an image sequence: the images of DIR in sorted order, all of one size')
    p.add_argument('--synthetic-hands-video', default=None, type=int, metavar='N', help='instead of --frames: N rendered frames of a moving hand '
                   'with exact key points; prints the end-point error')
    p.add_argument('--video-size', default=256, type=int, help='frame side of --synthetic-hands-video (a multiple of 16 up to 512)')
    p.add_argument('--seed', default=1, type=int, help='seed of --synthetic-hands-video')
    p.add_argument('--render-gap', default=1.0, type=float, help="--synthetic-hands-video: distance of the 'photo' scene from the 'cg' one, as train1.py's")
    p.add_argument('--init-box', nargs=4, type=float, action=_Box, default=None, metavar=('X0', 'Y0', 'X1', 'Y1'),
                   help='rough box of one hand in the first frame, frame pixels; repeat per hand')
    p.add_argument('--left', nargs=0, action=_Left, default=None, help='the hand of the preceding --init-box is a left hand: shown mirrored to the network')
    p.add_argument('--track', dest='track', action='store_true', default=True, help='follow the boxes from frame to frame (default)')
    p.add_argument('--no-track', dest='track', action='store_false', help='re-use the given boxes on every frame')
    p.add_argument('--out', default=None, metavar='PATH.npz', help='write kp, vis, score, live, boxes per frame')
    p.add_argument('--overlay', default=None, metavar='DIR', help='write every frame with the skeletons drawn over it')
    p.add_argument('--scale', type=float, default=D['scale'], help="box side over the key points' extent (1.5: the data sets' crop)")
    p.add_argument('--tau', type=float, default=D['tau'], help='a joint is visible when its confidence reaches this' + PLACEHOLDER)
    p.add_argument('--min-joints', type=int, default=D['min_joints'], help='visible joints a hand needs to move its box' + PLACEHOLDER)
    p.add_argument('--alpha', type=float, default=D['alpha'], help='share of the way the box moves to the new one, 1: no smoothing' + PLACEHOLDER)
    p.add_argument('--grow', type=float, default=D['grow'], help='factor the box of an unseen hand grows by per frame' + PLACEHOLDER)
    p.add_argument('--max-lost', type=int, default=D['max_lost'], help='frames a hand may stay unseen before it is dropped' + PLACEHOLDER)
    p.add_argument('--min-side', type=float, default=D['min_side'], help='least box side, frame pixels' + PLACEHOLDER)
    return p


def read_frames(parser, folder):
    """(T, H, W, 3) uint8 of the images in `folder`, sorted by name."""
    import numpy as np
    from PIL import Image
    if not os.path.isdir(folder):
        parser.error('--frames %s is not a directory' % folder)
    names = sorted(n for n in os.listdir(folder) if n.lower().endswith(IMAGE_TYPES))
    if not names:
        parser.error('--frames %s holds no image (%s)' % (folder, ' '.join(IMAGE_TYPES)))
    frames = []
    for n in names:
        a = np.asarray(Image.open(os.path.join(folder, n)).convert('RGB'), dtype=np.uint8)
        if frames and a.shape != frames[0].shape:
            parser.error('--frames %s: %s has size %dx%d, %s has %dx%d; the frames of a sequence must be of one size'
                         % (folder, n, a.shape[1], a.shape[0], names[0], frames[0].shape[1], frames[0].shape[0]))
        frames.append(a)
    return np.stack(frames), names


def parse(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if (args.frames is None) == (args.synthetic_hands_video is None):
        parser.error('give one of --frames DIR and --synthetic-hands-video N' + (', not both' if args.frames is not None else ''))
    if args.frames is not None and not args.init_box:
        parser.error('--frames needs one --init-box X0 Y0 X1 Y1 per hand')
    if args.synthetic_hands_video is not None and args.synthetic_hands_video < 1:
        parser.error('--synthetic-hands-video N needs N >= 1, got %d' % args.synthetic_hands_video)
    args.host_frames, args.names = read_frames(parser, args.frames) if args.frames is not None else (None, None)
    return args


def build_model(args, device):
    import torch
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    backbone = models.__dict__[args.arch](pretrained=False)
    model = PoseResNetx9(backbone, Upsampling(backbone.out_features), 256, 21, num_head_layers=args.num_head_layers, finetune=True).to(device)
    if args.resume:
        ck = torch.load(args.resume, map_location='cpu', weights_only=False)
        if 'model' not in ck:
            raise SystemExit("checkpoint %s lacks the key 'model'" % args.resume)
        model.load_state_dict(ck['model'])
        print('loaded checkpoint (epoch %s)' % ck.get('epoch'))
    if args.ema_model:
        model.load_state_dict(torch.load(args.ema_model, map_location='cpu', weights_only=False)['model_ema'])
        print('loaded the EMA teacher of %s' % args.ema_model)
    if not (args.resume or args.ema_model):
        print('no --resume / --ema_model: the weights are random')
    return model.eval()


def main(args):
    import numpy as np
    import torch
    import mi355
    from mi355.infer import HandTracker
    if not torch.cuda.is_available():
        raise SystemExit('this path needs an MI355X (HIP kernels only, no CPU fallback)')
    device = torch.device('cuda', torch.cuda.current_device())
    mi355.load()
    mi355.set_compute_dtype(args.dtype)
    gt = None
    if args.synthetic_hands_video is not None:
        from utils.rendered_dataset import hand_sequence, render_sequence
        recs, gt = hand_sequence(args.synthetic_hands_video, args.video_size, seed=args.seed, gap=args.render_gap)
        frames = render_sequence(recs, args.video_size, device)
        boxes = args.init_box or [[float(gt[0, :, 0].min()), float(gt[0, :, 1].min()), float(gt[0, :, 0].max()), float(gt[0, :, 1].max())]]
        left = args.left or [False]
    else:
        frames, boxes, left = torch.from_numpy(args.host_frames).to(device), args.init_box, args.left
    T_, Hf, Wf = (int(v) for v in frames.shape[:3])
    N = len(boxes)
    model = build_model(args, device)
    tracker = HandTracker(model, args.image_size, (Hf, Wf), N, decode=args.decode, flip_test=args.flip_test, flip_shift=args.flip_shift,
                          conf_beta=args.conf_beta, tau=args.tau, min_joints=args.min_joints, scale=args.scale, alpha=args.alpha, grow=args.grow,
                          max_lost=args.max_lost, min_side=args.min_side)
    tracker.reset(boxes, mirror=left, device=device)
    out = None
    for t in range(T_):                                      # nothing in this loop waits for the GPU
        f = frames[t:t + 1]
        res = tracker.step(f) if args.track else tracker.predict(f, boxes, mirror=left)
        if out is None:
            out = [torch.zeros((T_,) + tuple(r.shape), dtype=r.dtype, device=device) for r in res]
        for o, r in zip(out, res):
            o[t].copy_(r)
    torch.cuda.synchronize()
    kp, vis, score, live, bx = (o.cpu().numpy() for o in out)
    tracked = int(live.all(axis=1).sum()) if args.track else T_
    print('frames %d  hands %d  frame %dx%d  %s' % (T_, N, Wf, Hf, 'tracked' if args.track else 'fixed boxes'))
    if gt is not None:
        epe = np.sqrt(((kp[:, 0] - gt) ** 2).sum(-1)).mean(-1)
        for t in range(T_):
            print('frame %3d  EPE %8.3f px  score %.4f  visible %2d  live %d' % (t, epe[t], score[t, 0], int(vis[t, 0].sum()), int(live[t, 0])))
        print('mean EPE %.3f px over %d frames; %d of %d frames tracked' % (float(epe.mean()), T_, tracked, T_))
    else:
        for t in range(T_):
            print('frame %3d  %s  score %s  live %s' % (t, args.names[t], ' '.join('%.4f' % s for s in score[t]), ' '.join(str(int(v)) for v in live[t])))
        print('%d of %d frames tracked' % (tracked, T_))
    if args.out:
        np.savez(args.out, kp=kp, vis=vis, score=score, live=live, boxes=bx)
        print('wrote %s' % args.out)
    if args.overlay:
        from utils.visualize import overlay
        os.makedirs(args.overlay, exist_ok=True)
        host = frames.cpu().numpy()
        for t in range(T_):
            name = os.path.splitext(args.names[t])[0] if args.names else 'frame_%04d' % t
            overlay(host[t], [kp[t, n] for n in range(N)], os.path.join(args.overlay, name + '.png'), labels=None if gt is None else [gt[t]])
        print('wrote %d overlays to %s' % (T_, args.overlay))


if __name__ == '__main__':
    main(parse())
