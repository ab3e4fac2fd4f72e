"""One training process of the resume test of the geometric teacher view (tests/test_gpu_view_step.py starts it):

    python tests/view_resume_child.py --mode full|resume --out DIR [--from CHECKPOINT]

tests/resume_child.py's helpers on its tiny ResNet-18 fixture, with every consumer of the teacher's forward on and
``--mt-view geom``; the fingerprint and the final state also hold the view's RNG state, its count of draws and its last draws."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import resume_child as rc                    # noqa: E402  (puts the package on sys.path)

FLAGS = rc.COMMON + ['--dtype', 'bf16', '--ema-update', 'warmup', '--ema-decay', '0.999', '--mt-loss', 'on', '--coord-loss', 'both',
                     '--mixup', 'on', '--mixup-beta', '0.5', '--mixup-labels', 'teacher', '--mt-view', 'geom', '--view-rot', '20',
                     '--view-scale', '0.8', '1.2', '--view-shift', '0.08', '--view-margin', '2']


def build(args, device):
    from mi355.teacher import GeometricView
    t = rc.build(args, device)
    t['step'].view = GeometricView(rot_deg=args.view_rot, scale=tuple(args.view_scale), shift=args.view_shift, margin=args.view_margin,
                                   seed=args.seed, rank=0)
    return t


_named_state = rc.named_state


def named_state(t):
    import torch
    out = _named_state(t)
    sd = t['step'].view.state_dict()
    out['view/draws'], out['view/rng_state'] = int(sd['draws']), sd['rng_state']
    if sd['params'] is not None:
        out['view/params'] = sd['params']
        out['view/valid'] = t['step']._last_teacher.valid
        assert torch.is_tensor(out['view/valid'])
    return out


rc.named_state = named_state                 # (Recorder and write_final look it up when they run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', required=True, choices=['full', 'resume'])
    ap.add_argument('--out', required=True)
    ap.add_argument('--from', dest='ckpt', default=None)
    opt = ap.parse_args()
    import torch
    import mi355
    import train1
    args = train1.build_parser().parse_args(FLAGS)
    assert torch.cuda.is_available(), 'the resume child needs the GPU'
    device = train1.device
    mi355.load()
    mi355.set_compute_dtype(args.dtype)
    torch.manual_seed(args.seed)
    os.makedirs(opt.out, exist_ok=True)
    fp = os.path.join(opt.out, 'fp.jsonl')
    t = build(args, device)
    rec = rc.Recorder(t, fp)
    if opt.mode == 'full':
        rc.run_epoch(t, args, 0, 0, rec)
        rc.save(t, args, opt.out, 0)
    else:
        ck = torch.load(opt.ckpt, map_location='cpu', weights_only=False)
        assert 'view_state' in ck
        rc.load(t, args, rc.stage(ck, os.path.dirname(os.path.abspath(opt.ckpt)), os.path.join(opt.out, 'from')), device)
    rc.run_epoch(t, args, 1, rc.ITERS, rec)
    rc.save(t, args, opt.out, 1)
    rc.write_final(t, opt.out)
    assert t['step'].graphs is not None and t['step'].view.draws == 2 * rc.ITERS


if __name__ == '__main__':
    main()
