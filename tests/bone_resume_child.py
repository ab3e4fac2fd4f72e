"""One training process of the resume test of the bone-ratio prior (tests/test_gpu_bone_resume.py starts it):

    python tests/bone_resume_child.py --mode full|resume --out DIR [--from CHECKPOINT] [--forget bone_state]

tests/resume_child.py's helpers on its tiny ResNet-18 fixture with ``--bone-loss on``; the fingerprint and the final state also
hold the running statistics (mean, var, seen).  ``--forget bone_state`` resumes from the checkpoint without that piece."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import resume_child as rc                    # noqa: E402  (puts the package on sys.path)
import resume_ref                            # noqa: E402

FLAGS = rc.COMMON + ['--dtype', 'bf16', '--bone-loss', 'on', '--bone-weight', '0.5', '--bone-margin', '0.5', '--bone-momentum', '0.1']
resume_ref.DOCTORS.setdefault('bone_state', lambda ck: ck.pop('bone_state'))


def build(args, device):
    import train1
    t = rc.build(args, device)
    t['step'].bone = train1.bone_term(args)
    return t


_named_state = rc.named_state


def named_state(t):
    out = _named_state(t)
    stats = t['step'].bone.stats
    if stats.table is not None:
        out['bone/mean'], out['bone/var'], out['bone/seen'] = stats.mean, stats.var, stats.seen
    return out


rc.named_state = named_state                 # (Recorder and write_final look it up when they run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', required=True, choices=['full', 'resume'])
    ap.add_argument('--out', required=True)
    ap.add_argument('--from', dest='ckpt', default=None)
    ap.add_argument('--forget', default='none', choices=['none', 'bone_state'])
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
        assert 'bone_state' in ck and int(ck['bone_state']['seen'].sum()) == 20
        rc.load(t, args, rc.stage(ck, os.path.dirname(os.path.abspath(opt.ckpt)), os.path.join(opt.out, 'from'), opt.forget), device)
    rc.run_epoch(t, args, 1, rc.ITERS, rec)
    rc.save(t, args, opt.out, 1)
    rc.write_final(t, opt.out)
    assert t['step'].graphs is not None


if __name__ == '__main__':
    main()
