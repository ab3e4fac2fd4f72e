"""One training process of the resume test of the adaptive occlusion (tests/test_gpu_occlude_resume.py starts it):

    python tests/occlude_resume_child.py --mode full|resume --out DIR [--from CHECKPOINT]

tests/resume_child.py's helpers on its tiny ResNet-18 fixture, with ``--mt-loss on``, ``--occlude keypoint`` and ``--teacher-conf``; the
fingerprint and the final state also hold the occlusion's RNG state, its count of draws, its last draws, the boxes and the flags."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import resume_child as rc                    # noqa: E402  (puts the package on sys.path)

FLAGS = rc.COMMON + ['--dtype', 'bf16', '--ema-update', 'warmup', '--ema-decay', '0.999', '--mt-loss', 'on', '--occlude', 'keypoint',
                     '--occlude-p', '0.75', '--occlude-n', '3', '--occlude-size', '0.08', '0.2', '--teacher-conf', '0.001', '--conf-beta', '1']


def build(args, device):
    from mi355.teacher import KeypointOcclusion
    t = rc.build(args, device)
    t['step'].occlude = KeypointOcclusion(prob=args.occlude_p, n=args.occlude_n, size=tuple(args.occlude_size), beta=args.conf_beta,
                                          seed=args.seed, rank=0)
    t['step'].teacher_conf, t['step'].conf_beta = float(args.teacher_conf), float(args.conf_beta)
    return t


_named_state = rc.named_state


def named_state(t):
    out = _named_state(t)
    o = t['step'].occlude
    sd = o.state_dict()
    out['occlude/draws'], out['occlude/rng_state'] = int(sd['draws']), sd['rng_state']
    if sd['u'] is not None:
        out['occlude/u'] = sd['u']
        out['occlude/boxes'], out['occlude/count'], out['occlude/conf'] = o.boxes, o.count, o.conf
    return out


rc.named_state = named_state                 # (Recorder and write_final look it up when they run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', required=True, choices=['full', 'resume'])
    ap.add_argument('--out', required=True)
    ap.add_argument('--from', dest='ckpt', default=None)
    ap.add_argument('--forget', default=None, help='resume: drop this key from the checkpoint first')
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
        assert 'occlude_state' in ck
        if opt.forget:
            del ck[opt.forget]
        rc.load(t, args, rc.stage(ck, os.path.dirname(os.path.abspath(opt.ckpt)), os.path.join(opt.out, 'from')), device)
    rc.run_epoch(t, args, 1, rc.ITERS, rec)
    rc.save(t, args, opt.out, 1)
    rc.write_final(t, opt.out)
    assert t['step'].graphs is not None
    assert opt.forget or t['step'].occlude.draws == 2 * rc.ITERS


if __name__ == '__main__':
    main()
