#!/usr/bin/env python
"""Evaluation entry point, mirror of the reference's ``test.py`` (= its train1.py with ``--checkpoint`` instead of
``--resume`` and one ``validate()`` on the source and target test splits, test.py:157,192-226,584).

    python test.py data/H3D -t Hand3DStudio --checkpoint models/H3D_best_754.pth [--synthetic] [--ema_model .../model_ema.pth]

``--dump-preds PATH`` (implies ``--metrics full``) writes the predictions of every evaluated split for tools outside this
script: ``PATH.source.npz``, ``PATH.target.npz`` and, with ``--ema_model``, ``PATH.ema.npz``, each with ``pred`` (N,K,2) and
``gt`` (N,K,2) in image pixels, ``visible`` (N,K), ``maxval`` (N,K), ``image_size``, ``decode``, ``flip_test``, ``flip_shift``,
``thresholds`` and the reported ``epe``, ``auc`` and ``pck_curve``, in data-set order.

``--flip-test`` (with ``--flip-shift {0,1}``) evaluates the average of the heat-maps of every image and its mirror image;
``--decode quarter|taylor`` decode the key points of ``--metrics full`` to sub-pixel positions.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch

import mi355
import train1 as T
import uda.model as models
from uda.model.loss import JointsKLLoss
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9
from utils.logger import CompleteLogger


def main(args):
    T.init_distributed()
    logger = CompleteLogger(args.log, 'test', quiet=T.RANK != 0)
    print(args)
    if T.device.type != 'cuda':
        raise SystemExit('this evaluation path needs an MI355X (HIP kernels only, no CPU fallback)')
    mi355.load()
    mi355.set_compute_dtype(args.dtype)
    _, val_s, _, val_t = T.build_datasets(args)
    val_source_loader, val_target_loader = T.make_loader(val_s, args, False), T.make_loader(val_t, args, False)
    backbone = models.__dict__[args.arch](pretrained=False)
    model = PoseResNetx9(backbone, Upsampling(backbone.out_features), 256, val_s.num_keypoints,
                         num_head_layers=args.num_head_layers, finetune=True).to(T.device)
    if args.checkpoint:
        ck = torch.load(args.checkpoint, map_location='cpu', weights_only=False)
        # the reference requires these keys (test.py:192-201); only `model` and `epoch` are needed to evaluate
        missing = [k for k in ('model',) if k not in ck]
        if missing:
            raise SystemExit('checkpoint lacks %s' % missing)
        model.load_state_dict(ck['model'])
        print('loaded checkpoint (epoch %s)' % ck.get('epoch'))
    criterion = JointsKLLoss()

    def evaluate(loader, split):
        if not args.dump_preds:
            return T.validate(loader, model, criterion, args)
        dump = {}
        acc = T.validate(loader, model, criterion, args, dump=dump)
        if T.RANK == 0:                                   # (gathered in validate: data-set order, one copy per split)
            import numpy as np
            np.savez('%s.%s.npz' % (args.dump_preds, split), **dump)
        return acc

    s_acc = evaluate(val_source_loader, 'source')
    t_acc = evaluate(val_target_loader, 'target')
    print("Source: {:4.3f} Target: {:4.3f}".format(s_acc['all'], t_acc['all']))
    for name, acc in t_acc.items():
        print("{}: {:4.3f}".format(name, acc))
    if args.ema_model:
        # the EMA teacher of a --ema-update run (its model_ema.pth): same network, the file's `model_ema` weights
        model.load_state_dict(torch.load(args.ema_model, map_location='cpu', weights_only=False)['model_ema'])
        e_acc = evaluate(val_target_loader, 'ema')
        print("ema: {:4.3f}".format(e_acc['all']))
    logger.close()


if __name__ == '__main__':
    p = T.build_parser('Evaluation for Keypoint Detection Domain Adaptation')
    p.add_argument('--checkpoint', type=str, default=None, help='where restore model parameters from.')
    p.add_argument('--dump-preds', type=str, default=None, metavar='PATH', help='write PATH.<split>.npz (pred, gt, visible, maxval in '
                   'image pixels, thresholds, epe, auc, pck_curve) per evaluated split; implies --metrics full')
    main(p.parse_args())
