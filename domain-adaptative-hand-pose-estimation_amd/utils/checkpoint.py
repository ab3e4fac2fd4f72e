"""The epoch checkpoint of train1.py as two functions: what ``main`` writes after every epoch and what ``--resume`` reads back.

Layout (reference train1.py:248-268 plus additive keys): ``<epoch>.pth`` holds ``model``, ``optimizer_f`` / ``_h`` / ``_h_adv`` and their
``lr_scheduler_*``, ``epoch`` and ``args``; additive: the same for ``h_adv2`` / ``h_adv3``, ``gl_iter_num``, ``ema_state``, ``proto_state``,
``bone_state``, ``mixup_state``, ``view_state``, ``occlude_state`` and -- ``--dtype fp8`` -- ``fp8_state``.  ``model_ema.pth`` beside it holds ``model_ema``.  Every piece is restored into
objects that have not run an iteration yet: optimizers that are not flat, a teacher without its mirror layout, no graphs.
"""
import os

import torch

import mi355
from mi355.nn import fp8_state_dict, load_fp8_state_dict
from mi355.optim import check_state_dict_kind

REFERENCE_KEYS = ('model', 'optimizer_f', 'optimizer_h', 'optimizer_h_adv', 'lr_scheduler_f', 'lr_scheduler_h', 'lr_scheduler_h_adv',
                  'epoch', 'args')
ADDITIVE_KEYS = ('optimizer_h_adv2', 'optimizer_h_adv3', 'lr_scheduler_h_adv2', 'lr_scheduler_h_adv3', 'gl_iter_num')
OPTIONAL_KEYS = ('ema_state', 'proto_state', 'bone_state', 'mixup_state', 'view_state', 'occlude_state', 'fp8_state')      # written when the run has the piece of state


def ema_path_beside(path):
    return os.path.join(os.path.dirname(os.path.abspath(path)), 'model_ema.pth')


def training_state(epoch, args, model, opts, scheds, step, ema):
    """The dict ``save_training_state`` writes as ``<epoch>.pth``."""
    ck_extra = {'ema_state': ema.state_dict()} if ema is not None else {}
    if getattr(step, 'proto', None) is not None:
        ck_extra['proto_state'] = step.proto.state_dict()
    if getattr(step, 'bone', None) is not None:
        ck_extra['bone_state'] = step.bone.state_dict()
    if getattr(step, 'mixup', None) is not None:
        ck_extra['mixup_state'] = step.mixup.state_dict()
    if getattr(step, 'view', None) is not None:
        ck_extra['view_state'] = step.view.state_dict()
    if getattr(step, 'occlude', None) is not None:
        ck_extra['occlude_state'] = step.occlude.state_dict()
    fp8 = fp8_state_dict(model) if mi355.fp8_convs() else None
    if fp8 is not None:
        ck_extra['fp8_state'] = fp8                     # the delayed-scaling records of --dtype fp8 (mi355.nn.fp8_state_dict)
    return {'model': model.state_dict(), **ck_extra,
            'optimizer_f': opts['f'].state_dict(), 'optimizer_h': opts['h'].state_dict(),
            'optimizer_h_adv': opts['h_adv'].state_dict(),
            'lr_scheduler_f': scheds['f'].state_dict(), 'lr_scheduler_h': scheds['h'].state_dict(),
            'lr_scheduler_h_adv': scheds['h_adv'].state_dict(), 'epoch': epoch, 'args': args,
            # additive keys: close the reference's resume gaps
            'optimizer_h_adv2': opts['h_adv2'].state_dict(), 'optimizer_h_adv3': opts['h_adv3'].state_dict(),
            'lr_scheduler_h_adv2': scheds['h_adv2'].state_dict(), 'lr_scheduler_h_adv3': scheds['h_adv3'].state_dict(),
            'gl_iter_num': model.gl_layer.iter_num}


def save_training_state(path, epoch, args, model, model_ema, opts, scheds, step, ema):
    """Write ``path`` (the epoch's checkpoint) and ``model_ema.pth`` beside it.  The caller is rank 0."""
    torch.save(training_state(epoch, args, model, opts, scheds, step, ema), path)
    torch.save({'model_ema': model_ema.state_dict()}, ema_path_beside(path))


def apply_training_state(ck, path, args, model, model_ema, opts, scheds, step, ema, device):
    """Restore the loaded dict `ck` (read from `path`) into freshly built objects; returns the epoch to start at."""
    model.load_state_dict(ck['model']); model_ema.load_state_dict(ck['model'])
    try:                                             # (SGD state under --optimizer adam, or the reverse: say so, no KeyError later)
        for k in opts:
            if 'optimizer_' + k in ck:
                check_state_dict_kind(opts[k], ck['optimizer_' + k], '%s: optimizer_%s' % (path, k))
    except ValueError as e:
        raise SystemExit('--resume ' + str(e))
    for k, name in (('f', 'optimizer_f'), ('h', 'optimizer_h'), ('h_adv', 'optimizer_h_adv')):
        opts[k].load_state_dict(ck[name]); scheds[k].load_state_dict(ck['lr_scheduler' + name[len('optimizer'):]])
    for k in ('h_adv2', 'h_adv3'):                    # additive keys (the reference never saved these two)
        if 'optimizer_' + k in ck:
            opts[k].load_state_dict(ck['optimizer_' + k]); scheds[k].load_state_dict(ck['lr_scheduler_' + k])
    model.gl_layer.iter_num = ck.get('gl_iter_num', 0)
    start_epoch = ck['epoch'] + 1
    beside = ema_path_beside(path)
    if ema is not None:
        # the teacher: --ema_model, else the model_ema.pth written next to the resumed checkpoint, else the model (above)
        ema_path = getattr(args, 'ema_model', None) or (beside if os.path.exists(beside) else None)
        if ema_path is not None:
            model_ema.load_state_dict(torch.load(ema_path, map_location='cpu', weights_only=False)['model_ema'])
        if 'ema_state' in ck:
            ema.load_state_dict(ck['ema_state'])
    elif os.path.exists(beside):
        # --ema-update off: the frozen teacher keeps the weights the saved run held (and wrote beside its checkpoints after every
        # epoch) instead of becoming a copy of the model at the epoch it happens to be resumed at
        model_ema.load_state_dict(torch.load(beside, map_location='cpu', weights_only=False)['model_ema'])
    if getattr(step, 'proto', None) is not None and 'proto_state' in ck:
        step.proto.load_state_dict(ck['proto_state'], device)      # both prototype memories and m
    if getattr(step, 'bone', None) is not None and 'bone_state' in ck:
        step.bone.load_state_dict(ck['bone_state'])                 # mean, var and seen of the bone-ratio statistics
    if getattr(step, 'mixup', None) is not None and 'mixup_state' in ck:
        step.mixup.load_state_dict(ck['mixup_state'])               # the RNG state of the blend coefficients (rank 0's)
    if getattr(step, 'view', None) is not None and 'view_state' in ck:
        step.view.load_state_dict(ck['view_state'])                 # the RNG state of the teacher's geometric views (rank 0's)
    if getattr(step, 'occlude', None) is not None and 'occlude_state' in ck:
        step.occlude.load_state_dict(ck['occlude_state'])           # the RNG state of the occlusion boxes (rank 0's)
    if ck.get('fp8_state') is not None and mi355.fp8_convs():
        try:                                         # --dtype fp8: the scaling records, to the layers that owned them
            load_fp8_state_dict(model, ck['fp8_state'], device)
        except ValueError as e:
            raise SystemExit('--resume %s: %s' % (path, e))
    return start_epoch


def load_training_state(path, args, model, model_ema, opts, scheds, step, ema, device):
    """``--resume path``: read the checkpoint and restore it (``apply_training_state``); returns the epoch to start at."""
    ck = torch.load(path, map_location='cpu', weights_only=False)
    return apply_training_state(ck, path, args, model, model_ema, opts, scheds, step, ema, device)
