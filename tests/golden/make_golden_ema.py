"""Generate the EMA-teacher golden vectors by calling the reference's live update_ema_variables5 and update_ema_variables2
(uda/model/loss.py:229-261; run where the reference tree is present).  Writes tests/golden/g11_ema.npz.  Import recipe as
make_golden.py: namespace stubs for the reference's packages; no reference source is copied, only arrays are stored.

    python tests/golden/make_golden_ema.py

A tiny two-module network (conv 3 -> 4, 3x3, no bias; BatchNorm2d(4)) gives the state dict: conv weight, BatchNorm weight, bias,
running_mean, running_var, num_batches_tracked.  Stored: the teacher's initial state `init/<key>`, the main model's state at three
successive updates `main<t>/<key>`, and the teacher after update t as `m999_<t>/<key>` (update_ema_variables5, m = 0.999),
`m9_<t>/<key>` (m = 0.9) and `warm_<t>/<key>` (update_ema_variables2, alpha = 0.999, global_step = t = 0, 1, 2)."""
import os
import sys
import types
import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get('REFERENCE_ROOT', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
np.int = int
np.float = float


def _stub(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub('utils', f'{REF}/utils')
_stub('uda', f'{REF}/uda')
_stub('uda.model', f'{REF}/uda/model')
_stub('uda.model.resnet', _resnet=None, Bottleneck=None)

import uda.model.loss as ref_loss  # noqa: E402

KEYS = ['0.weight', '1.weight', '1.bias', '1.running_mean', '1.running_var', '1.num_batches_tracked']


def net():
    return nn.Sequential(nn.Conv2d(3, 4, 3, bias=False), nn.BatchNorm2d(4))


def fill(m, gen, tracked):
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if 'num_batches_tracked' in k:
                v.fill_(tracked)
            elif 'running_var' in k:
                v.copy_(torch.rand(v.shape, generator=gen) + 0.5)
            else:
                v.copy_(torch.randn(v.shape, generator=gen))


def main():
    gen = torch.Generator().manual_seed(1107)
    out = {}
    init = net()
    fill(init, gen, 0)
    assert list(init.state_dict()) == KEYS
    mains = []
    for t in range(3):
        m = net()
        fill(m, gen, 7 * t + 3)
        mains.append(m)
        out.update({'main%d/%s' % (t, k): v.clone() for k, v in m.state_dict().items()})
    out.update({'init/' + k: v.clone() for k, v in init.state_dict().items()})
    for tag, upd in (('m999', lambda mn, e, t: ref_loss.update_ema_variables5(mn, e, 0.999)),
                     ('m9', lambda mn, e, t: ref_loss.update_ema_variables5(mn, e, 0.9)),
                     ('warm', lambda mn, e, t: ref_loss.update_ema_variables2(mn, e, 0.999, t))):
        ema = net()
        ema.load_state_dict(init.state_dict())
        for t in range(3):
            with torch.no_grad():
                upd(mains[t], ema, t)
            out.update({'%s_%d/%s' % (tag, t, k): v.clone() for k, v in ema.state_dict().items()})
    arrs = {k: v.numpy() for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, 'g11_ema.npz'), **arrs)
    print('g11_ema', len(arrs), 'arrays')


if __name__ == '__main__':
    main()
