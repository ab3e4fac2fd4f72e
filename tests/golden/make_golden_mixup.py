"""Generate the cross-domain mixup golden vectors by calling the reference's live mixup (uda/model/loss.py:13-24; run where the
reference tree is present).  Writes tests/golden/g17_mixup.npz.  Import recipe as make_golden_ema.py: namespace stubs for the
reference's packages; no reference source is copied, only arrays are stored.

    python tests/golden/make_golden_mixup.py

B = 5, images 3 x 16 x 16, heat-maps 21 x 8 x 8, weights (B, 21, 1) in {0, 1}.  One set of inputs `x_s, hm_s, w_s, x_t, hm_t, w_t`;
per beta in (0.5, 1.0), under `torch.manual_seed(SEED)` set right before the call: `b<beta>/lam` (B,), the coefficients the call
drew -- max(mix, 1 - mix), obtained by drawing the reference's expression again under the same seed -- and the six outputs
`b<beta>/out0 .. out5` in the order the function returns them.  `seed` holds SEED."""
import os
import sys
import types
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference tree: REFERENCE_ROOT, else a directory `reference` beside this repository
REF = os.environ.get('REFERENCE_ROOT') or os.path.normpath(os.path.join(HERE, '..', '..', '..', 'reference'))
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

SEED = 1713
B, C, S, K, H = 5, 3, 16, 21, 8
BETAS = (0.5, 1.0)


def tag(beta):
    return 'b%g' % beta


def main():
    ref_loss.device = torch.device('cpu')              # the module-level device of the reference: the CPU here
    gen = torch.Generator().manual_seed(SEED + 1)
    x_s, x_t = torch.randn(B, C, S, S, generator=gen), torch.randn(B, C, S, S, generator=gen) * 0.7 + 0.1
    hm_s, hm_t = torch.rand(B, K, H, H, generator=gen), torch.rand(B, K, H, H, generator=gen) ** 4
    w_s = (torch.rand(B, K, 1, generator=gen) < 0.8).float()
    w_t = (torch.rand(B, K, 1, generator=gen) < 0.6).float()
    out = dict(x_s=x_s, hm_s=hm_s, w_s=w_s, x_t=x_t, hm_t=hm_t, w_t=w_t, seed=torch.tensor(SEED))
    for beta in BETAS:
        torch.manual_seed(SEED)
        res = ref_loss.mixup(x_s, hm_s, w_s, x_t, hm_t, w_t, beta)
        assert len(res) == 6 and res[2] is res[5]
        torch.manual_seed(SEED)                        # the same draw once more, to store what the call used
        mix = torch.distributions.beta.Beta(torch.tensor(beta), torch.tensor(beta)).rsample(sample_shape=(B, 1, 1, 1))
        lam = torch.max(mix, 1 - mix)
        assert torch.equal(res[0], x_s * lam + x_t * (1. - lam))
        out[tag(beta) + '/lam'] = lam.reshape(-1)
        for i, r in enumerate(res):
            out['%s/out%d' % (tag(beta), i)] = r
    arrs = {k: v.numpy() for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, 'g17_mixup.npz'), **arrs)
    print('g17_mixup', len(arrs), 'arrays')


if __name__ == '__main__':
    main()
