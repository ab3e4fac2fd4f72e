"""A resumed ``--occlude keypoint`` run equals the uninterrupted one bit for bit, and a checkpoint without ``occlude_state`` is
noticed.  tests/occlude_resume_child.py runs as fresh processes (the scheme of tests/test_gpu_resume.py): two epochs of five
iterations on the tiny ResNet-18 fixture, graphs captured after three, one SHA-256 per piece of training state after every
iteration -- the occlusion's RNG state, its draws, the boxes and the confidence flags among them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resume_ref
from conftest import PKG

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_resumed_run_equals_the_uninterrupted_one_and_a_dropped_occlude_state_is_noticed(gpu, tmp_path):
    child = os.path.join(HERE, 'occlude_resume_child.py')
    env = dict(os.environ, PYTHONPATH=PKG)

    def start(mode, out, ckpt=None, forget=None):
        cmd = ['timeout', '-k', '10', '300', sys.executable, child, '--mode', mode, '--out', out] + (['--from', ckpt] if ckpt else []) + \
            (['--forget', forget] if forget else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=330)
        assert r.returncode == 0, '%s child: status %d\n%s' % (mode, r.returncode, (r.stdout + r.stderr)[-4000:])
        return out

    full = start('full', str(tmp_path / 'full'))
    ckpt = os.path.join(full, 'checkpoints', '0.pth')
    res = start('resume', str(tmp_path / 'resume'), ckpt)
    lost = start('resume', str(tmp_path / 'lost'), ckpt, forget='occlude_state')
    lf, lr, ll = (resume_ref.read_lines(os.path.join(d, 'fp.jsonl')) for d in (full, res, lost))
    assert [l['it'] for l in lf] == list(range(10)) and [l['it'] for l in lr] == list(range(5, 10))
    assert len({l['all'] for l in lf}) == 10
    assert all(k in l['tensors'] for l in lf for k in ('occlude/u', 'occlude/boxes', 'occlude/count', 'occlude/conf', 'out/loss_mt'))
    assert len({l['tensors']['occlude/boxes'] for l in lf}) > 5       # boxes are drawn, and not the same ones every iteration

    def final(d):
        with np.load(os.path.join(d, 'final.npz'), allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    msg = resume_ref.describe_difference(lf, lr, range(5, 10), final(full), final(res))
    assert msg is None, 'resumed against uninterrupted: %s' % msg
    # without occlude_state the draws start over: iteration 5 already differs, in the occlusion's own state first
    d = resume_ref.first_difference(lf, ll, range(5, 10))
    assert d is not None and d[0] == 5, d
