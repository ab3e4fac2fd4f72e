"""A resumed run equals the run that never stopped, bit for bit.

Every test here is about processes: tests/resume_child.py is started as a fresh process (never exec'ed, one at a time, never
retried) that builds what train1.py builds, drives ``train1.train()`` -- its "three eager iterations, then capture, then replay" rule is
the one that runs, nothing is mirrored -- and checkpoints through ``utils.checkpoint``, the functions train1.py calls.  Two epochs of
5 iterations; after every iteration the child writes one SHA-256 per piece of training state (tests/resume_ref.py), at the end
the tensors themselves.  Per configuration (tests/resume_child.CONFIGS):

* control: the uninterrupted run twice -- a condition on the reference, and the cross-process determinism check;
* the run resumed from the first's epoch-0 checkpoint: iterations 5..9 and the final tensors equal the uninterrupted run's.  The
  uninterrupted epoch 1 is all replays, the resumed one three eager iterations, a capture and two replays;
* the checkpoints the runs wrote load to equal tensors key by key;
* teeth (two configurations): with one piece of the checkpoint forgotten at a time, iteration 6 must differ; with nothing
  forgotten -- asked first and last in that process -- it must not.

Everything is compared by bytes, so there is no tolerance."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import PKG
import resume_ref

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'resume_child.py')
CONFIGS = ['plain-bf16', 'all-f32', 'all-bf16-adamw', 'plain-fp8', 'plain-mxfp8']
ITERS = 5
_BROKEN = []                 # why no further GPU process may be started (a child died of a signal, a fault or its time limit)
WALL = {}                    # (config, mode) -> seconds


class Runs:
    """The children of this module, started when a test first asks for one and at most once each."""

    def __init__(self, root):
        self.root, self.done = root, {}

    def _start(self, config, mode, tag, ckpt=None):
        key = (config, tag)
        if key in self.done:
            out = self.done[key]
            if isinstance(out, str) and out.startswith('FAILED'):
                pytest.fail('the %s child of %s failed earlier: %s' % (tag, config, out))
            return out
        if _BROKEN:
            pytest.fail('no further GPU process is started: %s' % _BROKEN[0])
        out = str(self.root / ('%s_%s' % (config, tag)))
        cmd = [sys.executable, CHILD, '--config', config, '--mode', mode, '--out', out] + (['--from', ckpt] if ckpt else [])
        t0 = time.time()
        try:
            r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            _BROKEN.append('the %s child of %s ran into its time limit' % (tag, config))
            self.done[key] = 'FAILED: time limit'
            pytest.fail(_BROKEN[0])
        WALL[key] = time.time() - t0
        print('resume child %s %s: %.1f s' % (config, tag, WALL[key]))
        text = r.stdout + r.stderr
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or 'illegal memory access' in text:
            _BROKEN.append('the %s child of %s ended with status %d' % (tag, config, r.returncode))
        if r.returncode != 0 or _BROKEN:
            self.done[key] = 'FAILED: status %d' % r.returncode
            pytest.fail('resume child %s %s: status %d\n%s' % (config, tag, r.returncode, text[-4000:]))
        self.done[key] = out
        return out

    def control(self, config):
        return self._start(config, 'full', 'control')

    def full(self, config):
        self.control(config)                      # the reference is established first
        return self._start(config, 'full', 'full')

    def resume(self, config):
        return self._start(config, 'resume', 'resume', os.path.join(self.full(config), 'checkpoints', '0.pth'))

    def forget(self, config):
        return self._start(config, 'forget', 'forget', os.path.join(self.full(config), 'checkpoints', '0.pth'))


@pytest.fixture(scope='module')
def runs(gpu, tmp_path_factory):
    return Runs(tmp_path_factory.mktemp('resume'))


def _lines(out):
    return resume_ref.read_lines(os.path.join(out, 'fp.jsonl'))


def _final(out):
    with np.load(os.path.join(out, 'final.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _ckpt(out, name):
    return torch.load(os.path.join(out, 'checkpoints', name), map_location='cpu', weights_only=False)


@pytest.mark.parametrize('config', CONFIGS)
def test_uninterrupted_run_is_the_same_in_two_processes(runs, config):
    a, b = runs.control(config), runs.full(config)
    la, lb = _lines(a), _lines(b)
    assert [l['it'] for l in la] == [l['it'] for l in lb] == list(range(2 * ITERS))
    assert len({l['all'] for l in la}) == 2 * ITERS                         # every iteration moves the state
    msg = resume_ref.describe_difference(la, lb, None, _final(a), _final(b))
    assert msg is None, '%s, two uninterrupted runs: %s' % (config, msg)


@pytest.mark.parametrize('config', CONFIGS)
def test_resumed_run_equals_the_uninterrupted_one(runs, config):
    full, res = runs.full(config), runs.resume(config)
    lf, lr = _lines(full), _lines(res)
    assert [l['it'] for l in lr] == list(range(ITERS, 2 * ITERS))
    msg = resume_ref.describe_difference(lf, lr, range(ITERS, 2 * ITERS), _final(full), _final(res))
    assert msg is None, '%s, resumed against uninterrupted: %s' % (config, msg)


@pytest.mark.parametrize('config', CONFIGS)
def test_saved_checkpoints_are_equal(runs, config):
    """What is saved after replays equals what is saved after eager iterations, and in another process."""
    ctl, full, res = runs.control(config), runs.full(config), runs.resume(config)
    for what, a, b, names in (('epoch 0 of two uninterrupted runs', ctl, full, ('0.pth', 'model_ema_0.pth')),
                              ('epoch 1, uninterrupted and resumed', full, res, ('1.pth', 'model_ema.pth'))):
        for name in names:
            ca, cb = _ckpt(a, name), _ckpt(b, name)
            assert len(resume_ref.flatten(ca)) > 100
            bad = resume_ref.compare_checkpoints(ca, cb)
            assert not bad, '%s, %s, %s: %d keys differ, first %s' % (config, what, name, len(bad), bad[:5])


@pytest.mark.parametrize('config', sorted(resume_ref.PIECES))
def test_every_forgotten_piece_is_noticed(runs, config):
    full = {l['it']: l for l in _lines(runs.full(config))}[ITERS + 1]
    with open(os.path.join(runs.forget(config), 'forget.json')) as f:
        got = json.load(f)
    assert set(got) == set(resume_ref.PIECES[config]) | {'none', 'none_again'}
    for control in ('none', 'none_again'):       # nothing forgotten: the two iterations of that process are the full run's
        d = resume_ref.first_difference([full], [got[control]])
        assert d is None, '%s, nothing forgotten (%s): first difference at iteration %d in %s' % ((config, control) + d)
    unnoticed = [p for p in resume_ref.PIECES[config] if got[p]['all'] == full['all']]
    assert not unnoticed, '%s: forgetting %s changes nothing by iteration %d' % (config, unnoticed, ITERS + 1)
    print({p: resume_ref.first_difference([full], [got[p]])[1] for p in resume_ref.PIECES[config]})
