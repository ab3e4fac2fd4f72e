"""What the resume suite compares with (tests/resume_child.py writes, tests/test_gpu_resume.py and tests/test_resume_cpu.py read):

* ``fingerprint``: one SHA-256 per named piece of training state, over its dtype, shape and bytes -- so two NaNs with different
  payloads, or -0.0 and 0.0, are different -- and one over all of them; a line of ``fp.jsonl`` is ``{'it': g, 'all': ..., 'tensors': {...}}``;
* ``first_difference`` / ``describe_difference``: two lists of such lines, iteration by iteration -> the first (iteration, name);
* ``count_differences``: two ``final.npz`` files, array by array -> how many elements differ, by bytes;
* ``compare_checkpoints``: two loaded checkpoint dicts, key by key;
* ``doctor``: the pieces of a checkpoint the ``forget`` child drops or spoils, one at a time.

Nothing here needs a GPU."""
import argparse
import copy
import hashlib
import json
import struct

import numpy as np
import torch


# ---------------------------------------------------------------- bytes of one piece of state
def as_array(v):
    """torch tensor (any device; bf16 as its int16 bits) / numpy array / python scalar / list of scalars -> a C-contiguous numpy array
    that holds exactly its bits (python floats as float64, ints as int64)."""
    if torch.is_tensor(v):
        t = v.detach().cpu().contiguous()
        if t.dtype == torch.bfloat16:
            t = t.view(torch.int16)
        return np.ascontiguousarray(t.numpy())
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v)
    if isinstance(v, (bool, int)):
        return np.asarray(int(v), dtype=np.int64)
    if isinstance(v, float):
        return np.frombuffer(struct.pack('<d', v), dtype='<f8').reshape(()).copy()
    if isinstance(v, (list, tuple)):
        if all(isinstance(x, (bool, int)) for x in v):
            return np.asarray([int(x) for x in v], dtype=np.int64)
        return np.frombuffer(b''.join(struct.pack('<d', float(x)) for x in v), dtype='<f8').copy()
    raise TypeError('no byte form for %r' % type(v))


def digest(v):
    a = as_array(v)
    h = hashlib.sha256()
    h.update(('%s|%s|' % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def fingerprint(named):
    """{name: value} -> {'tensors': {name: sha256}, 'all': sha256 over the names and digests in sorted order}."""
    per = {k: digest(named[k]) for k in sorted(named)}
    h = hashlib.sha256()
    for k, d in per.items():
        h.update(k.encode()); h.update(b'='); h.update(d.encode()); h.update(b';')
    return {'tensors': per, 'all': h.hexdigest()}


def read_lines(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


# ---------------------------------------------------------------- two runs, line by line
def first_difference(a, b, iterations=None):
    """a, b: lists of fingerprint lines.  None when the lines of every iteration in `iterations` (default: every iteration either
    has) agree; else (iteration, name) of the first that do not -- name is the first differing tensor in sorted order,
    '<missing in a|b>' when one side has no line for the iteration or the tensor, '<all>' when only the totals differ."""
    ia, ib = {l['it']: l for l in a}, {l['it']: l for l in b}
    its = sorted(set(ia) | set(ib)) if iterations is None else list(iterations)
    for it in its:
        la, lb = ia.get(it), ib.get(it)
        if la is None or lb is None:
            return it, '<missing in %s>' % ('a' if la is None else 'b')
        if la['all'] == lb['all'] and la['tensors'] == lb['tensors']:
            continue
        for k in sorted(set(la['tensors']) | set(lb['tensors'])):
            if k not in la['tensors'] or k not in lb['tensors']:
                return it, '%s <missing in %s>' % (k, 'a' if k not in la['tensors'] else 'b')
            if la['tensors'][k] != lb['tensors'][k]:
                return it, k
        return it, '<all>'
    return None


def as_bytes_per_element(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8).reshape(a.size, a.itemsize) if a.size else np.zeros((0, max(a.itemsize, 1)), np.uint8)


def count_differences(fa, fb):
    """fa, fb: {name: array} (np.load of two final.npz) -> {name: number of elements whose bytes differ}; a name one side lacks, or
    a different dtype or shape, counts every element (at least 1).  Empty when the two are equal."""
    out = {}
    for k in sorted(set(fa) | set(fb)):
        if k not in fa or k not in fb:
            out[k] = max(int((fa[k] if k in fa else fb[k]).size), 1)
            continue
        x, y = np.asarray(fa[k]), np.asarray(fb[k])
        if x.dtype != y.dtype or x.shape != y.shape:
            out[k] = max(int(x.size), int(y.size), 1)
            continue
        n = int((as_bytes_per_element(x) != as_bytes_per_element(y)).any(axis=1).sum())
        if n:
            out[k] = n
    return out


def describe_difference(a, b, iterations=None, final_a=None, final_b=None):
    """None when equal; else a message with the first differing (iteration, tensor) and, given the two final.npz contents, how
    many elements of that tensor (and of how many tensors in all) differ at the end."""
    d = first_difference(a, b, iterations)
    counts = count_differences(final_a, final_b) if final_a is not None and final_b is not None else {}
    if d is None and not counts:
        return None
    msg = 'fingerprints agree' if d is None else 'first difference at iteration %d in %s' % d
    if final_a is not None and final_b is not None:
        name = d[1] if d is not None else None
        msg += '; final.npz: %d tensors differ' % len(counts)
        if name in counts:
            msg += ', %s in %d elements' % (name, counts[name])
        elif counts:
            k = sorted(counts)[0]
            msg += ', first %s in %d elements' % (k, counts[k])
    return msg


# ---------------------------------------------------------------- two checkpoints, key by key
def flatten(obj, prefix=''):
    """A checkpoint dict -> {path: leaf}; dicts, lists, tuples and argparse.Namespace are walked, everything else is a leaf."""
    if isinstance(obj, argparse.Namespace):
        obj = vars(obj)
    if isinstance(obj, dict):
        out = {}
        for k in obj:
            out.update(flatten(obj[k], '%s/%s' % (prefix, k)))
        return out or {prefix + '/<empty>': None}
    if isinstance(obj, (list, tuple)) and not all(isinstance(x, (bool, int, float)) for x in obj):
        out = {}
        for i, x in enumerate(obj):
            out.update(flatten(x, '%s/%d' % (prefix, i)))
        return out or {prefix + '/<empty>': None}
    return {prefix: obj}


def leaf_equal(x, y):
    if torch.is_tensor(x) or torch.is_tensor(y) or isinstance(x, (np.ndarray, float)) or isinstance(y, (np.ndarray, float)):
        try:
            return type(x) == type(y) and digest(x) == digest(y)
        except TypeError:
            return False
    if isinstance(x, (list, tuple)) and isinstance(y, (list, tuple)) and x and all(isinstance(v, (bool, int, float)) for v in list(x) + list(y)):
        return len(x) == len(y) and [type(v) for v in x] == [type(v) for v in y] and digest(list(x)) == digest(list(y))
    return type(x) == type(y) and x == y


def compare_checkpoints(a, b, ignore=()):
    """The paths at which two loaded checkpoints differ (a leaf one side lacks included), sorted; `ignore`: path prefixes left out."""
    fa, fb = flatten(a), flatten(b)
    bad = []
    for k in sorted(set(fa) | set(fb)):
        if any(k.startswith(p) for p in ignore):
            continue
        if k not in fa or k not in fb or not leaf_equal(fa[k], fb[k]):
            bad.append(k)
    return bad


# ---------------------------------------------------------------- what the forget child does to a checkpoint
def _zero_optimizer_f(ck):
    for st in ck['optimizer_f']['state'].values():
        for k, v in st.items():
            if torch.is_tensor(v):
                st[k] = torch.zeros_like(v)


def _reset_scheduler_f(ck):
    ck['lr_scheduler_f']['last_epoch'] = 0
    ck['lr_scheduler_f']['_step_count'] = 1


def _spoil_running_var(ck):
    k = next(k for k in ck['model'] if k.endswith('running_var'))
    ck['model'][k] = torch.ones_like(ck['model'][k])


def _drop(key):
    return lambda ck: ck.pop(key)


DOCTORS = {
    'none': lambda ck: None,                                   # the control: the forget child must then reproduce the full run
    'optimizer_f': _zero_optimizer_f,                          # every state tensor of optimizer_f zeroed
    'optimizer_h_adv3': _drop('optimizer_h_adv3'),             # (the loader then leaves its scheduler alone as well)
    'lr_scheduler_f': _reset_scheduler_f,                      # the schedule of optimizer_f starts over
    'gl_iter_num': _drop('gl_iter_num'),
    'model_ema.pth': lambda ck: None,                          # the file beside the checkpoint is left out (keeps_ema_file)
    'ema_state': _drop('ema_state'),
    'proto_state': _drop('proto_state'),
    'mixup_state': _drop('mixup_state'),
    'running_var': _spoil_running_var,                         # the first BatchNorm running_var of the model set to 1
    'fp8_state': _drop('fp8_state'),
}
PIECES = {
    'all-bf16-adamw': ('optimizer_f', 'optimizer_h_adv3', 'lr_scheduler_f', 'gl_iter_num', 'model_ema.pth', 'ema_state', 'proto_state',
                       'mixup_state', 'running_var'),
    'plain-fp8': ('fp8_state', 'optimizer_f'),
}


def doctor(piece, ck):
    """A deep copy of the checkpoint dict `ck` with `piece` forgotten; every other key is untouched."""
    out = copy.deepcopy(ck)
    DOCTORS[piece](out)
    return out


def keeps_ema_file(piece):
    return piece != 'model_ema.pth'
