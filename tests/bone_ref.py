"""Float64 numpy restatement of mi355_softargmax_backward, mi355_bone_prior and mi355_bone_stats_update (include/mi355pose.h), in the
operation order the header gives (every sum in ascending bone / sample order), the same expressions in torch for autograd, and
the input builders and exact cases of tests/test_bone_cpu.py and tests/test_gpu_bone.py.  No GPU-only code."""
import numpy as np
import torch

HAND = tuple((0 if j % 4 == 1 else j - 1, j) for j in range(1, 21))      # uda/dataset/keypoint_dataset.py:47-57
CHAIN = ((0, 1), (1, 2), (2, 3))                                           # a 4-joint chain


def f32(x):
    """The float32 value the C ABI receives for a Python float argument."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ soft-arg-max backward
def softargmax_backward(pred, g_uv, beta, dtype=torch.float64):
    """grad [rows, H, W] of item 1: beta * p_i * ((x_i - u) g_u + (y_i - v) g_v), evaluated in `dtype` with torch expressions; a
    row whose two upstream components are exactly 0 is selected out (+0 whatever it holds)."""
    rows, H, W = pred.shape
    z = pred.to(dtype) * beta
    p = torch.softmax(z.reshape(rows, H * W), dim=1)
    i = torch.arange(H * W)
    x, y = (i % W).to(dtype), (i // W).to(dtype)
    u, v = (p * x).sum(1), (p * y).sum(1)
    g = g_uv.to(dtype)
    t = (x[None] - u[:, None]) * g[:, :1] + (y[None] - v[:, None]) * g[:, 1:]
    out = beta * p * t
    skip = (g[:, 0] == 0) & (g[:, 1] == 0)
    return torch.where(skip[:, None], torch.zeros_like(out), out).reshape(rows, H, W)


def softargmax(pred, beta, dtype=torch.float64):
    rows, H, W = pred.shape
    p = torch.softmax((pred.to(dtype) * beta).reshape(rows, H * W), dim=1)
    i = torch.arange(H * W)
    return torch.stack([(p * (i % W).to(dtype)).sum(1), (p * (i // W).to(dtype)).sum(1)], 1)


# ------------------------------------------------------------------------------------------------------- bone prior
def _sample_lengths(uv, w, bones, seen):
    """(l [E], d [E, 2], present [E] bool, n, S) of one sample, float64, S summed in ascending bone order."""
    E = len(bones)
    l, d, present = np.zeros(E), np.zeros((E, 2)), np.zeros(E, bool)
    n, S = 0, np.float64(0.0)
    for e, (p, c) in enumerate(bones):
        d[e] = uv[c].astype(np.float64) - uv[p].astype(np.float64)
        l[e] = np.sqrt(d[e, 0] * d[e, 0] + d[e, 1] * d[e, 1])
        present[e] = (w is None or (w[p] > 0 and w[c] > 0)) and (seen is None or seen[e] != 0)
        if present[e]:
            n += 1
            S = S + l[e]
    return l, d, present, n, S


def bone_prior(uv, weight, bones, mean, var, seen, margin, eps, coef):
    """(loss_rows [B] float64, g_uv [B, K, 2] float64) of item 2.  uv [B, K, 2], weight [B, K] or None, mean / var [E] are float32
    numpy arrays (the kernel's operands); margin, eps, coef the float32 values the ABI receives (coef: the kernel's, term / B)."""
    uv = np.asarray(uv, np.float32)
    B, K, _ = uv.shape
    mean, var = np.asarray(mean, np.float32).astype(np.float64), np.asarray(var, np.float32).astype(np.float64)
    margin, eps, coef = np.float64(f32(margin)), np.float64(f32(eps)), np.float64(f32(coef))
    rows, g = np.zeros(B), np.zeros((B, K, 2))
    with np.errstate(all='ignore'):
        for b in range(B):
            w = None if weight is None else np.asarray(weight, np.float32).reshape(B, K)[b]
            l, d, present, n, S = _sample_lengths(uv[b], w, bones, seen)
            if n < 2 or S == 0:
                continue
            dn = np.float64(n)
            lbar = S / dn
            q, r = np.zeros(len(bones)), np.zeros(len(bones))
            loss, Qs = np.float64(0.0), np.float64(0.0)
            for e in range(len(bones)):
                if not present[e]:
                    continue
                r[e] = l[e] / lbar
                sd = np.sqrt(var[e] + eps)
                z = (r[e] - mean[e]) / sd
                a = np.abs(z) - margin
                h = a if (a > 0 or a != a) else np.float64(0.0)
                sg = np.float64(1.0) if z > 0 else (np.float64(-1.0) if z < 0 else z)
                loss = loss + 0.5 * (h * h)
                q[e] = h * sg / (dn * sd)
                Qs = Qs + q[e] * r[e]
            rows[b] = loss / dn
            Q = Qs / dn
            for e, (p, c) in enumerate(bones):
                if not present[e] or l[e] == 0:
                    continue
                k = coef * ((q[e] - Q) / lbar) / l[e]
                t = k * d[e]
                g[b, c] += t
                g[b, p] -= t
    return rows, g


def bone_prior_torch(uv, weight, bones, mean, var, seen, margin, eps):
    """[B] loss rows of the same expression as a differentiable float64 torch graph (vectorised: its sums are in torch's order)."""
    B, K, _ = uv.shape
    p = torch.tensor([b[0] for b in bones]); c = torch.tensor([b[1] for b in bones])
    d = uv[:, c] - uv[:, p]
    l = torch.sqrt((d * d).sum(-1) + 0.0)
    on = torch.ones(B, len(bones), dtype=torch.bool) if weight is None else (weight[:, p] > 0) & (weight[:, c] > 0)
    on = on & (torch.as_tensor(seen) != 0)[None]
    n = on.sum(1)
    S = torch.where(on, l, torch.zeros_like(l)).sum(1)
    keep = (n >= 2) & (S != 0)
    nn = n.clamp(min=1).to(uv.dtype)
    lbar = torch.where(keep, S / nn, torch.ones_like(S))
    r = l / lbar[:, None]
    sd = torch.sqrt(torch.as_tensor(var, dtype=uv.dtype) + eps)
    z = (r - torch.as_tensor(mean, dtype=uv.dtype)) / sd
    h = torch.clamp(z.abs() - margin, min=0)
    per = torch.where(on, 0.5 * h * h, torch.zeros_like(h)).sum(1) / nn
    return torch.where(keep, per, torch.zeros_like(per))


# ------------------------------------------------------------------------------------------------------ statistics
def bone_stats_update(kp, weight, bones, mean, var, seen, rho):
    """-> (mean, var, seen) after item 3, float32 / int32 numpy arrays (copies); float64 arithmetic, one rounding at the store."""
    kp = np.asarray(kp, np.float32)
    B, K, _ = kp.shape
    E = len(bones)
    mean, var, seen = np.array(mean, np.float32), np.array(var, np.float32), np.array(seen, np.int32)
    rho = np.float64(f32(rho))
    ratios = [[] for _ in range(E)]
    with np.errstate(all='ignore'):
        for b in range(B):
            w = None if weight is None else np.asarray(weight, np.float32).reshape(B, K)[b]
            l, d, present, n, S = _sample_lengths(kp[b], w, bones, None)
            if n < 2 or S == 0:
                continue
            lbar = S / np.float64(n)
            for e in range(E):
                if present[e]:
                    ratios[e].append(l[e] / lbar)
        for e in range(E):
            if not ratios[e]:
                continue
            cnt = np.float64(len(ratios[e]))
            s = np.float64(0.0)
            for r in ratios[e]:
                s = s + r
            m = s / cnt
            s = np.float64(0.0)
            for r in ratios[e]:
                s = s + (r - m) * (r - m)
            v = s / cnt
            if seen[e] == 0:
                mean[e], var[e], seen[e] = np.float32(m), np.float32(v), 1
            else:
                mean[e] = np.float32((1.0 - rho) * np.float64(mean[e]) + rho * m)
                var[e] = np.float32((1.0 - rho) * np.float64(var[e]) + rho * v)
    return mean, var, seen


# ------------------------------------------------------------------------------------------------------- builders
def hands(B, K=21, seed=0, spread=12.0, centre=32.0):
    """[B, K, 2] float32 points: chains that walk outwards from a wrist with bones of varied length, in heat-map pixels."""
    rng = np.random.default_rng(8800 + 97 * B + K + seed)
    return (centre + rng.standard_normal((B, K, 2)) * spread).astype(np.float32)


def stats_for(bones, seed=0, unseen=()):
    """(mean, var, seen) as the statistics might stand after some source batches: ratios around 1, one bone unseen on request."""
    rng = np.random.default_rng(9900 + len(bones) + seed)
    E = len(bones)
    mean = (1.0 + 0.3 * rng.standard_normal(E)).astype(np.float32)
    var = (0.02 + 0.05 * rng.random(E)).astype(np.float32)
    seen = np.ones(E, np.int32)
    for e in unseen:
        seen[e] = 0
    return mean, var, seen


def weights_case(B, K, bones, case):
    """[B, K] float32 joint weights of a named case: 'all' (every joint visible), 'invisible' (some joints of weight 0),
    'onebone' (sample 0 keeps the two joints of bone 0 only: n = 1, skipped)."""
    w = np.ones((B, K), np.float32)
    if case == 'invisible':
        for b in range(B):
            if K < 8:                                # a short chain loses one end joint: two bones are left
                w[b, 0 if b % 2 == 0 else K - 1] = 0.0
            else:
                w[b, (3 * b + 2) % K] = 0.0
                w[b, (5 * b + 7) % K] = 0.0
    elif case == 'onebone':
        w[0] = 0.0
        w[0, bones[0][0]] = w[0, bones[0][1]] = 1.0
    elif case != 'all':
        raise KeyError(case)
    return w


def exact_case(name):
    """Exact cases: integer 3-4-5 bones of length 5, 5, 10, 20 on a 5-joint chain (lbar = 10, r = 0.5, 0.5, 1, 2) with mean, var +
    eps and margin powers of two, so that every z, h and the loss are exact in float32 and float64 alike: the loss is met bit for
    bit as written here.  The gradient divides by lbar = 10; every operation is a correctly rounded IEEE one in a fixed order, so
    it is met bit for bit as float32(`bone_prior`) ('inside': all zeros)."""
    bones = ((0, 1), (1, 2), (2, 3), (3, 4))
    uv = np.array([[[0, 0], [3, 4], [6, 8], [12, 16], [24, 32]]], np.float32)          # d = (3,4), (3,4), (6,8), (12,16)
    seen = np.ones(4, np.int32)
    if name == 'inside':           # mean 1, sd 1, margin 1: |z| = (0.5, 0.5, 0, 1) -> h = 0 everywhere
        mean, var, eps, margin = np.ones(4, np.float32), np.full(4, 0.75, np.float32), 0.25, 1.0
        loss = 0.0
    elif name == 'hinge':          # mean 1, sd 0.5, margin 1: z = (-1, -1, 0, 2) -> h = (0, 0, 0, 1); loss = 0.5 / 4
        mean, var, eps, margin = np.ones(4, np.float32), np.full(4, 0.125, np.float32), 0.125, 1.0
        loss = 0.125
    elif name == 'nomargin':       # margin 0, mean 0.5, sd 1: z = h = (0, 0, 0.5, 1.5); loss = (0.125 + 1.125) / 4
        mean, var, eps, margin = np.full(4, 0.5, np.float32), np.full(4, 0.5, np.float32), 0.5, 0.0
        loss = 0.3125
    else:
        raise KeyError(name)
    return dict(bones=bones, uv=uv, mean=mean, var=var, seen=seen, eps=eps, margin=margin, loss=np.float32(loss))


EXACT = ('inside', 'hinge', 'nomargin')
