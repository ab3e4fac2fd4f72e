"""numpy restatement of the reference's cross-domain mixup (uda/model/loss.py:13-24) with torch's float32 roundings:

    om  = fl(1 - lam)                                 one rounding per sample
    out = fl(fl(a * lam) + fl(b * om))                two products and a sum, each rounded on its own

numpy's float32 arithmetic rounds every operation once (no contraction), so the plain expression is the three-rounding form.
`lam` (B,) is already max(mix, 1 - mix)."""
import numpy as np


def blend(a, b, lam):
    """a * lam + b * (1 - lam), lam per sample (axis 0), all float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    lam = np.asarray(lam, np.float32).reshape((-1,) + (1,) * (a.ndim - 1))
    om = (np.float32(1.0) - lam).astype(np.float32)
    p, q = (a * lam).astype(np.float32), (b * om).astype(np.float32)
    return (p + q).astype(np.float32)


def mixup_pairs(x_s, hm_s, w_s, x_t, hm_t, w_t, lam):
    """(x_mix (2B, ...), hm_mix (2B, ...), w_mix (2B, ...)) as mi355_mixup_pairs writes them."""
    w = np.maximum(np.asarray(w_s, np.float32), np.asarray(w_t, np.float32))
    return (np.concatenate([blend(x_s, x_t, lam), blend(x_t, x_s, lam)]),
            np.concatenate([blend(hm_s, hm_t, lam), blend(hm_t, hm_s, lam)]), np.concatenate([w, w]))


def mixup(x_s, hm_s, w_s, x_t, hm_t, w_t, lam):
    """The reference's 6-tuple."""
    x, hm, w = mixup_pairs(x_s, hm_s, w_s, x_t, hm_t, w_t, lam)
    B = len(np.asarray(lam).reshape(-1))
    return x[:B], hm[:B], w[:B], x[B:], hm[B:], w[:B]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
