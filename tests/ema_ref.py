"""The EMA teacher update restated (reference uda/model/loss.py:229-261: update_ema_variables5 / 3 / 2):

    v_ema = v_ema * m + (1. - m) * v_main      for every floating-point tensor of the two state dicts
    v_ema = v_main                             for num_batches_tracked

in numpy fp32: a = fl(e * k), b = fl(p * c), e' = fl(a + b) with k = float32(m), c = float32(1.0 - m) (the subtraction in
double).  numpy rounds each fp32 operation on its own, so there is nothing to contract."""
import numpy as np


def warmup_momentum(step, decay):
    """update_ema_variables2: the true average until the exponential one is more correct (step counted from 0)."""
    return min(1 - 1 / (step + 1), decay)


def ema_array(e, p, m):
    e, p = np.asarray(e), np.asarray(p)
    assert e.dtype == np.float32 and p.dtype == np.float32 and e.shape == p.shape
    k, c = np.float32(m), np.float32(1.0 - m)
    a = (e * k).astype(np.float32)
    b = (p * c).astype(np.float32)
    return (a + b).astype(np.float32)


def ema_state(ema, main, m):
    """ema, main: dicts name -> array in state_dict() order; returns the teacher's next state."""
    assert list(ema) == list(main), 'state_dict names are different!'
    out = {}
    for k in ema:
        assert np.shape(ema[k]) == np.shape(main[k]), 'state_dict shapes are different!'
        out[k] = np.array(main[k], copy=True) if 'num_batches_tracked' in k else ema_array(ema[k], main[k], m)
    return out
