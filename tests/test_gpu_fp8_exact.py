"""The per-tensor fp8 front end byte for byte: quantize_fp8_kernel, fp8_update_scale_kernel, pack_weights_fp8_kernel and
pack_weights_fp8_batched_kernel (csrc/igemm_fp8.hip, csrc/fp8_common.h) with mi355.fp8_alloc_state / fp8_tick and
nn.repack_params_fp8 above them, against the numpy reference tests/fp8_ref.py.  Every comparison is equality of bytes or of
32-bit words; the only latitude is the sign bit of a NaN element.  tests/test_fp8_ref_cpu.py shows that the input sets used
here tell the reference from wrong roundings, amax rules, scale rules and layouts."""
import numpy as np
import pytest
import torch

import fp8_ref as R

pytestmark = pytest.mark.gpu

FMTS = [R.E4M3, R.E5M2]
SENT = 0xA5                                      # guard byte
SENT_W = 0x4b1dbeef                              # guard word (a finite float, 10337007.0)
GUARD = 64


def _rt():
    import mi355
    mi355.load()
    from mi355 import ops
    return mi355, ops


def _words(t):
    """a float32 / uint8 device tensor as numpy uint32 words"""
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).copy()


def _dev_state(words, gpu):
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy()).to(gpu).view(torch.float32)


def _dev(x, gpu, dtype=torch.float32):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(gpu).to(dtype)


def _assert_bytes(got, ref, src_scaled, fmt, what):
    """bytes equal, except that a NaN element only has to stay NaN (its sign bit is not pinned)"""
    got = got.detach().cpu().numpy().reshape(-1)
    nan = np.isnan(src_scaled).reshape(-1)
    bad = np.nonzero((got != ref) & ~nan)[0]
    assert bad.size == 0, '%s: %d bytes differ, first at %s: got %s, reference %s' % (
        what, bad.size, bad[:6].tolist(), got[bad[:6]].tolist(), ref[bad[:6]].tolist())
    assert np.isnan(R.decode_table(fmt)[got[nan]]).all(), '%s: a NaN element lost its NaN' % what


def _assert_words(got, ref, what):
    got, ref = np.asarray(got, dtype=np.uint32), np.asarray(ref, dtype=np.uint32)
    assert np.array_equal(got, ref), '%s: got %s (%s), reference %s (%s)' % (
        what, [hex(v) for v in got.tolist()], R.from_bits(got).tolist(), [hex(v) for v in ref.tolist()], R.from_bits(ref).tolist())


def _quantize_raw(mi355, x, st, fmt, write, room):
    """mi355_fp8_quantize into a buffer of `room` bytes + a guard; returns the whole buffer"""
    buf = torch.full((room + GUARD,), SENT, dtype=torch.uint8, device=x.device)
    mi355.call('mi355_fp8_quantize', x.data_ptr(), buf.data_ptr(), st.data_ptr(), x.numel(), mi355.dtype_code(x.dtype), int(fmt),
               int(write), mi355.stream_ptr())
    torch.cuda.synchronize()
    return buf


# ---------------------------------------------------------------- a. every bf16 value
@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('finite_only', [False, True])
def test_every_bf16_value_at_delayed_scales(gpu, fmt, finite_only):
    """All 65 536 bf16 patterns (then with the non-finite ones zeroed) at the scales 2^k written straight into the state:
    bytes, the copy's record, the recorded amax (Inf, then the largest finite bf16) and the update that must keep the scale.
    The full set holds signalling NaN patterns right behind each Inf: a running max that lets one of them through forgets
    the Inf (the kernel's fmaxf did, and recorded 0x7f7f0000)."""
    mi355, ops = _rt()
    x = R.bf16_patterns(finite_only)
    # from the bits, not through a cast, so that every NaN pattern arrives as it is
    xd = torch.from_numpy((R.bits(x) >> 16).astype(np.uint16).view(np.int16)).to(gpu).view(torch.bfloat16)
    for k in R.SCALE_KS:
        st0 = R.make_state(R.pow2(k), R.pow2(-k), 0, SENT_W)
        st = _dev_state(st0, gpu)
        q = ops.fp8_quantize(xd, st, fmt)
        torch.cuda.synchronize()
        qr, rec, st1 = R.quantize(x, st0, fmt, 2)
        what = 'fmt %d scale 2^%d' % (fmt, k)
        _assert_bytes(q, qr, R.scaled(x, st0), fmt, what)
        _assert_words(_words(q._mi_rec), rec, what + ' record')
        _assert_words(_words(st), st1, what + ' state')
        assert st1[2] == (0x7f7f0000 if finite_only else R.INF_BITS) and np.array_equal(st1[:2], st0[:2])
        # the recorded amax is >= 3.0e38: the update keeps the scale and clears the amax
        ops.fp8_update_scale(st, 1, fmt)
        torch.cuda.synchronize()
        _assert_words(_words(st), [st0[0], st0[1], 0, SENT_W], what + ' state after the update')


# ---------------------------------------------------------------- b. fp32 ties
@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('k', R.TIE_KS)
def test_fp32_ties_saturation_and_specials(gpu, fmt, k):
    mi355, ops = _rt()
    x = R.tie_set(fmt, k)
    st0 = R.make_state(R.pow2(k), R.pow2(-k), 0, SENT_W)
    st = _dev_state(st0, gpu)
    q = ops.fp8_quantize(_dev(x, gpu), st, fmt)
    torch.cuda.synchronize()
    qr, rec, st1 = R.quantize(x, st0, fmt, 2)
    _assert_bytes(q, qr, R.scaled(x, st0), fmt, 'ties')
    _assert_words(_words(q._mi_rec), rec, 'record')
    _assert_words(_words(st), st1, 'state')
    assert st1[2] == R.INF_BITS


# ---------------------------------------------------------------- c. loop and reduction geometry
_GEOM = {}


def _geometry(n, fmt):
    """(base tensor, its reference bytes at scale 1): computed once per length"""
    if (n, fmt) not in _GEOM:
        base = R.geometry_base(n, fmt)
        base.setflags(write=False)
        qr = R.encode(base, fmt)
        qr.setflags(write=False)
        _GEOM[(n, fmt)] = (base, qr)
    return _GEOM[(n, fmt)]


@pytest.mark.parametrize('n', R.GEOMETRY_NS)
@pytest.mark.parametrize('fmt', FMTS)
def test_loop_and_reduction_geometry(gpu, fmt, n):
    mi355, ops = _rt()
    base, qbase = _geometry(n, fmt)
    st0 = R.make_state(1.0, 1.0, 0, SENT_W)
    amax_code = R.encode(-R.GEOMETRY_AMAX, fmt)
    xd = _dev(base, gpu)
    for p in R.geometry_positions(n):
        xd[p] = -float(R.GEOMETRY_AMAX)
        st = _dev_state(st0, gpu)
        q = ops.fp8_quantize(xd, st, fmt)
        torch.cuda.synchronize()
        qr = qbase.copy()
        qr[p] = amax_code
        _assert_bytes(q, qr, base, fmt, 'n %d, amax at %d' % (n, p))
        _assert_words(_words(q._mi_rec), [st0[0], st0[1], 0, 0], 'record')
        _assert_words(_words(st), [st0[0], st0[1], R.bits(R.GEOMETRY_AMAX), SENT_W], 'n %d, amax at %d: state' % (n, p))
        # the amax-only pass finds it as well
        st = _dev_state(st0, gpu)
        ops.fp8_amax(xd, st)
        torch.cuda.synchronize()
        _assert_words(_words(st), [st0[0], st0[1], R.bits(R.GEOMETRY_AMAX), SENT_W], 'n %d, amax at %d: amax-only state' % (n, p))
        xd[p] = float(base[p])


# ---------------------------------------------------------------- d. the `seen` shortcut and the write modes
@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('src', ['f32', 'bf16'])
def test_seen_shortcut_and_write_modes(gpu, fmt, src):
    mi355, ops = _rt()
    n = R.GEOMETRY_NS[1]
    base, _ = _geometry(n, fmt)
    x = base.copy()
    x[R.geometry_positions(n)[-1]] = -R.GEOMETRY_AMAX
    xd = _dev(x, gpu, torch.bfloat16 if src == 'bf16' else torch.float32)
    x = xd.float().cpu().numpy()               # (bf16: the cast rounds the ties' fp32 neighbours; the reference reads what the device holds)
    assert float(np.abs(x).max()) == float(R.GEOMETRY_AMAX) and int((np.abs(x) == R.GEOMETRY_AMAX).sum()) == 1
    ab = int(R.bits(R.GEOMETRY_AMAX))
    for pre in (ab - 1, ab, ab + 1):                               # below, equal, above: raised, kept, kept
        st0 = R.make_state(2.0, 0.5, pre, SENT_W)
        for write in (0, 1, 2):
            st = _dev_state(st0, gpu)
            qr, rec, st1 = R.quantize(x, st0, fmt, write)
            assert st1[2] == max(pre, ab)
            what = 'write %d, state[2] preloaded with %#x' % (write, pre)
            if write == 0:
                ops.fp8_amax(xd, st)
                torch.cuda.synchronize()
            else:
                room = n + (16 if write == 2 else 0)
                buf = _quantize_raw(mi355, xd, st, fmt, write, room)
                _assert_bytes(buf[:n], qr, R.scaled(x, st0), fmt, what)
                if write == 2:
                    _assert_words(_words(buf[n:n + 16]), rec, what + ': record')
                assert bool((buf[room:] == SENT).all()), what + ': bytes behind the copy were written'
            _assert_words(_words(st), st1, what + ': state')


# ---------------------------------------------------------------- e. fp8_update_scale
def _scale_buffer(pts, n, stride, off):
    """(n + 2) slots of `stride` words: slot i < n holds point (i + off) mod len; every other word is a sentinel"""
    buf = (SENT_W + np.arange((n + 2) * stride, dtype=np.uint32)).astype(np.uint32)
    for i in range(n):
        ab, sc, de = pts[(i + off) % len(pts)]
        buf[i * stride: i * stride + 3] = [R.bits(np.float32(sc)), R.bits(np.float32(de)), ab]
    return buf


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('margin', [0, 1, 8])
def test_update_scale_follows_the_exact_rule(gpu, fmt, margin):
    """n = 1, 64, 65, 130 states (64 threads per block) at strides 4 and 6 with sentinels around words 0-2, over the amax
    points of fp8_ref.scale_points.  The float form of the rule failed here for every amax 2^margin below fmt_max / FLT_MAX (scale Inf,
    descale 0) and, with a margin, for the amax just below 3.0e38 (scale 0, descale Inf); at fmt_max * 2^j and its neighbours
    the device's log2f / exp2f agreed with the exact rule."""
    mi355, ops = _rt()
    pts = R.scale_points(fmt)
    bad = []
    for stride in (4, 6):
        for n, off in ((1, 0), (1, 40), (64, 0), (65, 60), (130, 0)):
            before = _scale_buffer(pts, n, stride, off)
            dev = _dev_state(before, gpu)
            mi355.call('mi355_fp8_update_scale', dev.data_ptr(), n, stride, int(fmt), margin, mi355.stream_ptr())
            torch.cuda.synchronize()
            got, ref = _words(dev), before.copy()
            for i in range(n):
                s = R.tick(before[i * stride: i * stride + 4], fmt, margin)
                assert R.from_bits(s[1]) == np.float32(1) / R.from_bits(s[0])
                ref[i * stride: i * stride + 3] = s[:3]
            # word 3 (and 4, 5) of every slot, and the slots from n on, are the reference's untouched sentinels
            for j in np.nonzero(got != ref)[0].tolist():
                i, wd = divmod(j, stride)
                bad.append('stride %d n %d slot %d word %d (amax %#x = %r): got %#x (%r), reference %#x (%r)' % (
                    stride, n, i, wd, before[i * stride + 2] if i < n else 0, float(R.from_bits(before[i * stride + 2])) if i < n else None,
                    got[j], float(R.from_bits(got[j])), ref[j], float(R.from_bits(ref[j]))))
    assert not bad, '%d words differ:\n%s' % (len(bad), '\n'.join(bad[:12]))


# ---------------------------------------------------------------- f. pools
def test_pools_tick_each_slot_by_its_own_format(gpu):
    """Three e4m3 and two e5m2 slots of the process-wide pools through mi355.fp8_tick: each follows its own format's rule and
    the slot behind the last used one of each pool stays as it was.  Only the slots allocated here are asserted on."""
    mi355, ops = _rt()
    pts = R.pool_points()
    slots = [(mi355.fp8_alloc_state(gpu, fmt), fmt) for fmt, _, _, _ in pts]
    before = []
    for (st, fmt), (_, a, sc, de) in zip(slots, pts):
        w = R.make_state(sc, de, int(R.bits(a)), SENT_W)
        st.copy_(_dev_state(w, gpu))
        before.append(w)
    dev = gpu.index if gpu.index is not None else torch.cuda.current_device()
    pools = [mi355._fp8_pools[(dev, fmt)] for fmt in FMTS]
    after_last = [_words(p['buf'][4 * p['used']: 4 * p['used'] + 4]) for p in pools]
    mi355.fp8_tick()
    torch.cuda.synchronize()
    for i, ((st, fmt), w) in enumerate(zip(slots, before)):
        _assert_words(_words(st), R.tick(w, fmt, 0), 'slot %d (format %d)' % (i, fmt))
    for p, w in zip(pools, after_last):
        _assert_words(_words(p['buf'][4 * p['used']: 4 * p['used'] + 4]), w, 'the slot behind the last used one')
    for st, _ in slots:            # leave them as a later user expects to find fresh ones
        st.zero_()


# ---------------------------------------------------------------- g. weight packs
def _pack_on_device(ops, w, st0, O, T, I, jit, gpu):
    """one single-launch pack into guarded buffers -> (wf, wt, state words)"""
    n = O * T * I
    wf, wt = (torch.full((n + GUARD,), SENT, dtype=torch.uint8, device=gpu) for _ in range(2))
    st = _dev_state(st0, gpu)
    ops.pack_weights_fp8(_dev(w, gpu), O, T, I, st, wf, wt, jit=jit)
    torch.cuda.synchronize()
    for b, name in ((wf, 'wf'), (wt, 'wt')):
        assert bool((b[n:] == SENT).all()), 'bytes behind %s were written' % name
    return wf[:n], wt[:n], _words(st)


def _check_pack(got, w, st0, O, T, I, margin, what):
    wf, wt, st = got
    rf, rt_, rs = R.pack(w, st0, O, T, I, margin)
    src = R.scaled(w, rs).reshape(O, T, I)
    _assert_bytes(wf, rf, src, R.E4M3, what + ': wf')
    _assert_bytes(wt, rt_, src.transpose(2, 1, 0), R.E4M3, what + ': wt')
    _assert_words(st, rs, what + ': state')
    assert rs[3] == rs[1]
    if margin < 0:
        assert np.array_equal(rs[:2], st0[:2])
    return rs


@pytest.mark.parametrize('shape', R.PACK_SHAPES)
def test_weight_pack_bytes_and_state(gpu, shape):
    mi355, ops = _rt()
    O, T, I = shape
    for variant in ('amax_last', 'zero', 'nan'):
        w = R.pack_weights(O, T, I, variant)
        st0 = R.make_state(0.0, 0.0, 0, SENT_W)
        rs = _check_pack(_pack_on_device(ops, w, st0, O, T, I, True, gpu), w, st0, O, T, I, 0, '%s, just in time' % variant)
        assert R.from_bits(rs[0]) == (1.0 if variant == 'zero' else R.PACK_SCALE)
        ab = int(R.bits(R.PACK_AMAX))
        for scale in (R.PACK_SCALE, 2 * R.PACK_SCALE):              # (the second saturates the amax element)
            for pre in (ab - 1, ab + 1):
                st0 = R.make_state(scale, 1 / scale, pre, SENT_W)
                rs = _check_pack(_pack_on_device(ops, w, st0, O, T, I, False, gpu), w, st0, O, T, I, -1,
                                 '%s, delayed, scale %g, state[2] %#x' % (variant, scale, pre))
                assert rs[2] == (pre if variant == 'zero' else max(pre, ab))


# ---------------------------------------------------------------- h. batched pack
def test_batched_pack_equals_single_launches(gpu):
    mi355, ops = _rt()
    small = R.PACK_SHAPES[0]
    shapes = [small, R.PACK_SHAPES[1], small, R.PACK_SHAPES[3], small]           # single-block items first, interior and last
    variants = ['amax_last', 'nan', 'zero', 'amax_last', 'nan']
    rec = np.zeros(len(shapes), dtype=[('w', '<u8'), ('wf', '<u8'), ('wt', '<u8'), ('state', '<u8'), ('O', '<i4'), ('T', '<i4'),
                                       ('I', '<i4'), ('blk0', '<i4')])
    items, blk = [], 0
    for i, ((O, T, I), variant) in enumerate(zip(shapes, variants)):
        n = O * T * I
        w = R.pack_weights(O, T, I, variant, seed=i)
        scale = R.PACK_SCALE * 2.0 ** (i - 2)                                    # each item its own scale
        st0 = R.make_state(scale, 1 / scale, int(R.bits(np.float32(0.5 * i))), SENT_W)
        wd, st = _dev(w, gpu), _dev_state(st0, gpu)
        wf, wt = (torch.full((n + GUARD,), SENT, dtype=torch.uint8, device=gpu) for _ in range(2))
        rec[i] = (wd.data_ptr(), wf.data_ptr(), wt.data_ptr(), st.data_ptr(), O, T, I, blk)
        blk += (O // 32) * (I // 32) * T
        items.append((w, st0, wd, st, wf, wt))
    tab = torch.from_numpy(rec.view(np.uint8).copy()).to(gpu)
    ops.pack_weights_fp8_batched(tab, len(shapes), blk)
    torch.cuda.synchronize()
    for i, ((O, T, I), (w, st0, wd, st, wf, wt)) in enumerate(zip(shapes, items)):
        n = O * T * I
        what = 'item %d %s' % (i, (O, T, I))
        assert bool((wf[n:] == SENT).all()) and bool((wt[n:] == SENT).all()), what + ': bytes behind the outputs were written'
        _check_pack((wf[:n], wt[:n], _words(st)), w, st0, O, T, I, -1, what)
        sf, stt, ss = _pack_on_device(ops, w, st0, O, T, I, False, gpu)
        assert torch.equal(sf, wf[:n]) and torch.equal(stt, wt[:n]), what + ': differs from the single launch'
        _assert_words(_words(st), ss, what + ': state against the single launch')


# ---------------------------------------------------------------- i. the protocol
def test_delayed_scaling_protocol(gpu):
    """One activation state and one weight state through a just-in-time start and five delayed steps (amax x64, x1/512, all
    zero, an Inf, magnitude 1e-37), then one more quantisation with the last scale; both states are refreshed by ONE
    two-state update launch per step."""
    mi355, ops = _rt()
    n, (O, T, I) = 16 * 257, (64, 9, 96)
    xs, ws = R.protocol_tensors(n), R.protocol_tensors(O * T * I, base_amax=0.5)
    states = torch.zeros(8, dtype=torch.float32, device=gpu)
    sx, sw = states[0:4], states[4:8]
    rx, rw = R.make_state(), R.make_state()
    wf, wt = (torch.empty(O * T * I, dtype=torch.uint8, device=gpu) for _ in range(2))
    bad = []

    def check(fn, *args):
        try:
            fn(*args)
        except AssertionError as e:
            bad.append(str(e))

    for step, (x, w) in enumerate(zip(xs + [xs[0]], ws + [ws[0]])):
        xd, wd = _dev(x, gpu), _dev(w, gpu)
        first = step == 0
        if first:                                        # the just-in-time start of nn._Fp8Stream and nn._PackedFp8
            rx = R.tick(R.quantize(x, rx, R.E4M3, 0)[2], R.E4M3, 0)
        q = ops.fp8_quantize(xd, sx, R.E4M3, jit=first)
        ops.pack_weights_fp8(wd, O, T, I, sw, wf, wt, jit=first)
        torch.cuda.synchronize()
        qr, rec, rx1 = R.quantize(x, rx, R.E4M3, 2)
        rf, rt_, rw1 = R.pack(w, rw, O, T, I, 0 if first else -1)
        what = 'step %d' % step
        check(_assert_bytes, q, qr, R.scaled(x, rx), R.E4M3, what + ': activation copy')
        check(_assert_words, _words(q._mi_rec), rec, what + ': the copy\'s record')
        check(_assert_words, _words(sx), rx1, what + ': activation state')
        src = R.scaled(w, rw1).reshape(O, T, I)
        check(_assert_bytes, wf, rf, src, R.E4M3, what + ': wf')
        check(_assert_bytes, wt, rt_, src.transpose(2, 1, 0), R.E4M3, what + ': wt')
        check(_assert_words, _words(sw), rw1, what + ': weight state')
        ops.fp8_update_scale(states, 2, R.E4M3)
        torch.cuda.synchronize()
        rx, rw = R.tick(rx1, R.E4M3, 0), R.tick(rw1, R.E4M3, 0)
        check(_assert_words, _words(sx), rx, what + ': activation state after the update')
        check(_assert_words, _words(sw), rw, what + ': weight state after the update')
        if bad:                                          # from here on device and reference run on different scales
            break
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------- j. through the layers
def test_optimizer_step_repacks_with_the_scale_before_the_tick(gpu):
    mi355, ops = _rt()
    from mi355 import nn as mnn
    from mi355.optim import FusedSGD
    from seeded import fill_module_, randn
    try:
        mi355.set_compute_dtype('fp8')
        convs = [fill_module_(mnn.Conv2d(128, 128, 3, 1, 1, bias=True).to(gpu), 40 + i) for i in range(2)]
        for c in convs:
            c.train()
        opt = FusedSGD([p for c in convs for p in c.parameters()], lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
        x = randn(50, 2, 128, 8, 8).to(gpu).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        y = convs[1](convs[0](x))
        y.backward((randn(51, *y.shape) * 1e-2).to(gpu).to(torch.bfloat16).contiguous(memory_format=torch.channels_last))
        packs = [c.weight._mi_pack8[0] for c in convs]
        with torch.no_grad():                            # grow one master so that its next scale differs from the current one
            convs[0].weight.mul_(16.0)
        torch.cuda.synchronize()
        before = [_words(pk.state) for pk in packs]
        opt.step()                                       # the step, ONE batched repack, then mi355.fp8_tick
        torch.cuda.synchronize()
        for i, (c, pk, s0) in enumerate(zip(convs, packs, before)):
            O, T, I = 128, 9, 128
            w = c.weight.detach().permute(0, 2, 3, 1).contiguous().view(-1).cpu().numpy()         # the NEW master, [O][T][I]
            rf, rt_, s1 = R.pack(w, s0, O, T, I, -1)
            src = R.scaled(w, s0).reshape(O, T, I)
            _assert_bytes(pk.wf, rf, src, R.E4M3, 'conv %d: wf' % i)
            _assert_bytes(pk.wt, rt_, src.transpose(2, 1, 0), R.E4M3, 'conv %d: wt' % i)
            s2 = R.tick(s1, R.E4M3, 0)
            _assert_words(_words(pk.state), s2, 'conv %d: state after the step' % i)
            assert s2[3] == s0[1], 'the pack is read with the descale it was made with'
            assert pk.rec.data_ptr() == pk.state.data_ptr() + 8
        assert _words(packs[0].state)[1] != before[0][1], 'the grown weight\'s descale has moved'
        assert _words(packs[0].state)[3] == before[0][1]
        mi355.fp8_tick()                                 # a tick with nothing recorded keeps every scale
        torch.cuda.synchronize()
        for pk, s0 in zip(packs, before):
            assert _words(pk.state)[2] == 0 and _words(pk.state)[3] == s0[1]
    finally:
        mi355.set_compute_dtype('bf16')
