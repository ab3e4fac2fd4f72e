"""tests/guarded.py catches what it claims to, on CPU tensors.  The "kernels" are a few lines of torch written here -- each one
makes a mistake a tiled kernel can make (a store outside its result, a launch or a split that writes nothing, a read past an
operand that a zero hides) -- and every case must end in a GuardError from check() or in a failed comparison of the caller."""
import types

import pytest
import torch

import guarded as G


@pytest.fixture(autouse=True)
def clean():
    G.reset()
    yield
    G.reset()


def _fake_ops():
    """Stands for mi355.ops: a module-like object whose `workspace` the wrappers call by name."""
    ops = types.SimpleNamespace()
    ops.real_workspace = ops.workspace = lambda nbytes, device, tag='main': torch.zeros(max(int(nbytes), 64 << 10), dtype=torch.uint8)
    return ops


def _raw_of(v):
    """The whole guarded buffer behind a view (flanks included) as bytes, and the payload's first byte in it."""
    b = G._buf_of(v)
    return b.raw, b.start, b.n


ROWS, C = 5, 24          # fp32 [rows][C] outputs: pitch 96 bytes


def _out(ops, label='kernel'):
    with G.window(ops, label):
        return torch.empty((ROWS, C), dtype=torch.float32)


# ------------------------------------------------------------------------------------------ writes outside the result
@pytest.mark.parametrize('where', ['one element before', 'one element after', 'one row after', 'last flank byte'])
def test_a_store_outside_the_payload_fails_the_check(where):
    ops = _fake_ops()
    y = _out(ops, 'store ' + where)
    raw, start, n = _raw_of(y)
    assert n == ROWS * C * 4
    y.fill_(1.0)                                   # the launch proper: all of the payload
    assert bool((raw[:start] == 0xFF).all()) and bool((raw[start + n:] == 0xFF).all())
    one = torch.tensor([0, 0, 128, 63], dtype=torch.uint8)          # the bytes of 1.0f
    if where == 'one element before':
        raw[start - 4:start] = one
        expect = 'front flank changed, bytes -4 .. -1 '
    elif where == 'one element after':
        raw[start + n:start + n + 4] = one
        expect = 'back flank changed, bytes %d .. %d ' % (n, n + 3)
    elif where == 'one row after':
        raw[start + n:start + n + C * 4] = 0
        expect = 'back flank changed, bytes %d .. %d ' % (n, n + C * 4 - 1)
    else:
        raw[-1] = 0
        expect = 'back flank changed, bytes %d .. %d ' % (raw.numel() - 1 - start, raw.numel() - 1 - start)
    with pytest.raises(G.GuardError) as e:
        G.check()
    text = str(e.value)
    assert expect in text and 'store ' + where in text and 'empty(%d, %d)' % (ROWS, C) in text, text
    G.check()                                      # reported once: the buffers of that call are gone


def test_an_intact_call_passes_and_flanks_hold_a_row_tile():
    ops = _fake_ops()
    y = _out(ops)
    raw, start, n = _raw_of(y)
    y.fill_(2.0)
    G.check()
    assert start >= max(G.FLOOR, G.ROWS * C * 4) and raw.numel() - start - n >= max(G.FLOOR, G.ROWS * C * 4)
    wide = G.place(torch.zeros(2, 4096, 3, 3).contiguous(memory_format=torch.channels_last), 'wide')        # pitch 16 KiB
    raw, start, n = _raw_of(wide)
    assert start >= 256 * 4096 * 4 and raw.numel() - start - n >= 256 * 4096 * 4
    assert G.flank_bytes(16384, 65 << 20, lean=True) == G.FLOOR + 256 * 16384 and G.flank_bytes(8, 65 << 20, lean=True) == G.FLOOR + 2048
    assert G.flank_bytes(8) == G.FLOOR and G.flank_bytes(100) == 25600


def test_a_workspace_write_one_byte_past_need_fails_the_check():
    ops = _fake_ops()
    for need in (4 * 24 * 4, 1001):                # a multiple of 16, and one the view rounds up to 1008
        with G.window(ops, 'slabs'):
            ws = ops.workspace(need, torch.device('cpu'))
            assert ws.numel() == (need + 15) // 16 * 16 and ws.dtype == torch.uint8 and ws.data_ptr() % 256 == G.START
            assert int((ws[:need] == 0xFF).sum()) == need
        raw, start, n = _raw_of(ws)
        assert n == need
        raw[start:start + need] = 0                # the slabs proper
        G.check()
    # (above: intact.)  Now the byte behind `need`
    with G.window(ops, 'slabs+1'):
        ws = ops.workspace(1001, torch.device('cpu'))
    raw, start, n = _raw_of(ws)
    raw[start + 1001] = 0
    with pytest.raises(G.GuardError) as e:
        G.check()
    assert 'workspace(1001)' in str(e.value) and 'back flank changed, bytes 1001 .. 1001 ' in str(e.value) and 'slabs+1' in str(e.value)


# ------------------------------------------------------------------------------------------ launches that write nothing
def test_a_launch_that_writes_nothing_compares_unequal_even_after_an_identical_call_was_freed():
    ops = _fake_ops()
    ref = torch.arange(ROWS * C, dtype=torch.float32).view(ROWS, C)

    def wrapper(store):
        y = torch.empty((ROWS, C), dtype=torch.float32)
        if store:
            y.copy_(ref)
        return y

    # without the window the allocator hands the freed block back with the old, correct bits in it (when it does, the comparison
    # cannot tell; whether it does is the allocator's business and not asserted here)
    with G.window(ops, 'first'):
        y = wrapper(True)
    G.check()
    assert torch.equal(y, ref) and G.unwritten(y) == 0
    del y
    with G.window(ops, 'second, stores nothing'):
        y = wrapper(False)
    G.check()
    assert not torch.equal(y, ref)
    assert bool(torch.isnan(y).all())                              # NaN, not the old bits
    assert G.unwritten(y) == ROWS * C * 4
    y[0].copy_(ref[0])                                             # ... and a launch that skipped all tiles but one
    assert G.unwritten(y) == (ROWS - 1) * C * 4 and not torch.equal(y, ref)


def test_a_slab_nobody_wrote_poisons_the_reduction():
    ops = _fake_ops()
    S, n = 4, 48
    parts = torch.arange(S * n, dtype=torch.float32).view(S, n)

    def wgrad(skip):
        ws = ops.workspace(S * n * 4, torch.device('cpu'))[:S * n * 4].view(torch.float32).view(S, n)
        for s in range(S):
            if s != skip:
                ws[s] = parts[s]                   # block s of the split writes its slab
        return ws.sum(0)                           # the slab reduction

    with G.window(ops, 'wgrad'):
        good = wgrad(None)
    with G.window(ops, 'wgrad, slab 2 missing'):
        bad = wgrad(2)
    G.check()
    assert torch.equal(good, parts.sum(0))
    assert bool(torch.isnan(bad).all())
    # the shared grow-only workspace would have hidden it: zeros (or the previous call's slab) add up to a plausible answer
    ops.workspace = ops.real_workspace
    assert not bool(torch.isnan(wgrad(2)).any())


# ------------------------------------------------------------------------------------------ reads outside an operand
def test_an_operand_read_past_its_end_times_zero_is_nan():
    x = torch.arange(1.0, 1.0 + ROWS * C).view(ROWS, C)
    xg = G.place(x, 'x')
    assert torch.equal(xg, x)
    # a K tail: the kernel reads C + 1 elements of the last row and multiplies the extra one by a zero weight
    w = torch.cat([torch.ones(C), torch.zeros(1)])
    tail = lambda t: t.as_strided((C + 1,), (1,), t.storage_offset() + (ROWS - 1) * C)
    assert torch.equal(tail(xg)[:C], x[ROWS - 1]) and bool(torch.isnan((tail(xg) * w).sum()))          # NaN: the flank is not a zero
    roomy = torch.zeros(ROWS + 1, C)                                           # the same read with a harmless neighbour: right today
    roomy[:ROWS] = x
    assert float((tail(roomy[:ROWS]) * w).sum()) == float(x[ROWS - 1].sum())
    head = xg.as_strided((C + 1,), (1,), xg.storage_offset() - 1)              # ... and one element in FRONT of the payload
    assert bool(torch.isnan((head * torch.cat([torch.zeros(1), torch.ones(C)])).sum()))
    G.check()
    for dt in (torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2):        # the same fill is a NaN in every element type in use
        g = G.place(torch.zeros(4, 32).to(dt), str(dt))
        raw, start, n = _raw_of(g)
        assert bool(torch.isnan(raw[start + n:start + n + 8].view(dt).float()).all())
    e8 = G.place(torch.full((64,), 127, dtype=torch.uint8), 'E8M0 scales')    # 2^0 each
    raw, start, n = _raw_of(e8)
    assert int(raw[start + n]) == 0xFF and int(raw[start - 1]) == 0xFF        # the NaN code of E8M0 on either side


# ------------------------------------------------------------------------------------------ the window and the views
def test_window_restores_what_it_replaced_after_an_exception():
    ops = _fake_ops()
    before = (torch.empty, torch.empty_strided, ops.workspace)
    with pytest.raises(RuntimeError):
        with G.window(ops, 'raises'):
            assert torch.empty is not before[0] and torch.empty_strided is not before[1] and ops.workspace is not before[2]
            raise RuntimeError('the wrapper refused')
    assert (torch.empty, torch.empty_strided, ops.workspace) == before
    with G.window(ops, 'outer'):
        with pytest.raises(ValueError):
            with G.window(ops, 'inner'):
                raise ValueError()
        assert torch.empty is not before[0]                # the outer window is still open
    assert (torch.empty, torch.empty_strided, ops.workspace) == before
    t = torch.empty(3, 5)                                  # outside a window: untouched allocations
    assert G._buf_of(t) is None


def _like_sources():
    base = torch.arange(64.0)
    return {'channels_last': torch.arange(2.0 * 8 * 3 * 5).view(2, 8, 3, 5).contiguous(memory_format=torch.channels_last),
            'offset': base[4:52].view(4, 12),                      # a dense view that starts 16 bytes into its storage
            'zero-size': torch.zeros(3, 0, 7)}


@pytest.mark.parametrize('what', ['channels_last', 'offset', 'zero-size'])
def test_empty_like_gives_a_guarded_view_of_the_same_shape_strides_and_dtype(what):
    ops = _fake_ops()
    t = _like_sources()[what]
    with G.window(ops, 'like ' + what):
        a = torch.empty_like(t)
        h = torch.empty_like(t, dtype=torch.bfloat16)
        c = torch.empty_like(t, device='cpu')
        m = torch.empty_like(t, device='meta')                     # another device type: the real function
        k = torch.empty_like(t, memory_format=torch.contiguous_format)    # not modelled: the real function
    assert m.device.type == 'meta' and tuple(m.shape) == tuple(t.shape)
    assert tuple(k.shape) == tuple(t.shape) and k.is_contiguous() and (t.numel() == 0 or G._buf_of(k) is None)
    for v, dt in ((a, torch.float32), (h, torch.bfloat16), (c, torch.float32)):
        assert tuple(v.shape) == tuple(t.shape) and v.stride() == t.stride() and v.dtype == dt and v.device == t.device
        if t.numel():
            assert v.data_ptr() % 256 == G.START and G._buf_of(v) is not None
            assert G.unwritten(v) == t.numel() * v.element_size()                  # nothing but the fill in it
            assert G._buf_of(v).n == t.numel() * v.element_size()
    if what == 'channels_last':
        assert a.permute(0, 2, 3, 1).is_contiguous()
    G.check()
    if not t.numel():
        return
    # an emulated one-element overrun behind the payload, then one in front of it
    one = torch.tensor([0, 0, 128, 63], dtype=torch.uint8)          # the bytes of 1.0f
    for side in ('behind', 'in front'):
        with G.window(ops, 'like %s, store %s' % (what, side)):
            y = torch.empty_like(t)
        raw, start, n = _raw_of(y)
        assert n == t.numel() * 4
        y.copy_(t)
        if side == 'behind':
            raw[start + n:start + n + 4] = one
            expect = 'back flank changed, bytes %d .. %d ' % (n, n + 3)
        else:
            raw[start - 4:start] = one
            expect = 'front flank changed, bytes -4 .. -1 '
        with pytest.raises(G.GuardError) as e:
            G.check()
        text = str(e.value)
        assert expect in text and 'empty_like%s' % (tuple(t.shape),) in text and 'store ' + side in text, text
        assert torch.equal(y, t)
        G.check()


def test_empty_like_passes_through_what_it_does_not_model_and_is_restored_after_an_exception():
    ops = _fake_ops()
    real = torch.empty_like
    gapped = torch.zeros(4, 16)[:, ::2]                             # a view with holes: torch chooses new strides for it
    with pytest.raises(RuntimeError):
        with G.window(ops, 'raises'):
            assert torch.empty_like is not real
            g = torch.empty_like(gapped)
            assert tuple(g.shape) == (4, 8) and G._buf_of(g) is None and g.stride() == real(gapped).stride()
            r = torch.empty_like(torch.zeros(3), requires_grad=True)
            assert r.requires_grad and G._buf_of(r) is not None
            raise RuntimeError('the wrapper refused')
    assert torch.empty_like is real
    with G.window(ops, 'outer'):
        with pytest.raises(ValueError):
            with G.window(ops, 'inner'):
                raise ValueError()
        assert torch.empty_like is not real                         # the outer window is still open
    assert torch.empty_like is real
    assert G._buf_of(torch.empty_like(torch.zeros(3, 5))) is None   # outside a window: untouched allocations


def test_views_keep_shape_strides_dtype_layout_and_start():
    ops = _fake_ops()
    is_nhwc = lambda x: x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous()
    for dt in (torch.float32, torch.bfloat16, torch.uint8):
        x = torch.arange(2 * 8 * 3 * 5).view(2, 8, 3, 5).to(dt).contiguous(memory_format=torch.channels_last)
        g = G.place(x, 'x')
        assert g.shape == x.shape and g.stride() == x.stride() and g.dtype == dt and is_nhwc(g) and torch.equal(g, x)
        assert g.data_ptr() % 256 == G.START
        g8 = G.place(x, 'x', start=8)
        assert g8.data_ptr() % 256 == 8 and torch.equal(g8, x)
        with G.window(ops, 'outputs'):
            a = torch.empty((2, 3, 5, 8), dtype=dt).permute(0, 3, 1, 2)             # ops.nhwc_empty
            b = torch.empty_strided(x.shape, x.stride(), dtype=dt)                 # the MX copy of an output
            c = torch.empty(40, dtype=dt)                                          # mean, invstd, coeff, a stats buffer
            d = torch.empty(2, 3, dtype=dt)
            e = torch.empty((2, 8, 3, 5), dtype=dt, memory_format=torch.channels_last)
        for t, shape, stride in ((a, x.shape, x.stride()), (b, x.shape, x.stride()), (c, (40,), (1,)), (d, (2, 3), (3, 1)), (e, x.shape, x.stride())):
            assert tuple(t.shape) == tuple(shape) and t.stride() == tuple(stride) and t.dtype == dt
            assert t.data_ptr() % 256 == G.START and G.unwritten(t) == t.numel() * t.element_size()
        assert is_nhwc(a) and is_nhwc(b) and is_nhwc(e)
        a.copy_(x)
        assert G.unwritten(a) == 0 and torch.equal(a, x)
    G.check()
    # a placed buffer stays under watch while its view lives: a later stray store in front of it is still found
    keep = G.place(torch.zeros(4, 16), 'kept operand')
    G.check()
    raw, start, n = _raw_of(keep)
    raw[start - 1] = 0
    with pytest.raises(G.GuardError) as e:
        G.check('a later call')
    assert 'kept operand' in str(e.value) and 'front flank changed, bytes -1 .. -1 ' in str(e.value) and 'a later call' in str(e.value)
