"""Poisoned guard buffers around the operands, outputs and workspace of one kernel call (no GPU-only code: any device).

Fill rule.  Every byte of a guarded buffer starts as 0xFF: a NaN as fp32, bf16, e4m3, e5m2 and E8M0, an impossible window
code, and a mask byte no fp32 launch writes.  One rule covers the flanks, payload a launch failed to write and workspace a
block failed to write, for every element type.

Layout.  [front flank][payload][back flank].  A flank is at least FLOOR = 4 KiB and at least ROWS = 256 rows of the payload's
innermost pitch (the extent of its unit-stride axis times the element size: one row tile of the widest build), rounded up to
256 bytes.  A flat (1-D) payload has no row of its own: it takes its length, at most 4 KiB, as its pitch.  row_pitch(nbytes)
names the widest row the kernels of the calls that follow stride by (a test sets it once from its shape): a lower bound for the
pitch of every buffer made after it, flat ones included.  `lean=True` (window) gives payloads above LEAN_ABOVE = 64 MB the floor
plus one row tile instead; nothing uses it unless the run time demands it.

Start alignment.  The payload starts START = 16 bytes past a 256-byte boundary -- the least alignment every entry point the
guarded suites reach accepts -- not at the allocator's 256- / 512-byte boundary.  What each kernel family
assumes of an operand's first byte, read from its address arithmetic (csrc/ at this commit):

  * gather loads of the implicit GEMMs (igemm.hip gather_kernel, igemm_fp8.hip gather_fp8_kernel, register-staged builds):
    16-byte chunks through a buffer resource sized to the operand, buf_load16(rs, byte offset) (igemm_common.h); every offset
    is a whole number of chunks ((pixel * Ci + chunk) with Ci a whole number of chunks: "gather: Ci not a multiple of",
    igemm.hip dispatch), so a chunk is aligned as the base is: 16 bytes.
  * LDS-DMA ring (igemm.hip dma_tile and the 256 x 256 tiles, pgemm.hip): raw_ptr_buffer_load_lds of 16 bytes per lane at the
    same chunk offsets, the swizzle applied to the SOURCE chunk index: 16 bytes.  The LDS side is aligned by the kernels' own
    arrays (aligned(16)), not by the operand.  pgemm's addend ring: 16-byte chunks of the residual / accumulate base, its mask
    bytes as dwords (Nout % 32 == 0 is a condition of pgemm_eligible): 4 bytes; its bias as float4 at multiples of 4: 16 bytes.
  * epilogue of the gather kernels: D, the residual, the accumulate base and the BatchNorm-backward x / y as 16-byte chunks at
    (row * ldd + column), ldd a whole number of chunks ("gather: Nout not a multiple of"): 16 bytes; bias, scale, mean, invstd,
    gamma, beta and the statistics / BatchNorm-backward partials [slice][C][3 | 2] as single floats: 4 bytes; the accumulate
    mask byte by byte.  The heat-map output (NCHW fp32) float by float.
  * MX scale loads (igemm_fp8.hip): buf_load4 of one E8M0 dword per 128-channel K tile at (byte offset of the tile's first
    element) >> 5, a multiple of 4 because the contracted channels are a multiple of 128 (checked by the mx entry points):
    4 bytes; the e4m3 elements in 16-byte chunks: 16 bytes.  mi355_mx_quantize checks 16 bytes of x and q itself, and
    mi355_conv_fwd_mx_act its 8-byte rule for the MX copy (not reached by the two suites).
  * fp8 quantiser and weight packs (igemm_fp8.hip, mx_fp8.hip): x and q as uint4 per 16 elements (n % 16 == 0 checked):
    16 bytes; the packs store dwords of 4 elements at multiples of 4: 4 bytes; the 4-float record n bytes behind q.
  * weight gradients (igemm.hip wgrad_gemm / wgrad_kw / wgrad_kw2 and the grouped kernels, wgrad_fp8.hip): x and dy in 16-byte
    chunks through buffer resources sized to the operands (the transposed reads happen in LDS, on the kernels' own arrays); the
    GEMM kernels store dw or their slab float by float: 4 bytes; slab_reduce and slab_reduce_group read the slabs and read /
    write dw as float4 (slab stride and offsets whole float4s): 16 bytes of the workspace and of dw.
  * BatchNorm (bn.hip): Chunk<T>::load / store and uint4 accesses of x, dy, y, residual, dx, dres through plain pointers at
    (row * C + chunk), C a whole number of chunks (bn_check): 16 bytes; the per-channel vectors, the statistics partials and
    the workspace (partials [slice][C][3], then coeff) as floats: 4 bytes; mask bytes one by one; the fp8 side output as one
    uint4 per pair of lanes (16 e4m3, C % 16 == 0 checked): 16 bytes.  The granules of the one-launch backward live in a buffer
    of the library's own, not in an operand.  mi355_colsum and mi355_apply_relu_mask: the same 16-byte chunks.
  * max-pool, layout, space-to-depth, stem pack (pool_layout.hip): the feature maps x, y, dy, dx as Chunk<T>::load / store
    (uint4) at (pixel * C + chunk), C a whole number of chunks ("bad args (C=...)"): 16 bytes; the window codes as ONE load /
    store of CH bytes (load_bytes / store_bytes of common.h: 8 bytes in bf16, 4 in fp32) at the same element offsets: 8 bytes;
    the NCHW fp32 side of the layout kernels, the stem weights and their gradient float by float: 4 bytes.
  * pw21 (pw21.hip): the feature maps x, the residual and the output in 16-byte chunks: 16 bytes; heat maps, weights, biases,
    scale_dev, the statistics partials [slice][C][3], the slabs of pw_wgrad's workspace [slice][K][C] and hm_rowsum's [N][K]
    floats one by one: 4 bytes (the kernels' float4 traffic is on their own LDS arrays, aligned(16)).
  * SGD, clipped SGD, cast, EMA (optim.hip): p, g, buf of the SGD kernels and e, p of mi355_ema_update as float4 with a scalar
    tail -- the entry points check 16 bytes themselves ("pointers must be 16-byte aligned"); the bf16 copy and cast's source
    and destination element by element: 2 / 4 bytes; lr_dev and the coefficient pair: 4 bytes; the clip record (a double
    first): 8 bytes, checked.  ema_update_batched walks its ranges float by float (4 bytes; the int64 counters 8) and reads
    records whose first field is a pointer: 8 bytes of the table.
  * gradient norm and Adam (optim.hip, adam_slice.h): every range / p, g, m, v as float4 per lane behind the item's base
    (gn_table and adam_table refuse a base off a 16-byte boundary): 16 bytes; the item tables, the partials (doubles) and the
    clip record: 8 bytes, checked by the entry points; step and lr of an item: one float each, 4 bytes.
  * MMD (mmd.hip): source, target, the gradients, rows and the workspace through plain float pointers: 4 bytes, checked
    ("pointers must be 4-byte aligned"); float4 accesses only when HW % 4 == 0 and the bases are 16-byte aligned (the host
    chooses the scalar build otherwise: the tests run both, at START and at START + 4).  The (K, n, n) workspace float by float.
  * per-joint pooling, KL, scatter, prototype update (jfa.hip, proto.hip, joint_pool.h): the feature map and its gradient in
    16-byte chunks (the wrappers refuse another start), descriptors, prototypes, the memory and the KL gradients as float4 rows
    ("must be 16-byte aligned", checked by the entry points): 16 bytes; key points, rows and the blend record float by float:
    4 bytes.
  * consistency MSE (mi355_mse_heatmap, teacher.hip): 4 bytes, checked; float4 only when HW % 4 == 0 and pred, target and the
    gradient sit on 16-byte boundaries (the scalar build otherwise: tests/test_gpu_mt.py runs it at START + 4).
  * MX quantiser and packs (mx_fp8.hip): above.  The item table of the batched pack holds pointers: 8 bytes.
  * training augmentation (augment.hip): the packed sources, the geometry image and the records' bytes one by one (the records
    are structs whose first field is an int64: 8 bytes); x and image_ema float by float: 4 bytes; the workspace begins with
    the B luminance sums (unsigned long long, atomicAdd): 8 bytes, the geometry image follows at the next multiple of 256.

No family assumes more than 16 bytes of an operand's first byte, so every payload of these suites starts at START and no
entry point had to learn a new refusal.  (16 bytes is also what a production run offers: mi355.nn hands the kernels views into
flat buffers of packed weights and gradients.)

What the window does not guard, and why.  torch.empty, torch.empty_strided, torch.empty_like and ops.workspace are replaced;
anything a wrapper makes by other means is outside: the device copy of the augmentation records (Tensor.to of a pinned host
array inside mi355.augment._prepare; tests/test_gpu_augment.py runs the mixed batch a second time through the ABI with a placed
copy), the item tables of ema_table / gn_table / adam_table / fold_table (torch.from_numpy(...).to(device): the tests place a
copy and hand that in), proto_blend's and mse_record's two-element records (placed by the tests likewise), and every gradient
autograd itself allocates in the tests that go through uda.model.loss.  The two caching wrappers (mi355.augment._ws,
mi355.ops._mmd_ws) allocate with torch.empty: a test empties the cache with monkeypatch, so the buffer is made inside the window
at exactly the size the library reports.  An all-ones element can be a right answer where the expected value is a NaN (the
hardware's float -> bf16 conversion keeps no promise about a NaN's payload; 0xFFFF was seen from the max-pool): such tests count
unwritten elements only where the reference is not a NaN.

What the fill cannot reach: the conv family reads x, w, dy, the second operand pair of the concat-K builds, the MX scale
arrays and pgemm's addends through buffer resources whose size is the operand's, so a read past the END of one of them returns
zero from the hardware, not the flank, and so does one in front of it (the offset is unsigned); a wrong row INSIDE the operand
shows as a wrong result, as before.  The addends of the gather epilogue, the per-channel vectors and every BatchNorm operand
go through plain pointers and do see the flanks.  Values a kernel loads and then discards (a masked lane, a row behind M that
is loaded and never stored) are invisible to this and every other test.

Use.
    v = place(t, 'x')                  # a copy of t inside a guarded buffer, same shape / strides / dtype
    with window(ops, 'fwd+bias'):      # torch.empty, empty_strided, empty_like and ops.workspace are guarded while it is open
        y = ops.conv_fwd(desc, v, w)
    torch.cuda.synchronize()
    check()                            # every flank byte of every buffer since the last check is still 0xFF
    assert unwritten(y) == 0           # ... and the launch wrote all of y
"""
import contextlib
import weakref

import torch

FILL = 0xFF
FLOOR = 4096             # least flank, bytes
ROWS = 256               # least flank, rows of the payload's pitch
BOUNDARY = 256
START = 16               # the payload's first byte, past a BOUNDARY
FLAT_PITCH = 4096        # a flat payload's own pitch is its length, at most this
LEAN_ABOVE = 64 << 20

_real_empty, _real_empty_strided, _real_empty_like = torch.empty, torch.empty_strided, torch.empty_like


class GuardError(AssertionError):
    pass


class _Buf(object):
    __slots__ = ('raw', 'start', 'n', 'name', 'label', 'view', 'placed')

    def front(self):
        return self.raw[:self.start]

    def back(self):
        return self.raw[self.start + self.n:]

    def payload(self):
        return self.raw[self.start:self.start + self.n]

    def address(self):
        return self.raw.data_ptr() + self.start


_bufs = []               # every buffer since the last check(), and the placed ones whose view is still alive
_state = {'label': '', 'pitch': 0, 'lean': False}


def row_pitch(nbytes):
    """Bytes of the widest row the kernels of the following calls stride by: from now on no flank is shorter than ROWS of it."""
    _state['pitch'] = int(nbytes)


def flank_bytes(pitch, nbytes=0, lean=False):
    rows = FLOOR + ROWS * pitch if (lean and nbytes > LEAN_ABOVE) else max(FLOOR, ROWS * pitch)
    return (rows + BOUNDARY - 1) // BOUNDARY * BOUNDARY


def _alloc(nbytes, pitch, device, name, start, extra=0):
    """A 0xFF-filled buffer with `nbytes` of payload at `start` bytes past a 256-byte boundary; the payload's view may run
    `extra` bytes into the back flank (the rounding of a workspace), which stay guarded."""
    flank = flank_bytes(max(pitch, _state['pitch']), nbytes, _state['lean'])
    raw = _real_empty(flank + BOUNDARY + nbytes + extra + flank, dtype=torch.uint8, device=device)
    raw.fill_(FILL)
    b = _Buf()
    b.raw, b.n, b.name, b.label, b.view, b.placed = raw, int(nbytes), name, _state['label'], None, False
    b.start = flank + (start - (raw.data_ptr() + flank)) % BOUNDARY
    assert b.start >= flank and raw.numel() - b.start - b.n - extra >= flank and b.address() % BOUNDARY == start % BOUNDARY
    _bufs.append(b)
    return b


def _extent(shape, strides):
    """Elements of storage a view of this shape and these strides spans, and the extent of its unit-stride axis."""
    if any(s == 0 for s in shape):
        return 0, 0
    ext = 1 + sum((n - 1) * st for n, st in zip(shape, strides))
    unit = [n for n, st in zip(shape, strides) if st == 1 and n > 1]
    return ext, (max(unit) if unit else 1)


def _pitch(shape, strides, esize, pitch):
    ext, unit = _extent(shape, strides)
    if pitch:
        return pitch
    return min(ext * esize, FLAT_PITCH) if len(shape) < 2 else unit * esize


def _strided(shape, strides, dtype, device, name, start=START, pitch=0):
    shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
    esize = torch.empty((), dtype=dtype).element_size() if not hasattr(dtype, 'itemsize') else dtype.itemsize
    ext, _ = _extent(shape, strides)
    assert all(st >= 0 for st in strides) and start % esize == 0
    b = _alloc(ext * esize, _pitch(shape, strides, esize, pitch), device, name, start)
    v = b.payload().view(dtype).as_strided(shape, strides) if ext else _real_empty_strided(shape, strides, dtype=dtype, device=device)
    return b, v


def _contiguous_strides(shape):
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= max(int(n), 1)
    return tuple(reversed(st))


def place(t, name='operand', start=START, pitch=0):
    """A copy of `t` inside a guarded buffer: same device, shape, strides and dtype (a channels_last tensor stays channels_last);
    the buffer is checked by every check() for as long as the returned view is alive."""
    b, v = _strided(t.shape, t.stride(), t.dtype, t.device, name, start, pitch)
    v.copy_(t)
    b.placed = True
    b.view = weakref.ref(v)
    return v


def empty(shape, dtype, device, name='output', start=START):
    """A guarded buffer of this shape with nothing but the fill in it: an output the caller hands to a launch that must write
    all of it (a weight gradient that overwrites)."""
    shape = tuple(int(s) for s in shape)
    return _strided(shape, _contiguous_strides(shape), dtype, device, name, start)[1]


def _guards(device, want):
    return torch.device(device).type == want


def _default_device():
    get = getattr(torch, 'get_default_device', None)
    return get() if get is not None else torch.device('cpu')


@contextlib.contextmanager
def window(ops, label='', device=None, pitch=0, start=START, lean=False):
    """While open: torch.empty, torch.empty_strided and torch.empty_like of `device`'s type (default: cuda where there is one, else
    cpu) return views of guarded 0xFF-filled buffers with the requested shape, strides and dtype (empty_like: those of its
    argument, which must be dense; dtype= and device= are honoured, anything else goes to the real function), and
    ops.workspace(nbytes, ...) returns a guarded 0xFF-filled view of exactly nbytes rounded up to 16, made for this call only.
    All four are restored on the way out, whatever happens inside.  pitch: bytes of the widest row a kernel of the call strides by (a lower bound for every flank)."""
    want = torch.device(device).type if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu')
    saved = (torch.empty, torch.empty_strided, ops.workspace, dict(_state), torch.empty_like)

    def empty(*size, **kw):
        dev = kw.get('device', None)
        dev = torch.device(dev) if dev is not None else _default_device()
        fmt = kw.get('memory_format', torch.contiguous_format)
        if not _guards(dev, want) or kw.get('out') is not None or kw.get('pin_memory') or kw.get('layout', torch.strided) != torch.strided \
                or fmt not in (torch.contiguous_format, torch.channels_last):
            return saved[0](*size, **kw)
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        dtype = kw.get('dtype') or torch.get_default_dtype()
        strides = _contiguous_strides(shape)
        if fmt == torch.channels_last:
            N, C, H, W = shape
            strides = (H * W * C, 1, W * C, C)
        v = _strided(shape, strides, dtype, dev, 'empty%s %s' % (shape, dtype), start)[1]
        return v.requires_grad_() if kw.get('requires_grad') else v

    def empty_strided(size, stride, **kw):
        dev = kw.get('device', None)
        dev = torch.device(dev) if dev is not None else _default_device()
        if not _guards(dev, want) or kw.get('pin_memory') or kw.get('layout', torch.strided) != torch.strided:
            return saved[1](size, stride, **kw)
        dtype = kw.get('dtype') or torch.get_default_dtype()
        return _strided(size, stride, dtype, dev, 'empty_strided%s %s' % (tuple(size), dtype), start)[1]

    def empty_like(t, **kw):
        dev = torch.device(kw['device']) if kw.get('device') is not None else t.device
        fmt = kw.get('memory_format', torch.preserve_format)
        layout = kw.get('layout') or t.layout
        dense = t.dim() == 0 or t.numel() == 0 or _extent(tuple(t.shape), t.stride())[0] == t.numel()
        if not _guards(dev, want) or kw.get('pin_memory') or layout != torch.strided or t.layout != torch.strided \
                or fmt != torch.preserve_format or not dense or any(st < 0 for st in t.stride()):
            return saved[4](t, **kw)                    # not modelled: a gapped or overlapping source, another memory format
        dtype = kw.get('dtype') or t.dtype
        v = _strided(t.shape, t.stride(), dtype, dev, 'empty_like%s %s' % (tuple(t.shape), dtype), start)[1]
        return v.requires_grad_() if kw.get('requires_grad') else v

    def workspace(nbytes, device, tag='main'):
        nbytes = int(nbytes)
        size = (nbytes + 15) // 16 * 16
        b = _alloc(nbytes, min(max(nbytes, 1), FLAT_PITCH), device, 'workspace(%d)' % nbytes, start, extra=size - nbytes)
        return b.raw[b.start:b.start + size]

    _state.update(label=label, pitch=max(int(pitch), _state['pitch']), lean=bool(lean))
    torch.empty, torch.empty_strided, torch.empty_like, ops.workspace = empty, empty_strided, empty_like, workspace
    try:
        yield
    finally:
        torch.empty, torch.empty_strided, ops.workspace = saved[:3]
        torch.empty_like = saved[4]
        _state.clear()
        _state.update(saved[3])


def _changed(b, side):
    """(first, last) changed byte of one flank, as offsets relative to the payload's first byte."""
    part = b.front() if side == 'front' else b.back()
    bad = (part != FILL).nonzero().view(-1)
    off = -b.start if side == 'front' else b.n
    return int(bad[0]) + off, int(bad[-1]) + off


def check(label=None):
    """After the device has been synchronised: every flank byte of every buffer made by place() or inside a window since the last
    check (and of every placed buffer whose view is still alive) is 0xFF.  Raises GuardError naming the buffer, the side, the first
    and last changed byte relative to the payload (negative: in front of it; >= its size: behind it) and the call's label."""
    global _bufs
    bufs, _bufs = _bufs, []
    # keep the placed buffers that are still in use; the window's are checked once (their views keep the storage alive)
    _bufs = [b for b in bufs if b.placed and b.view is not None and b.view() is not None]
    if not bufs:
        return
    # 0xFF is the largest byte: a flank is intact iff its minimum is 0xFF.  One host read per device for all of them.
    by_dev = {}
    for b in bufs:
        by_dev.setdefault(b.raw.device, []).append(b)
    wrong = []
    for dev, group in by_dev.items():
        mins = torch.stack([m for b in group for m in (b.front().min(), b.back().min())]).cpu().tolist()
        for i, b in enumerate(group):
            for side, m in (('front', mins[2 * i]), ('back', mins[2 * i + 1])):
                if m != FILL:
                    first, last = _changed(b, side)
                    wrong.append('%s [%s]: %s flank changed, bytes %d .. %d relative to a payload of %d bytes (call: %s)' % (
                        b.name, b.label or '-', side, first, last, b.n, label or b.label or _state['label'] or '-'))
    if wrong:
        raise GuardError('%d guard flank(s) written:\n  %s' % (len(wrong), '\n  '.join(wrong)))


def _buf_of(t):
    p = t.data_ptr()
    for b in _bufs:
        if b.address() <= p < b.address() + max(b.n, 1):
            return b
    return None


def unwritten(t):
    """Bytes of `t`'s storage span that still belong to an element whose every byte is 0xFF (the span runs from t's first
    element over its extent: for a dense view, all of it).  0 for an output its launch wrote completely, provided the right
    answer holds no all-ones element (it never does for the integer operands of the exact suites: 0xFF.. is a NaN)."""
    ext, _ = _extent(tuple(t.shape), tuple(t.stride()))
    if ext == 0:
        return 0
    esize = t.element_size()
    flat = t.as_strided((ext,), (1,)).view(torch.uint8).view(ext, esize)
    return int((flat == FILL).all(dim=1).sum()) * esize


def reset():
    """Forget every buffer and the row pitch (a test that expects check() to fail cleans up with this)."""
    del _bufs[:]
    _state.update(label='', pitch=0, lean=False)
