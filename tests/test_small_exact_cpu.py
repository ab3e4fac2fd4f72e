"""CPU half of the exact-operand suite of the small kernels: the range condition of every case of tests/small_exact_ref.py, and
each float64 reference held against torch on the CPU.  test_gpu_small_exact.py compares the HIP kernels with these references."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_exact_ref as R


# ---------------------------------------------------------------- A. max-pool
@pytest.fixture(scope='module')
def mp_refs():
    return {}


def _mp(mp_refs, name):
    if name not in mp_refs:
        c = R.mp_case(name)
        c['y'], c['code'], c['dx'] = R.check_exact_maxpool(c)
        mp_refs[name] = c
    return mp_refs[name]


def test_maxpool_table_reaches_every_edge(mp_refs):
    """Over the table: NaN windows, windows of nothing but -inf, whole-window ties, every one of the nine codes, and sums of
    two and more gradients in one input element."""
    nan = ninf = tie = multi = 0
    codes = set()
    for name in R.MP_CASES:
        c = _mp(mp_refs, name)
        nan += int((c['y'] != c['y']).sum())
        ninf += int((c['y'] == -R.INF).sum())
        tie += int(((c['y'] == 0) & (c['code'] != 4)).sum())
        codes |= set(c['code'].unique().tolist())
        hits = R.maxpool_bwd(torch.ones_like(c['dy']), c['code'], c['x'].shape)
        multi += int((hits >= 2).sum())
    assert nan > 100 and ninf > 10 and tie > 100 and multi > 100 and codes == set(range(9))


@pytest.mark.parametrize('name', list(R.MP_CASES))
@pytest.mark.parametrize('layout', ['contiguous', 'channels_last'])
def test_maxpool_reference_is_torch(mp_refs, name, layout):
    """Values, window codes and the backward against ATen's CPU max-pool in float64 (its tie, -inf and NaN rules are the
    kernel's)."""
    c = _mp(mp_refs, name)
    N, C, H, W = c['x'].shape
    x = c['x'].clone()
    if layout == 'channels_last':
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    y, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    assert R.bits_equal(y.detach().contiguous(), c['y'])
    Ho, Wo = R.mp_out(H, W)
    oy, ox = torch.arange(Ho).view(Ho, 1), torch.arange(Wo).view(1, Wo)
    code = (idx // W - (2 * oy - 1)) * 3 + (idx % W - (2 * ox - 1))
    assert torch.equal(code, c['code'].long())
    y.backward(c['dy'])
    assert torch.equal(x.grad.contiguous(), c['dx'])
    assert np.array_equal(R.maxpool_bwd_np(c['dy'].numpy(), c['code'].numpy(), (N, C, H, W)), c['dx'].numpy())


def test_maxpool_lap_case_shape():
    dt, N, C, H, W = R.MP_LAP
    Ho, Wo = R.mp_out(H, W)
    assert N * Ho * Wo * (C // R.PER[dt]) == 2119936 > 8192 * 256
    assert 3 * 8192 * 256 < N * H * W * (C // R.PER[dt]) <= 5 * 8192 * 256 and N * H * W * (C // R.PER[dt]) < 2 ** 31


# ---------------------------------------------------------------- B. layout
def test_special_values_are_what_they_claim():
    s = torch.from_numpy(R.SPECIALS)
    b = s.to(torch.bfloat16).float()
    assert float(b[0]) == 1.0 and float(b[1]) == 1.015625 and float(b[2]) == -1.0 and float(b[3]) == -1.015625      # ties to even
    assert torch.signbit(s[4]) and float(s[4]) == 0 and not torch.signbit(s[5])
    assert 0 < float(s[6]) < 2.0 ** -126 and float(s[7]) == 2.0 ** -133 and float(b[7]) == 2.0 ** -133
    assert float(b[8]) == float(s[8]) == R.BF16_MAX and float(b[10]) == R.INF and np.isfinite(float(s[10]))
    assert float(s[11]) == R.INF and float(s[12]) == -R.INF and bool(s[13] != s[13])
    assert R.ties(s[:4].double(), 'bf16') == 4
    v = R.layout_values('probe', 3, 33, 9, 33)
    for q in s[:13]:
        assert bool(((v == q) & (torch.signbit(v) == torch.signbit(q))).any())
    assert bool((v != v).any())
    nan2 = torch.tensor([float('nan'), 1.0]).view(torch.int32)
    nan2[0] |= 1                                       # another payload
    assert R.bits_equal(nan2.view(torch.float32), torch.tensor([float('nan'), 1.0]))
    assert not R.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))


@pytest.mark.parametrize('dt', R.DTS)
@pytest.mark.parametrize('C,cpad', R.TO_NHWC_C)
def test_to_nhwc_reference(dt, C, cpad):
    for N in (1, 3):
        for H, W in R.TO_NHWC_MAPS:
            x = R.layout_values('to_nhwc', N, C, H, W)
            out = R.to_nhwc(x, dt, cpad)
            cp = cpad or R.default_cpad(C, dt)
            assert out.shape == (N, cp, H, W) and cp % R.PER[dt] == 0
            mem = out.permute(0, 2, 3, 1)                                      # the NHWC order
            assert R.bits_equal(mem[..., :C].contiguous(), x.permute(0, 2, 3, 1).to(R.TDT[dt]).contiguous())
            pad = mem[..., C:]
            assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any())


def test_to_nhwc_lap_case_shape():
    N, C, cpad, H, W = R.TO_NHWC_LAP
    assert cpad == R.default_cpad(C, 'f32') and N * H * W * (cpad // 4) == 4456448 > 16384 * 256


@pytest.mark.parametrize('dt', R.DTS)
def test_to_nchw_reference(dt):
    for C in R.TO_NCHW_C:
        for H, W in R.TO_NCHW_MAPS:
            x = R.nhwc(R.layout_values('to_nchw', 3, C, H, W), R.TDT[dt])
            y = R.to_nchw_f32(x)
            assert y.is_contiguous() and y.dtype == torch.float32
            assert R.bits_equal(y, x.float().contiguous())
            assert R.bits_equal(R.to_nhwc(y, dt, C if C % R.PER[dt] == 0 else None)[:, :C].contiguous(), x.contiguous())


@pytest.mark.parametrize('N,H,W', R.S2D_SHAPES)
def test_s2d_reference(N, H, W):
    x = R.layout_values('s2d', N, 3, H, W)
    y = R.s2d(x, 'f32')
    for dy in range(2):
        for dx in range(2):
            g = (dy * 2 + dx) * 4
            assert R.bits_equal(y[:, g:g + 3].contiguous(), x[:, :, dy::2, dx::2].contiguous())
            assert bool((y[:, g + 3] == 0).all()) and not bool(torch.signbit(y[:, g + 3]).any())
    assert R.bits_equal(R.s2d(x, 'bf16'), y.to(torch.bfloat16))


def _pack_by_index(w):
    """The formula in the comment above nchw_to_s2d_kernel, element by element: kh = 2 * tap_row + dy - 1 (kw alike)."""
    Co = w.shape[0]
    out = torch.zeros(Co * 256, dtype=w.dtype)
    flat = w.reshape(-1)
    for i in range(Co * 256):
        ch, tap, o = i % 16, (i // 16) % 16, i // 256
        c, dy, dx = ch % 4, ch // 8, (ch // 4) % 2
        kh, kw = 2 * (tap // 4) + dy - 1, 2 * (tap % 4) + dx - 1
        if c < 3 and 0 <= kh < 7 and 0 <= kw < 7:
            out[i] = flat[((o * 7 + kh) * 7 + kw) * 3 + c]
    return out.view(Co, 4, 4, 16)


@pytest.mark.parametrize('Co', R.STEM_CO)
def test_stem_pack_unpack_reference(Co):
    w = R.int_values('stem w', -8, 8, Co, 7, 7, 3)
    gs = R.int_values('stem gs', -8, 8, Co, 4, 4, 16)
    assert torch.equal(R.stem_pack(w), _pack_by_index(w))
    # every weight appears exactly once; 256 - 147 slots stay zero
    ids = torch.arange(1, Co * 147 + 1, dtype=torch.float64).view(Co, 7, 7, 3)
    assert torch.equal(R.stem_pack(ids).reshape(-1).sort().values[-Co * 147:], ids.reshape(-1))
    assert torch.equal(R.stem_unpack(R.stem_pack(w)), w)
    # adjoint: <pack(w), gs> == <w, unpack(gs)>
    assert float((R.stem_pack(w) * gs).sum()) == float((w * R.stem_unpack(gs)).sum())
    prior = R.int_values('stem prior', -8, 8, Co, 7, 7, 3)
    assert torch.equal(R.stem_unpack(gs, prior), R.stem_unpack(gs) + prior)


def test_folded_stem_is_the_7x7_stride_2_conv():
    x = R.int_values('stem x', -4, 4, 2, 3, 12, 10)
    w = R.int_values('stem w', -4, 4, 5, 7, 7, 3)                              # [Co][kh][kw][c]
    ref = F.conv2d(x, w.permute(0, 3, 1, 2), stride=2, padding=3)
    wp = R.stem_pack(w).permute(0, 3, 1, 2)                                    # [Co][16][4][4]
    got = F.conv2d(F.pad(R.s2d(x), (2, 1, 2, 1)), wp)
    assert torch.equal(got, ref)


# ---------------------------------------------------------------- C. pw21
def _pw_shapes():
    seen = []
    for dt, C, K in R.C2K_CASES + R.K2C_CASES:
        for N in R.PW_N:
            for HW in R.PW_HW:
                seen.append((dt, N, C, K, HW))
    seen += [(dt, N, C, 21, 100) for dt, C, N in R.K2C_STATS_CASES]
    seen += [(dt, 2, C, 21, HW) for dt in R.DTS for C in (24, 264) for HW in R.PW_EDGE_HW]       # the statistics at the tile edges
    seen += [(dt, N, C, K, HW) for dt, C, K, N, HW in R.WGRAD_CASES]
    return sorted(set(seen))


def test_pw_cases_are_exact_and_hold_ties():
    tied = 0
    for dt, N, C, K, HW in _pw_shapes():
        t = R.check_exact_pw(R.pw_case(dt, N, C, K, HW))
        if R.needs_tie(dt, N, C, K, HW):
            assert t >= 1, (dt, N, C, K, HW)
            tied += 1
    assert tied > 30


def test_pw_lds_sizes():
    """C = 512 in bf16 is the only C -> K case above the 64 KB default; fp32 at C = 512 and K = 21 is above the 160 KB limit."""
    smem = lambda C, K, esz: 64 * (C * esz + 16) + K * C * 4
    assert 64 * 1024 < smem(512, 21, 2) == 109568 and smem(512, 32, 2) <= 160 * 1024
    assert max(smem(C, 32, 2 if dt == 'bf16' else 4) for dt, C, K in R.C2K_CASES if C < 512) < 160 * 1024
    assert smem(512, 21, 4) > 160 * 1024


@pytest.mark.parametrize('dt,N,C,K,HW', [('bf16', 3, 24, 21, 65), ('f32', 1, 264, 32, 100), ('bf16', 3, 8, 1, 192)])
def test_pw_references_are_torch(dt, N, C, K, HW):
    c = R.pw_case(dt, N, C, K, HW)
    x, y = c['x'], c['y']
    assert torch.equal(R.pw_c2k(x, c['wkc'], c['bias_k']), F.conv2d(x, c['wkc'].view(K, C, 1, 1), c['bias_k']))
    assert torch.equal(R.pw_c2k(x, c['wkc']), F.conv2d(x, c['wkc'].view(K, C, 1, 1)))
    assert torch.equal(R.pw_k2c(y, c['wck'], c['bias_c'], c['res'], 0.5),
                       0.5 * (F.conv2d(y, c['wck'].view(C, K, 1, 1), c['bias_c']) + c['res']))
    assert torch.equal(R.pw_k2c(y, c['wck']), F.conv2d(y, c['wck'].view(C, K, 1, 1)))
    # the weight gradient of the C -> K conv by autograd
    w = c['wkc'].clone().requires_grad_(True)
    F.conv2d(x, w.view(K, C, 1, 1)).backward(y)
    assert torch.equal(R.pw_wgrad(x, y), w.grad)
    assert torch.equal(R.pw_wgrad(x, y, c['prior_w']), w.grad + c['prior_w'])
    b = c['bias_k'].clone().requires_grad_(True)
    F.conv2d(x, c['wkc'].view(K, C, 1, 1), b).backward(y)
    assert torch.equal(R.hm_rowsum(y), b.grad)


def test_slice_stats_reference():
    out = R.int_values('stats', -9, 9, 3, 24, 10, 10)
    st = R.slice_stats(out, 100)
    assert st.shape == (6, 24, 3)
    assert torch.equal(st[:, :, 0], torch.tensor([64.0, 36.0] * 3).view(6, 1).expand(6, 24))
    rows = out.reshape(3, 24, 100)
    assert torch.allclose(st[3, :, 1], rows[1, :, 64:].mean(1), rtol=0, atol=1e-12)
    assert torch.allclose(st[2, :, 2], rows[1, :, :64].var(1, unbiased=False) * 64, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('N,K,HW', R.ROWSUM_CASES)
def test_rowsum_cases_are_exact(N, K, HW):
    R.check_exact_rowsum(R.rowsum_case(N, K, HW))


# ---------------------------------------------------------------- D. optimiser
@pytest.mark.parametrize('case', R.SGD_CASES, ids=R.case_id)
def test_sgd_reference_is_torch(case):
    n, nesterov, wd = case
    c = R.sgd_case(n)
    assert bool((c['p'] % 4 == 0).all()) and float(c['p'].abs().max()) <= 64
    p_ref, buf_ref = R.check_exact_sgd(c, nesterov, wd)
    p = c['p'].clone().requires_grad_(True)
    opt = torch.optim.SGD([p], lr=1.0, momentum=R.SGD_MU, weight_decay=wd, nesterov=nesterov)
    for g, lr in zip(c['g'], R.SGD_LRS):
        opt.param_groups[0]['lr'] = lr
        p.grad = g.clone()
        opt.step()
    assert torch.equal(p.detach(), p_ref)
    assert torch.equal(opt.state[p]['momentum_buffer'], buf_ref)


def test_sgd_table_reaches_the_second_lap_and_every_tail():
    assert {n % 4 for n in R.SGD_N} == {0, 1, 2, 3} and min(R.SGD_N) < 4
    big = max(R.SGD_N)
    assert big // 4 == 4096 * 256 + 300 and big % 4 == 3
    assert max(R.CAST_N) == 4096 * 256 + 77
    v = R.cast_values(257)
    assert bool((v != v).any()) and R.ties(v[(v == v) & (v.abs() < 2)].double(), 'bf16') >= 1
