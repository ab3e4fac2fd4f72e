"""The reference of the per-tensor fp8 front end (tests/fp8_ref.py) is right, and the input sets of
tests/test_gpu_fp8_exact.py discriminate: each wrong variant a kernel could implement differs from the reference on them."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import fp8_ref as R

FMTS = [R.E4M3, R.E5M2]
TDT = {R.E4M3: torch.float8_e4m3fn, R.E5M2: torch.float8_e5m2}


# ---------------------------------------------------------------- the reference against torch and against fractions
@pytest.mark.parametrize('fmt', FMTS)
def test_decode_table_is_torchs(fmt):
    ref = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(TDT[fmt]).float().numpy()
    mine = R.decode_table(fmt)
    assert np.array_equal(np.isnan(mine), np.isnan(ref))
    assert np.array_equal(mine[~np.isnan(ref)], ref[~np.isnan(ref)].astype(np.float64))
    assert np.array_equal(np.signbit(mine[~np.isnan(ref)]), np.signbit(ref[~np.isnan(ref)]))


def _torch_encode(y, fmt):
    lim = R.FMT_MAX[fmt]
    return torch.from_numpy(y).clamp(-lim, lim).to(TDT[fmt]).view(torch.uint8).numpy()


def _assert_codes_equal(mine, ref, src, fmt):
    nan = np.isnan(src)
    assert np.array_equal(mine[~nan], ref[~nan]), np.nonzero((mine != ref) & ~nan)[0][:8]
    tab = R.decode_table(fmt)
    assert np.isnan(tab[mine[nan]]).all() and np.isnan(tab[ref[nan]]).all()


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('k', R.SCALE_KS)
def test_encode_equals_torch_cast_on_every_bf16_value(fmt, k):
    y = R.scaled(R.bf16_patterns(), R.make_state(R.pow2(k), R.pow2(-k)))
    _assert_codes_equal(R.encode(y, fmt), _torch_encode(y, fmt), y, fmt)


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('k', R.TIE_KS)
def test_encode_equals_torch_cast_on_the_tie_set(fmt, k):
    x = R.tie_set(fmt, k)
    y = R.scaled(x, R.make_state(R.pow2(k), R.pow2(-k)))
    assert np.array_equal(y[:len(R.tie_values(fmt))].view(np.uint32), R.tie_values(fmt).view(np.uint32))     # x * scale is exact
    _assert_codes_equal(R.encode(y, fmt), _torch_encode(y, fmt), y, fmt)
    assert R.encode(np.float32(-0.0), fmt) == 0x80 and R.encode(np.float32(np.inf), fmt) == R.TOP[fmt]


def _fraction_rule(amax_bits, old_scale, old_descale, fmt, margin):
    amax = float(R.from_bits(np.uint32(amax_bits)))
    if not (amax > 0 and amax < float(np.float32(3.0e38))):
        return (1.0, 1.0) if old_scale == 0 else (old_scale, old_descale)
    a, lim = Fraction(amax) * 2 ** margin, Fraction(R.FMT_MAX[fmt])
    k = -200
    while a * Fraction(2) ** (k + 1) <= lim:
        k += 1
    assert a * Fraction(2) ** k <= lim < a * Fraction(2) ** (k + 1)
    k = max(-126, min(126, k))
    return float(Fraction(2) ** k), float(Fraction(2) ** -k)


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('margin', [0, 1, 8])
def test_scale_rule_equals_the_rule_stated_in_fractions(fmt, margin):
    for ab, sc, de in R.scale_points(fmt):
        got = R.scale_rule(ab, sc, de, fmt, margin)
        assert (float(got[0]), float(got[1])) == _fraction_rule(ab, sc, de, fmt, margin), hex(ab)
        assert all(np.isfinite(g) and g.dtype == np.float32 and (R.bits(g) & 0x7f800000) != 0 for g in got)     # normal floats


# ---------------------------------------------------------------- wrong variants
def _enc_variant(mode=None, saturate=True):
    """encode with another rounding ('away': ties away from zero, 'trunc': toward zero) or without saturation (overflow -> the
    format's NaN / Inf code, as an unclamped conversion gives)"""
    def enc(x, fmt):
        x = R.f32(x)
        vals = R.decode_table(fmt)[:R.TOP[fmt] + 1]
        a = np.abs(x.astype(np.float64))
        nan = np.isnan(a)
        over = ~nan & (a > R.FMT_MAX[fmt])
        a = np.where(nan, 0.0, np.minimum(a, R.FMT_MAX[fmt]))
        lo = np.searchsorted(vals, a, side='right') - 1
        hi = np.minimum(lo + 1, R.TOP[fmt])
        two_a, s = 2.0 * a, vals[lo] + vals[hi]
        if mode == 'away':
            up = two_a >= s
        elif mode == 'trunc':
            up = np.zeros_like(nan)
        else:
            up = (two_a > s) | ((two_a == s) & (lo % 2 == 1))
        code = np.where(up, hi, lo)
        if not saturate:
            code = np.where(over, 0x7f if fmt == R.E4M3 else 0x7c, code)
        code = np.where(nan, R.NAN_CODE, code)
        return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)
    return enc


ENC_VARIANTS = {'round-half-away': _enc_variant('away'), 'truncation': _enc_variant('trunc'), 'no saturation': _enc_variant(saturate=False)}


def _amax_nan_as_zero(x):
    """a max that NaN poisons, recorded as 0"""
    m = np.abs(R.f32(x)).max()
    return 0 if np.isnan(m) else int(R.bits(m))


def _amax_ignores_inf(x):
    a = np.abs(R.f32(x).reshape(-1))
    a = a[np.isfinite(a)]
    return int(R.bits(a.max())) if a.size else 0


def _amax_forgets_at_signalling_nan(x):
    """a running max per 16-element chunk that a signalling NaN turns into NaN, which the next number then replaces (a hardware
    max on raw inputs); chunks are combined by a max that skips NaN"""
    x = R.f32(x).reshape(-1, 16)
    b = R.bits(x)
    snan = np.isnan(x) & ((b & 0x00400000) == 0)
    best = np.float32(0)
    for row, srow in zip(np.abs(x), snan):
        m = np.float32(0)
        for a, s in zip(row, srow):
            if s:
                m = np.float32(np.nan)
            elif not np.isnan(a):
                m = a if np.isnan(m) else max(m, a)
        if not np.isnan(m):
            best = max(best, m)
    return int(R.bits(best))


AMAX_VARIANTS = {'NaN as 0': _amax_nan_as_zero, 'ignores Inf': _amax_ignores_inf}


def _log2_rule(amax_bits, old_scale, old_descale, fmt, margin):
    """the scale rule through float32 log2 / exp2, without a clamp"""
    amax = R.from_bits(np.uint32(amax_bits))
    if amax > 0 and amax < np.float32(3.0e38):
        with np.errstate(over='ignore', divide='ignore'):
            raw = np.float32(R.FMT_MAX[fmt]) / (amax * np.float32(1 << margin))
            sc = np.exp2(np.floor(np.log2(raw)))
            return np.float32(sc), np.float32(1) / np.float32(sc)
    return R.scale_rule(amax_bits, old_scale, old_descale, fmt, margin)


def _unclamped_rule(amax_bits, old_scale, old_descale, fmt, margin):
    amax = R.from_bits(np.uint32(amax_bits))
    if amax > 0 and amax < np.float32(3.0e38):
        k = R.scale_exponent(amax_bits, fmt, margin)
        with np.errstate(over='ignore', under='ignore'):
            return np.float32(2.0 ** k), np.float32(2.0 ** -k)
    return R.scale_rule(amax_bits, old_scale, old_descale, fmt, margin)


RULE_VARIANTS = {'float32 log2': _log2_rule, 'no clamp': _unclamped_rule}


def _differs(a, b):
    """do two results (tuples of byte / word arrays or None) differ anywhere"""
    return any((x is None) != (y is None) or (x is not None and not np.array_equal(x, y)) for x, y in zip(a, b))


def _delayed(k):
    return R.make_state(R.pow2(k), R.pow2(-k))


@pytest.mark.parametrize('fmt', FMTS)
def test_quantiser_sets_tell_rounding_saturation_and_amax_variants_apart(fmt):
    """sets a (every bf16 value), b (ties), c (geometry) and d (write modes; it quantises the middle geometry tensor)"""
    sets = {'a k=%d' % k: (R.bf16_patterns(), _delayed(k)) for k in R.SCALE_KS}
    sets.update({'b k=%d' % k: (R.tie_set(fmt, k), _delayed(k)) for k in R.TIE_KS})
    for n in R.GEOMETRY_NS[:2]:
        x = R.geometry_base(n, fmt).copy()
        x[R.geometry_positions(n)[-1]] = -R.GEOMETRY_AMAX
        sets['c/d n=%d' % n] = (x, _delayed(0))
    for name, (x, st) in sets.items():
        ref = R.quantize(x, st, fmt, 2)
        for vn, enc in ENC_VARIANTS.items():
            if vn == 'no saturation' and name.startswith('c'):
                continue                                 # (the geometry tensors stay below max by construction)
            assert _differs(R.quantize(x, st, fmt, 2, enc=enc), ref), (name, vn)
    # the amax variants: set a holds NaN and Inf, set b too; the finite-only form of a tells 'ignores Inf' nothing, so it is
    # the Inf of the full set that pins it
    for name in ('a k=0', 'b k=0'):
        x, st = sets[name]
        for vn, am in AMAX_VARIANTS.items():
            assert _differs(R.quantize(x, st, fmt, 2, amax=am), R.quantize(x, st, fmt, 2)), (name, vn)
    x, st = sets['a k=0']                 # (set a alone holds signalling NaNs: 15 of them follow each Inf in its chunk)
    assert R.quantize(x, st, fmt, 0, amax=_amax_forgets_at_signalling_nan)[2][2] == 0x7f7f0000 != R.quantize(x, st, fmt, 0)[2][2]


def test_pool_points_tell_the_two_formats_rules_apart():
    """set f: every slot whose scale is updated gets another one under the other format's rule, and the set takes the kept
    branch and the never-set branch as well"""
    after = [R.tick(R.make_state(sc, de, int(R.bits(a))), fmt) for fmt, a, sc, de in R.pool_points()]
    other = [R.tick(R.make_state(sc, de, int(R.bits(a))), 1 - fmt) for fmt, a, sc, de in R.pool_points()]
    moved = [not np.array_equal(s[:2], R.make_state(sc, de)[:2]) or sc == 0 for s, (fmt, a, sc, de) in zip(after, R.pool_points())]
    assert moved == [True, True, True, True, False]
    assert [not np.array_equal(s, o) for s, o in zip(after, other)] == [True, True, False, True, False]
    assert sorted(p[0] for p in R.pool_points()) == [R.E4M3] * 3 + [R.E5M2] * 2


@pytest.mark.parametrize('fmt', FMTS)
def test_geometry_sets_tell_a_missed_chunk_apart(fmt):
    """set c: the unique amax sits where a loop that drops its last chunk, its second block or its second trip loses it"""
    for n in R.GEOMETRY_NS:
        base = R.geometry_base(n, fmt)
        assert float(np.abs(base).max()) < float(R.GEOMETRY_AMAX)
        for p in R.geometry_positions(n):
            x = base.copy()
            x[p] = -R.GEOMETRY_AMAX
            assert R.quantize(x, _delayed(0), fmt, 0)[2][2] == R.bits(R.GEOMETRY_AMAX)
            x[p] = 0
            assert R.quantize(x, _delayed(0), fmt, 0)[2][2] != R.bits(R.GEOMETRY_AMAX)
    n = R.GEOMETRY_NS[2]
    assert R.geometry_positions(n)[-1] // 16 >= 1024 * 256          # reached on the second trip of a 1024 x 256 grid only


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('margin', [0, 1, 8])
def test_scale_points_tell_the_log2_rule_and_a_missing_clamp_apart(fmt, margin):
    """sets e and f"""
    pts = R.scale_points(fmt)
    ref = [R.scale_rule(ab, sc, de, fmt, margin) for ab, sc, de in pts]
    for vn, rule in RULE_VARIANTS.items():
        got = [rule(ab, sc, de, fmt, margin) for ab, sc, de in pts]
        bad = [hex(p[0]) for p, g, r in zip(pts, got, ref) if R.bits(g[0]) != R.bits(r[0]) or R.bits(g[1]) != R.bits(r[1])]
        assert bad, vn
    for s in ref:
        assert s[1] == np.float32(1) / s[0]


def _pack_layout_variants():
    return {'wt not transposed': lambda wf: wf.copy(),
            'tap and channel swapped': lambda wf: np.ascontiguousarray(wf.transpose(1, 2, 0))}       # [T][I][O] for [I][T][O]


@pytest.mark.parametrize('shape', R.PACK_SHAPES)
def test_pack_sets_tell_layout_rounding_and_rule_variants_apart(shape):
    """sets g and h"""
    O, T, I = shape
    w = R.pack_weights(O, T, I, 'amax_last')
    ref = R.pack(w, R.make_state(), O, T, I, 0)
    assert R.from_bits(ref[2][0]) == R.PACK_SCALE and ref[2][2] == R.bits(R.PACK_AMAX) and ref[2][3] == ref[2][1]
    assert np.array_equal(R.scaled(w, ref[2]) / np.float32(R.PACK_SCALE), w)                     # w * scale is exact
    for vn, lay in _pack_layout_variants().items():
        if vn == 'tap and channel swapped' and T == 1:
            continue                                     # (one tap: the two orders are the same bytes)
        assert _differs(R.pack(w, R.make_state(), O, T, I, 0, layout=lay), ref), vn
    for vn, enc in ENC_VARIANTS.items():
        st = R.make_state(2 * R.PACK_SCALE, 0.5 / R.PACK_SCALE)              # delayed with a scale that saturates the amax element
        assert _differs(R.pack(w, st, O, T, I, -1, enc=enc), R.pack(w, st, O, T, I, -1)), vn
    if O * T * I > 32 * 32:      # an amax taken from block 0 alone (tap 0, the first 32 x 32 channels) misses the last element
        assert R.amax_bits_of(w.reshape(O, T, I)[:32, 0, :32]) != R.bits(R.PACK_AMAX)
    wn = R.pack_weights(O, T, I, 'nan')
    assert R.pack(wn, R.make_state(), O, T, I, 0)[2][2] == R.bits(R.PACK_AMAX)


def test_protocol_tells_the_log2_rule_and_a_missing_clamp_apart():
    """set i: five delayed steps (quantise, then tick) after a just-in-time start"""
    xs = R.protocol_tensors(16 * 257)
    steps = [('quantize', xs[0], R.E4M3, 0), ('tick', R.E4M3, 0)]
    for x in xs:
        steps += [('quantize', x, R.E4M3, 2), ('tick', R.E4M3, 0)]
    ref = R.run_stream(steps)
    scales = [float(R.from_bits(s[0][0])) for st, s in zip(steps, ref) if st[0] == 'tick']
    assert scales == [128.0, 128.0, 2.0, 1024.0, 1024.0, 1024.0, 2.0 ** 126]         # grows, shrinks, kept, kept, clamped
    for vn, rule in RULE_VARIANTS.items():
        got = R.run_stream(steps, rule=rule)
        assert any(not np.array_equal(g[0], r[0]) for g, r in zip(got, ref)), vn
