"""CPU reference of the per-tensor fp8 front end (csrc/igemm_fp8.hip: quantiser, scale update, weight packs), written from
the OCP format definitions and the documented scale rule, not from the kernels.  numpy only; everything is bit patterns.

A scaling state is four 32-bit words, kept here as np.uint32[4]: the float bits of {scale, descale}, the bits of the amax seen
since the last update, and the descale of the weight pack most recently made with the state (csrc/fp8_common.h).

Also here: the input sets of tests/test_gpu_fp8_exact.py, so that tests/test_fp8_ref_cpu.py can show on the CPU that each of
them tells the reference from the wrong variants a kernel could implement."""
import numpy as np

E4M3, E5M2 = 0, 1
FMT_MAX = {E4M3: 448.0, E5M2: 57344.0}
TOP = {E4M3: 0x7e, E5M2: 0x7b}                  # largest finite non-negative code
NAN_CODE = 0x7f                                 # a NaN in both formats
SCALE_KS = (-20, -3, 0, 1, 9)                   # the delayed scales 2^k of the every-bf16-value set
TIE_KS = (0, 7, -5)
INF_BITS = 0x7f800000


def f32(x):
    return np.asarray(x, dtype=np.float32)


def bits(x):
    """float32 value(s) -> uint32 bit pattern(s)"""
    return f32(x).reshape(-1).view(np.uint32).reshape(np.shape(x))


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).reshape(-1).view(np.float32).reshape(np.shape(b))


def pow2(k):
    return np.float32(2.0 ** int(k))


# ---------------------------------------------------------------- the formats
def decode_table(fmt):
    """float64 value of each of the 256 codes: e4m3fn (bias 7, no Inf, NaN = S.1111.111) or e5m2 (bias 15, IEEE Inf / NaN)"""
    mb, bias = (3, 7) if fmt == E4M3 else (2, 15)
    out = np.empty(256, dtype=np.float64)
    for c in range(256):
        e, m = (c & 0x7f) >> mb, c & ((1 << mb) - 1)
        if fmt == E4M3 and (c & 0x7f) == 0x7f:
            v = float('nan')
        elif fmt == E5M2 and e == 31:
            v = float('inf') if m == 0 else float('nan')
        elif e == 0:
            v = m / (1 << mb) * 2.0 ** (1 - bias)
        else:
            v = (1 + m / (1 << mb)) * 2.0 ** (e - bias)
        out[c] = -v if c & 0x80 else v
    return out


def encode(x, fmt):
    """float32 -> code: NaN -> a NaN code, saturate to +-max (Inf included), round to nearest, ties to the even code, by search
    in the decode table in float64 (2a against lo + hi: both sides are exact)"""
    x = f32(x)
    vals = decode_table(fmt)[:TOP[fmt] + 1]
    a = np.minimum(np.abs(x.astype(np.float64)), FMT_MAX[fmt])
    nan = np.isnan(a)
    a = np.where(nan, 0.0, a)
    lo = np.searchsorted(vals, a, side='right') - 1
    hi = np.minimum(lo + 1, TOP[fmt])
    two_a, s = 2.0 * a, vals[lo] + vals[hi]
    up = (two_a > s) | ((two_a == s) & (lo % 2 == 1))
    code = np.where(up, hi, lo)
    code = np.where(nan, NAN_CODE, code)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


# ---------------------------------------------------------------- the scale rule
def scale_exponent(amax_bits, fmt, margin):
    """the largest integer k with amax * 2^margin * 2^k <= fmt_max, for the bits of a positive finite float, in integers"""
    b = int(amax_bits)
    ex, frac = (b >> 23) & 0xff, b & 0x7fffff
    M, e = ((1 << 23) | frac, ex - 150) if ex else (frac, -149)            # amax = M * 2^e
    p = 6 if fmt == E4M3 else 13                                           # fmt_max = 7 * 2^p
    L = M.bit_length()                                                     # M * 2^(3 - L) is in [4, 8)
    fits = (M << (3 - L)) <= 7 if L <= 3 else M <= (7 << (L - 3))
    t = 3 - L if fits else 2 - L                                           # the largest t with M * 2^t <= 7
    return t + p - e - int(margin)


def scale_rule(amax_bits, old_scale, old_descale, fmt, margin):
    """(scale, descale) after a scale update: (2^k, 2^-k) with k = scale_exponent clamped to [-126, 126] iff
    0 < amax < 3.0e38f; otherwise the old pair, or (1, 1) when the old scale is 0"""
    amax = from_bits(np.uint32(amax_bits))
    if amax > 0 and amax < np.float32(3.0e38):
        k = max(-126, min(126, scale_exponent(amax_bits, fmt, margin)))
        return pow2(k), pow2(-k)
    if np.float32(old_scale) == 0:
        return np.float32(1), np.float32(1)
    return np.float32(old_scale), np.float32(old_descale)


def make_state(scale=0.0, descale=0.0, amax_bits=0, word3=0):
    return np.array([bits(np.float32(scale)), bits(np.float32(descale)), amax_bits, word3], dtype=np.uint32)


def tick(state, fmt, margin=0, rule=scale_rule):
    """one scale update of one state: words 0 and 1 by the rule, word 2 cleared, word 3 never written"""
    sc, de = rule(state[2], from_bits(state[0]), from_bits(state[1]), fmt, margin)
    return np.array([bits(sc), bits(de), 0, state[3]], dtype=np.uint32)


# ---------------------------------------------------------------- quantiser and weight pack
def amax_bits_of(x):
    """bits of max |x| over the non-NaN elements (Inf counts); 0 for none"""
    a = np.abs(f32(x).reshape(-1))
    a = a[~np.isnan(a)]
    return int(bits(a.max())) if a.size else 0


def merge_amax(state, ab):
    s = state.copy()
    if ab > 0:
        s[2] = max(int(s[2]), int(ab))                  # unsigned max of bits
    return s


def scaled(x, state):
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        return f32(x) * from_bits(state[0])              # the product rounded to fp32, as the kernel's is


def quantize(x, state, fmt, write, enc=encode, amax=amax_bits_of):
    """-> (bytes | None, record | None, new state); write 0 = amax only, 1 = copy, 2 = copy + its {scale, descale, 0, 0}"""
    q = enc(scaled(x, state), fmt) if write else None
    rec = np.array([state[0], state[1], 0, 0], dtype=np.uint32) if write == 2 else None
    return q, rec, merge_amax(state, amax(x))


def pack(w, state, O, T, I, margin, rule=scale_rule, enc=encode, layout=None):
    """fp32 master [O][T][I] -> (wf [O][T][I], wt [I][T][O], new state), both e4m3.  margin >= 0: amax -> scale rule -> pack;
    margin < 0: pack with state[0].  state[3] = state[1] as of packing; the amax is merged into state[2] either way."""
    w = f32(w).reshape(O, T, I)
    s = state.copy()
    if margin >= 0:
        s = tick(merge_amax(s, amax_bits_of(w)), E4M3, margin, rule)
    s[3] = s[1]
    wf = enc(scaled(w, s), E4M3)
    wt = np.ascontiguousarray(wf.transpose(2, 1, 0)) if layout is None else layout(wf)
    return wf.reshape(-1), wt.reshape(-1), merge_amax(s, amax_bits_of(w))


def run_stream(steps, state=None, rule=scale_rule):
    """The delayed-scaling state machine on ONE state.  steps: ('quantize', x, fmt, write) | ('pack', w, O, T, I, margin) |
    ('tick', fmt, margin).  Returns one (state after the step, bytes or (wf, wt) or None, record or None) per step."""
    s = make_state() if state is None else state.copy()
    out = []
    for st in steps:
        if st[0] == 'quantize':
            q, rec, s = quantize(st[1], s, st[2], st[3])
            out.append((s.copy(), q, rec))
        elif st[0] == 'pack':
            wf, wt, s = pack(st[1], s, st[2], st[3], st[4], st[5], rule=rule)
            out.append((s.copy(), (wf, wt), None))
        elif st[0] == 'tick':
            s = tick(s, st[1], st[2], rule)
            out.append((s.copy(), None, None))
        else:
            raise ValueError(st[0])
    return out


# ---------------------------------------------------------------- input sets of the GPU tests
def bf16_patterns(finite_only=False):
    """every bf16 bit pattern as float32 (exact); finite_only: the non-finite ones replaced by 0"""
    x = from_bits(np.arange(65536, dtype=np.uint32) << 16).copy()
    if finite_only:
        x[~np.isfinite(x)] = 0.0
    return x


def _around(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def tie_values(fmt):
    """fp32 values at which a wrong rounding or saturation shows: the midpoint of every pair of adjacent non-negative finite
    codes with its two fp32 neighbours, max, the float after it, the midpoint to the first unrepresentable step with its
    neighbours, all with both signs, then +-Inf, NaN, +-0"""
    vals = decode_table(fmt)[:TOP[fmt] + 1]
    pos = []
    for c in range(TOP[fmt]):
        pos += _around((vals[c] + vals[c + 1]) / 2)          # (c = 0: half of the smallest subnormal)
    mx = np.float32(FMT_MAX[fmt])
    pos += [mx, np.nextafter(mx, np.float32(np.inf))] + _around(464.0 if fmt == E4M3 else 61440.0)
    pos = f32(pos)
    return np.concatenate([pos, -pos, f32([np.inf, -np.inf, np.nan, 0.0, -0.0])])


def pad16(x):
    return np.concatenate([f32(x), np.zeros(-len(x) % 16, dtype=np.float32)])


def tie_set(fmt, k):
    """tie_values / 2^k padded to a multiple of 16 with zeros: times the scale 2^k they are exact again"""
    return pad16(tie_values(fmt) / pow2(k))


GEOMETRY_NS = (16, 16 * 257, 16 * (1024 * 256 + 773))       # one chunk; two blocks; the capped grid's second trip
GEOMETRY_AMAX = np.float32(300.0)


def geometry_base(n, fmt=E4M3):
    """n fp32 elements of magnitude <= 8 cycling through the small tie values of the format (and their neighbours)"""
    t = tie_values(fmt)
    t = t[np.isfinite(t) & (np.abs(t) <= 8)]
    return np.resize(t, n).astype(np.float32)


def geometry_positions(n):
    """element indices for the unique amax: in the first chunk, in a block other than 0, in the very last chunk"""
    pos = [3]
    if n > 16 * 256:
        pos.append(16 * 256 + 5)
    if n > 16:
        pos.append(n - 16 + 7)
    return pos


def scale_points(fmt):
    """(amax bits, old scale, old descale) of the scale-update test"""
    mx = FMT_MAX[fmt]
    pts = [(0, 0.0, 0.0), (0, 8.0, 0.125)]
    for j in range(-20, 12):
        pts += [(int(bits(v)), 8.0, 0.125) for v in _around(mx * 2.0 ** j)]
    big = np.float32(3.0e38)
    for v in (np.float32(1.0), from_bits(np.uint32(0x00800000)), from_bits(np.uint32(0x00000123)), np.float32(1e-37),
              np.nextafter(big, np.float32(0)), big, np.float32(np.inf)):
        pts.append((int(bits(v)), 8.0, 0.125))
    pts += [(0x7fc00001, 8.0, 0.125), (INF_BITS, 0.0, 0.0), (0x7fc00001, 0.0, 0.0)]
    return pts


def pool_points():
    """(format, amax, old scale, old descale) of the five pool slots of the tick test, in allocation order: three e4m3 and two
    e5m2 slots interleaved, each amax one on which the two formats' rules give different scales or the kept / fresh branch"""
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    return [(E4M3, up(448.0 / 8), 8.0, 0.125), (E5M2, np.float32(1.0), 0.0, 0.0), (E4M3, np.float32(0.0), 0.0, 0.0),
            (E5M2, up(57344.0 * 4), 8.0, 0.125), (E4M3, np.float32(np.inf), 4.0, 0.25)]


PACK_SHAPES = ((32, 1, 32), (64, 9, 96), (160, 9, 128), (128, 16, 32))      # (O, T, I)
PACK_AMAX = np.float32(5.0)                      # -> just-in-time scale 64 (5 * 64 = 320 <= 448 < 640)
PACK_SCALE = 64.0


def pack_weights(O, T, I, variant, seed=0):
    """fp32 [O*T*I]: multiples of 1/8 below 4 mixed with e4m3 tie values / 64, so that w * 2^k is exact.
    variant 'amax_last': the unique amax (5.0, negative) is the very last element, in the last block; 'zero': all zero;
    'nan': as amax_last with one NaN element."""
    n = O * T * I
    if variant == 'zero':
        return np.zeros(n, dtype=np.float32)
    rs = np.random.RandomState(1234 + seed)
    w = (rs.randint(-31, 32, size=n) / 8.0).astype(np.float32)
    t = tie_values(E4M3)
    t = t[np.isfinite(t) & (np.abs(t) <= 256)] / np.float32(PACK_SCALE)
    idx = rs.permutation(n)[:n // 3]
    w[idx] = np.resize(t, idx.size)
    w[-1] = -PACK_AMAX
    if variant == 'nan':
        w[n // 2 + 1] = np.float32(np.nan)
    return w


def protocol_tensors(n, base_amax=2.0):
    """the five tensors (fp32, n elements) of the protocol test after a base tensor: amax x64, x1/512, all zero, one Inf,
    magnitude 1e-37"""
    base = geometry_base(n).copy() / np.float32(8)           # |x| <= 1
    def with_amax(a):
        x = base * np.float32(a / 4)
        x[n // 2] = -np.float32(a)
        return x
    inf = with_amax(base_amax / 8)
    inf[5] = np.float32(np.inf)
    tiny = (np.resize(f32([1.0, -0.5, 0.0, 0.75]), n) * np.float32(1e-37)).astype(np.float32)
    return [with_amax(base_amax), with_amax(base_amax * 64), with_amax(base_amax / 8), np.zeros(n, dtype=np.float32), inf, tiny]
