"""Exact-operand reference for the BatchNorm kernels (csrc/bn.hip), in the style of conv_exact_ref.py.

The backward takes save_mean and save_invstd as INPUTS.  With integer x and dy, integer means and power-of-two invstd and
gamma, every value it forms is a dyadic rational fp32 holds exactly: xhat = (x - mean) * invstd is an integer, both sums
s1 = sum dy_eff and s2 = sum dy_eff * xhat are integers in any order, k1 = s1 * (1 / rows) and k2 = s2 * (1 / rows) are exact
when rows is a power of two, and k0 * (g - k1 - xhat * k2) is exact with or without FMA contraction.  A correct kernel then
returns the float64 result BIT FOR BIT on every path (reduce / finalize / apply, the one-launch LDS-resident kernel, the
`*_partials` entry points); the bf16 expectation of dx is the round-to-nearest-even of that exact value.

Range condition (asserted by check_exact, never assumed): x, dy, the residual and y are values of the activation type;
sum |dy_eff| and sum |dy_eff * xhat| stay below 2^24 per channel (so every partial sum in every order is an fp32 integer);
s1, s2, k0, k1, k2, xhat * k2, g - k1, g - k1 - xhat * k2 and the product with k0 survive a float32 round trip.  The
per-element intermediates depend on (g, xhat, channel) only, so they are checked over ALL 7 x 5 combinations of every
channel: a superset of the combinations a case holds.

Generator, per channel: mean an integer in [-4, 4]; invstd = 2^-j, j in {0, 1, 2}; gamma in {+-0.5, +-1, +-2} (negative
gamma flips the mask recomputed from x); beta in {-1, -0.5, 0, 0.5, 1}.  Per element: xhat an integer in {-2..2} and
x = mean + xhat / invstd (|x| <= 12), dy an integer in {-3..3}, the residual an integer in {-4..4}.  Then the forward's
pre-activation xhat * gamma + beta is exact and about a tenth of the elements sit at exactly 0, where the strict `> 0` of
every mask source decides.

Everything is float64 torch on the device of the operands (CPU in test_bn_exact_cpu.py; the GPU tests compute the same
functions with torch's float64 there, so that 16 M-element cases stay within seconds).  Matrices are [rows][C], the NHWC
memory order; nchw() gives the logical NCHW view the ops take.
"""
import zlib

import numpy as np
import torch

F32_EXACT = float(1 << 24)
U32 = 2.0 ** -24             # unit roundoff of fp32
EPS = 1e-5
MOMENTUM = float(np.float32(0.1))     # the kernels hold the momentum as a float

# rows -> (N, H, W): every row count the case tables use
GEOM = {1: (1, 1, 1), 2: (2, 1, 1), 3: (1, 3, 1), 16: (1, 4, 4), 256: (4, 8, 8), 315: (5, 7, 9), 512: (2, 16, 16),
        1000: (10, 10, 10), 1024: (4, 16, 16), 4096: (4, 32, 32), 4099: (1, 4099, 1), 8192: (8, 32, 32),
        16384: (16, 32, 32), 16400: (16, 25, 41), 32768: (32, 32, 32)}
PER = {'bf16': 8, 'f32': 4}           # elements per 16-byte chunk = per byte of a ReLU bit mask
TDT = {'bf16': torch.bfloat16, 'f32': torch.float32}


def nchw(mat):
    """[rows][C] matrix (NHWC memory order) -> logical NCHW view of the same memory."""
    rows, C = mat.shape
    N, H, W = GEOM[rows]
    return mat.view(N, H, W, C).permute(0, 3, 1, 2)


def rows_of(t):
    """logical NCHW tensor -> [rows][C] matrix in NHWC order."""
    N, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(N * H * W, C)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).double()


# ---------------------------------------------------------------- operands
def make_case(rows, C, device='cpu', mirror=False):
    """Exact operands of one (rows, C) problem.  mirror: the second half of the rows repeats the first with dy negated, so
    that both sums vanish for a mask that depends on x alone (dx = k0 * g: exact in e5m2, for the fp8 side output)."""
    rng = _rng('case', rows, C, mirror)
    mean = rng.integers(-4, 5, size=C)
    j = rng.integers(0, 3, size=C)
    gamma = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), size=C)
    beta = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), size=C)
    xhat = rng.integers(-2, 3, size=(rows, C), dtype=np.int8)
    dy = rng.integers(-3, 4, size=(rows, C), dtype=np.int8)
    res = rng.integers(-4, 5, size=(rows, C), dtype=np.int8)
    if mirror:
        assert rows % 2 == 0
        h = rows // 2
        xhat[h:], dy[h:], res[h:] = xhat[:h], -dy[:h], res[:h]
    c = dict(rows=rows, C=C, mean=_t(mean, device), invstd=_t(0.5 ** j, device), gamma=_t(gamma, device), beta=_t(beta, device),
             xhat=_t(xhat, device), dy=_t(dy, device), res=_t(res, device))
    c['x'] = c['mean'] + c['xhat'] / c['invstd']
    c['ypre'] = c['xhat'] * c['gamma'] + c['beta']
    return c


def stats_case(rows, C, device='cpu'):
    """Forward-statistics operands that notice one row: x = mean_c + d, d in {-3, -2, 2, 3} (no small deviations: dropping or
    doubling any single row of <= 4096 moves the channel mean by at least 2 / 4096 = 4.9e-4).  mean_c is an integer in
    +-{1..4}, never 0: the statistics tolerance is relative, at a mean of 0 only its atol = 1e-6 would remain, which is the
    size of the fp32 Welford / Chan arithmetic's own error and leaves the reference no room; at |mean| >= 1 the smallest
    tolerance is 1.1e-5, ten times that error and forty times below what a lost row moves."""
    rng = _rng('stats', rows, C)
    mean = rng.integers(1, 5, size=C) * (rng.integers(0, 2, size=C) * 2 - 1)
    d = rng.choice(np.array([-3, -2, 2, 3], dtype=np.int8), size=(rows, C))
    return dict(rows=rows, C=C, mean_c=_t(mean, device), x=_t(mean, device) + _t(d, device),
                gamma=_t(rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), size=C), device),
                beta=_t(rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), size=C), device))


def int_prior(C, tag, device='cpu'):
    """Integer prior values of dgamma / dbeta / a column sum for the `accumulate` forms."""
    return _t(_rng('prior', C, tag).integers(-8, 9, size=C), device)


def mask_bytes(n, tag):
    return torch.from_numpy(_rng('mask', n, tag).integers(0, 256, size=n).astype(np.uint8))


# ---------------------------------------------------------------- ReLU masks
def pack_mask(m, per):
    """bool [rows][C] -> uint8 [rows * C / per]: byte i covers NHWC chunk i, bit e its element e."""
    w = (1 << torch.arange(per, device=m.device, dtype=torch.int32))
    return (m.reshape(-1, per).to(torch.int32) * w).sum(1).to(torch.uint8)


def unpack_mask(b, rows, C, per):
    bits = (b.view(-1, 1).to(torch.int32) >> torch.arange(per, device=b.device, dtype=torch.int32).view(1, per)) & 1
    return bits.view(rows, C).bool()


def fwd_y(c, residual, relu):
    """The forward output of the case's own statistics: exact."""
    y = c['ypre'] + c['res'] if residual else c['ypre']
    return torch.clamp(y, min=0.0) if relu else y


def relu_mask(c, source):
    """The mask the backward applies for mask source 0 (none), 1 (y > 0, y = relu(ypre + residual) as stored), 2 (recomputed
    from x: ypre > 0, the residual is not seen) and 3 (a given bit mask: here the bits of source 1).  Strict: a
    pre-activation of exactly 0 passes no gradient."""
    if source == 0:
        return None
    if source == 2:
        return c['ypre'] > 0
    return fwd_y(c, True, True) > 0


# ---------------------------------------------------------------- references
def bn_bwd(c, mask=None, prior_dgamma=None, prior_dbeta=None):
    """float64 backward from save_mean / save_invstd: dx, dres (= the masked dy), dgamma, dbeta and the named intermediates."""
    g = c['dy'] if mask is None else c['dy'] * mask
    xhat = (c['x'] - c['mean']) * c['invstd']
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    k0, k1, k2 = c['gamma'] * c['invstd'], s1 / c['rows'], s2 / c['rows']
    dx = k0 * (g - k1 - xhat * k2)
    return dict(dx=dx, dres=g, dbeta=s1 + (0 if prior_dbeta is None else prior_dbeta), dgamma=s2 + (0 if prior_dgamma is None else prior_dgamma),
                g=g, xhat=xhat, s1=s1, s2=s2, k0=k0, k1=k1, k2=k2)


def dx_bound(r):
    """Per-element bound of an fp32 evaluation of dx when rows is no power of two (1.0f / rows is rounded): 8 units of
    roundoff on the magnitudes the formula combines."""
    return 8 * U32 * r['k0'].abs() * (r['g'].abs() + r['k1'].abs() + (r['xhat'] * r['k2']).abs())


def train_fwd(x, gamma, beta, res=None, relu=False, eps=EPS, momentum=MOMENTUM, rm0=None, rv0=None, repeats=0):
    """float64 training forward over [rows][C]: batch statistics (biased variance for invstd, unbiased for the running
    variance), y, the pre-ReLU sign bits and the running statistics after `repeats` momentum updates."""
    n = x.shape[0]
    mean = x.mean(0)
    m2 = ((x - mean) ** 2).sum(0)
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + eps)
    ypre = (x - mean) * (gamma * invstd) + beta
    if res is not None:
        ypre = ypre + res
    out = dict(mean=mean, var=var, invstd=invstd, ypre=ypre, mask=ypre > 0, y=torch.clamp(ypre, min=0.0) if relu else ypre)
    if rm0 is not None:
        out['rm'], out['rv'] = running(mean, m2, n, rm0, rv0, momentum, repeats)
    return out


def running(mean, m2, n, rm0, rv0, momentum=MOMENTUM, repeats=1):
    uvar = m2 / (n - 1) if n > 1 else m2 / n
    rm, rv = rm0.clone(), rv0.clone()
    for _ in range(repeats):
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * uvar
    return rm, rv


def eval_fwd(x, gamma, beta, rm, rv, res=None, relu=False, eps=EPS):
    y = (x - rm) * (gamma / torch.sqrt(rv + eps)) + beta
    if res is not None:
        y = y + res
    return torch.clamp(y, min=0.0) if relu else y


def colsum(dy, prior=None):
    s = dy.sum(0)
    return s if prior is None else s + prior


def apply_relu_mask(g, b, per):
    rows, C = g.shape
    return g * unpack_mask(b, rows, C, per)


def rne(v, dt):
    """float64 -> the activation type, round to nearest even (through fp32, which holds every expected value exactly or
    is the type itself), back as float64 for comparisons."""
    return v.float().to(TDT[dt]).double()


# ---------------------------------------------------------------- the range condition
def _f32_exact(name, v):
    assert torch.equal(v.float().double(), v), '%s does not survive a float32 round trip' % name


def check_exact(c, mask, dt, prior_dgamma=None, prior_dbeta=None, pow2_rows=True):
    """Assert (not assume) that fp32 arithmetic in any order returns the float64 backward of this case exactly."""
    for k in ('x', 'dy', 'res'):
        assert torch.equal(rne(c[k], dt), c[k]), '%s is not a %s value' % (k, dt)
    assert torch.equal(rne(fwd_y(c, True, True), dt), fwd_y(c, True, True)), 'y is not a %s value' % dt
    r = bn_bwd(c, mask, prior_dgamma, prior_dbeta)
    assert torch.equal(r['xhat'], c['xhat']), 'xhat is not the generated integer'
    assert float(r['g'].abs().sum(0).max()) < F32_EXACT and float((r['g'] * r['xhat']).abs().sum(0).max()) < F32_EXACT
    for k in ('s1', 's2', 'k0', 'dgamma', 'dbeta'):
        _f32_exact(k, r[k])
        assert float(r[k].abs().max()) < F32_EXACT
    assert torch.equal(r['s1'], r['s1'].round()) and torch.equal(r['s2'], r['s2'].round())
    if not pow2_rows:
        return r
    rows = c['rows']
    assert rows & (rows - 1) == 0
    _f32_exact('k1', r['k1']); _f32_exact('k2', r['k2'])
    dev = c['x'].device
    g = torch.arange(-3, 4, dtype=torch.float64, device=dev).view(7, 1, 1)          # every dy_eff, masked (0) included
    xh = torch.arange(-2, 3, dtype=torch.float64, device=dev).view(1, 5, 1)         # every xhat
    k0, k1, k2 = r['k0'].view(1, 1, -1), r['k1'].view(1, 1, -1), r['k2'].view(1, 1, -1)
    _f32_exact('xhat*k2', xh * k2)
    _f32_exact('g-k1', g - k1)
    _f32_exact('g-k1-xhat*k2', g - k1 - xh * k2)
    _f32_exact('k0*(g-k1-xhat*k2)', k0 * (g - k1 - xh * k2))
    _f32_exact('fma(-xhat, k2, g-k1) operands', (-xh) * k2)
    _f32_exact('dx', r['dx'])
    return r


# ---------------------------------------------------------------- crafted partials
def fwd_partials(x, bounds):
    """Forward statistics partials [nslices][C][(n, mean, M2)] in float64 of the row partition `bounds` (a list of (r0, r1);
    r0 == r1 gives the empty slice n = 0, mean = 0, M2 = 0)."""
    out = torch.zeros(len(bounds), x.shape[1], 3, dtype=torch.float64, device=x.device)
    for i, (r0, r1) in enumerate(bounds):
        if r1 > r0:
            s = x[r0:r1]
            m = s.mean(0)
            out[i, :, 0], out[i, :, 1], out[i, :, 2] = r1 - r0, m, ((s - m) ** 2).sum(0)
    return out


def combine_fwd_partials(p):
    """float64 combination of [nslices][C][3] partials: (n, mean, M2) per channel."""
    n = p[:, :, 0].sum(0)
    mean = (p[:, :, 0] * p[:, :, 1]).sum(0) / n
    m2 = (p[:, :, 2] + p[:, :, 0] * (p[:, :, 1] - mean) ** 2).sum(0)
    return n, mean, m2


def sliced_stats_partials(nslices, C, device='cpu'):
    """[nslices][C][3] partials of 64-row slices of a tensor x = mean_c + d, about a tenth of the slices empty.  The
    deviations of one slice share a sign (d in {2, 3} or in {-3, -2}, the sign alternating over the non-empty slices), so every
    slice mean sits at least 2 from the overall mean and ONE lost slice moves the mean by at least
    64 * 2 / (64 * 4097) = 4.9e-4, twelve times the tolerance -- whichever slice it is (test_bn_exact_cpu.py checks each).
    n, mean (a multiple of 1/64) and M2 = sum d^2 - (sum d)^2 / 64 are exact in fp32."""
    rng = _rng('sliced', nslices, C)
    mean_c = rng.integers(1, 5, size=C) * (rng.integers(0, 2, size=C) * 2 - 1)
    full = rng.random(nslices) >= 0.1
    if not full.any():
        full[nslices // 2] = True
    sign = np.zeros(nslices, dtype=np.int64)
    sign[full] = 1 - 2 * (np.arange(int(full.sum())) % 2)
    d = rng.integers(2, 4, size=(nslices, 64, C)).astype(np.int64) * sign[:, None, None]
    sd, sq = d.sum(1).astype(np.float64), (d * d).sum(1).astype(np.float64)
    p = np.zeros((nslices, C, 3))
    p[:, :, 0] = 64.0 * full[:, None]
    p[:, :, 1] = (mean_c[None, :] + sd / 64.0) * full[:, None]
    p[:, :, 2] = sq - sd * sd / 64.0
    p = torch.from_numpy(p).to(device)
    _f32_exact('forward partials', p)
    return p


def bwd_partials(s1, s2, nslices, tag):
    """Backward partials [nslices][C][2] of arbitrary integers (either sign) that add up to the true s1 and s2; the sum of
    their magnitudes stays below 2^24, so fp32 adds them exactly in any order."""
    C = s1.numel()
    rng = _rng('bwdp', nslices, C, tag)
    p = rng.integers(-1000, 1001, size=(nslices, C, 2)).astype(np.float64)
    p = torch.from_numpy(p).to(s1.device)
    p[nslices - 1] = 0
    p[nslices - 1, :, 0] = s1 - p[:, :, 0].sum(0)
    p[nslices - 1, :, 1] = s2 - p[:, :, 1].sum(0)
    assert float(p.abs().sum(0).max()) < F32_EXACT
    return p


# ---------------------------------------------------------------- case tables (read by both test files)
# a. backward, rows a power of two: (rows, C, dtype), the smallest shapes that reach each edge
BWD_SHAPES = [
    (2, 64, 'bf16'), (2, 64, 'f32'),              # resident: one row or none per block; three-launch: one short slice
    (256, 64, 'bf16'), (256, 64, 'f32'),          # resident: one row per block
    (1024, 64, 'bf16'), (1024, 64, 'f32'),        # 4 rows per block: fewer rows than row lanes
    (16384, 64, 'bf16'), (16384, 64, 'f32'),      # 64 rows per block; three-launch: many slices
    (256, 8, 'bf16'), (256, 4, 'f32'),            # narrowest C, TX = 1, not resident
    (1024, 192, 'bf16'), (1024, 24, 'f32'),       # TX does not divide cpr: the second column group is partly empty
    (512, 4096, 'bf16'),                          # cpr = 512: two full column groups, G = 64
    (8192, 2048, 'bf16'), (8192, 1024, 'f32'),    # 32 MB per tensor, 1024 rows per block: the streamed remainder of both passes
    (256, 16384, 'bf16'),                         # G = the CU count, R = 1
]
# b. backward, ragged row counts (1.0f / rows is rounded: dx within the derived bound, the sums still exact)
RAGGED_SHAPES = [(r, 64, dt) for r in (1, 3, 315, 1000, 4099) for dt in ('bf16', 'f32')] + [(315, 192, 'bf16')]
# (relu source, want_dres, accumulate)
BWD_MODES = [(0, False, False), (0, False, True), (1, False, False), (1, True, False), (1, False, True), (1, True, True),
             (2, False, False), (2, False, True), (3, False, False), (3, True, False), (3, False, True), (3, True, True)]
RAGGED_MODES = [(0, False, False), (1, True, True), (2, False, True), (3, True, False)]


def resident_eligible(C, dt):
    """The one-launch form covers whole 64 (bf16) / 32 (fp32) channel groups, at most one per CU (256)."""
    gc = 8 * PER[dt]
    return C % gc == 0 and C // gc <= 256


def bwd_cases(shapes, modes):
    """(rows, C, dtype, form, relu, want_dres, accumulate); mask source 1 is never resident (`relu != 1` in the dispatch)."""
    out = []
    for rows, C, dt in shapes:
        for form in ('three', 'resident'):
            if form == 'resident' and not resident_eligible(C, dt):
                continue
            for relu, dres, acc in modes:
                if form == 'resident' and relu == 1:
                    continue
                out.append((rows, C, dt, form, relu, dres, acc))
    return out


def case_id(c):
    return '-'.join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


# c. mi355_bn_bwd_partials: (nslices, rows, C, dtype, relu, want_dres, accumulate)
BWD_PARTIAL_NSLICES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
BWD_PARTIAL_CASES = [(ns, rows, C, dt, relu, dres, acc) for rows, C in ((256, 64), (256, 8)) for dt in ('bf16', 'f32')
                     for ns in BWD_PARTIAL_NSLICES for relu, dres, acc in ((0, False, False), (3, True, True))]
# d. forward statistics
STATS_SHAPES = [(2, 64, 'bf16'), (2, 64, 'f32'), (256, 8, 'bf16'), (256, 4, 'f32'), (315, 64, 'bf16'), (315, 64, 'f32'),
                (1000, 192, 'bf16'), (1000, 24, 'f32'), (4096, 64, 'bf16'), (4096, 64, 'f32'), (512, 4096, 'bf16')]
STAT_UPDATES = [0, 1, 3]
# e. forward apply / eval forward / mask bits
APPLY_SHAPES = [(315, 64, 'bf16'), (315, 64, 'f32'), (1000, 192, 'bf16'), (1000, 24, 'f32'), (512, 4096, 'bf16'),
                (32768, 64, 'bf16'), (32768, 64, 'f32')]
APPLY_MODES = [(False, False), (False, True), (True, True)]          # (residual, relu)
# f. mi355_bn_train_fwd_partials
FWD_PARTIAL_NSLICES = [1, 63, 64, 65, 511, 512, 513, 1024, 1025, 2048, 2049, 4097]
FWD_PARTIAL_CASES = [(ns, C, dt) for dt, Cs in (('bf16', (8, 64)), ('f32', (4, 64))) for C in Cs for ns in FWD_PARTIAL_NSLICES]
# g. column sums over the shapes of a. and b.; apply_relu_mask
COLSUM_SHAPES = BWD_SHAPES + RAGGED_SHAPES
MASK_APPLY_SHAPES = [(315, 64, 'bf16'), (315, 64, 'f32'), (16400, 512, 'bf16')]      # the last: 1 049 600 chunks > 4096 * 256
# h. fp8 side outputs (bf16 only)
FP8_SHAPES = [(256, 16), (1024, 128), (1024, 192)]
