"""An exact statement of the uint8 pixel rule (oracle/sightpy_oracle.py:srgb_u8; on the device
csrc/rt_device.h resolve_pixel), evaluated with mpmath at 256 bits on the given doubles:

    e_k  = 12.92 c_k                        where c_k <= 0.00304
         = 1.055 c_k^(1/2.4) - 0.055        elsewhere
    peak = max(e_0, e_1, e_2) + 0.00001
    e_k  = e_k / peak                       where peak > 1.0
    q_k  = 255 clip(e_k, 0, 1)              and the byte is floor(q_k)

The constants are the doubles the code uses (12.92, 1.055, 1.0 / 2.4, 0.055, 0.00304, 0.00001 as Python
floats, converted exactly); the two comparisons are evaluated on the exact values (the first is a comparison
of two doubles, the second of the exact peak with 1).

bounds(rgb, eps) gives, per value, lo = floor(max(q - eps, 0)) and hi = floor(q + eps): every evaluation of
the rule in float64 whose error stays below eps lands in [lo, hi], and where lo == hi (the value is
*unambiguous*) there is one right byte.

eps.  With u = 2^-53 and a pow within 2 ulp (relative error <= 4u):
  * power branch: fl(c^(1/2.4)) = a (1 + d1), |d1| <= 4u; the product by 1.055 adds u, so t = 1.055 a carries
    an absolute error <= 5u t; the subtraction rounds once more: |fl(e) - e| <= 5u t + u e.  Without the
    normalisation only e <= 1 matters beyond the clip, so t <= 1.055 and |fl(e) - e| <= (5.275 + 1) u < 6.3u.
    The linear branch is one rounding, far below that.
  * q = fl(255 e): 255 * 6.3u + one rounding of a value <= 255: |fl(q) - q| <= 255 * 7.3u = 1862u = 2.1e-13.
  * with the peak division: the largest e has the relative error (5 t + m) u / m <= 6.3u (m >= 1 - 1e-5), the
    sum with 0.00001 rounds once: peak within 7.3u relative.  The quotient e_k / peak <= 1 then carries
    6.3u + 7.3u + u (the division) = 14.6u absolute, and q 255 * 15.6u = 3978u = 4.5e-13.
  * a float64 peak on the other side of 1.0 than the exact one (they differ by <= 7.3u) divides, or does
    not, by a number within 1e-15 of 1: 255 * 7.3u on top of the un-normalised 2.1e-13, still 4.2e-13.
So EPS = 5e-13.  It is derived, not fitted: numpy's own evaluation stays within 8.4e-14 of q on the values
below.  A level's boundary is hit, at this eps, by about 1e-12 of all values: a rendered frame has no
ambiguous value, the boundary table (built to sit on the boundaries) about half.

Non-finite and negative inputs are not classified (bounds raises on them): what they give is the
behaviour of numpy's where / amax / clip / astype(uint8) on NaN, stated as the explicit table SPECIALS."""
import numpy as np
from mpmath import MPContext

EPS = 5e-13

_mp = MPContext()
_mp.prec = 256
_C1292, _C1055, _C0055 = _mp.mpf(12.92), _mp.mpf(1.055), _mp.mpf(0.055)
_P, _T, _CPEAK = _mp.mpf(1.0 / 2.4), 0.00304, _mp.mpf(0.00001)
_ZERO, _ONE = _mp.mpf(0), _mp.mpf(1)

# the highest level of the linear branch: q(0.00304) = 255 * 12.92 * 0.00304 = 10.0155
LINEAR_LEVELS = 10

# (pixel, bytes): numpy's srgb_u8 on this CPU, both the oracle's and the kernels' rule
SPECIALS = [
    # NaN -> 0 in its channel; the peak is NaN, NaN > 1.0 is false: the other channels are NOT normalised
    # (4.0 clips to 255 and 0.25 keeps its own 136; normalised they would be 254 and 75)
    ((np.nan, 4.0, 0.25), (0, 255, 136)),
    ((0.25, np.nan, np.nan), (136, 0, 0)),
    ((4.0, 0.25, np.nan), (255, 136, 0)),
    ((np.nan, np.inf, 0.25), (0, 255, 136)),
    # inf -> inf / inf = NaN -> 0; the finite channels are divided by inf -> 0
    ((np.inf, 4.0, 0.25), (0, 0, 0)),
    ((0.25, np.inf, np.inf), (0, 0, 0)),
    # negative values (the linear branch, below the clip) and -0.0 -> 0; the others as without them
    ((-1.0, 0.25, 0.0), (0, 136, 0)),
    ((-1.0, 4.0, 0.25), (0, 254, 75)),
    ((-1e300, 0.0, 0.25), (0, 0, 136)),
    ((-np.inf, 0.25, 0.0), (0, 136, 0)),
    ((-0.0, 0.25, -0.0), (0, 136, 0)),
    ((-0.0, -0.0, -0.0), (0, 0, 0)),
]


def specials():
    """SPECIALS as (rgb (3, n) float64, bytes (n, 3) uint8)."""
    rgb = np.array([p for p, _ in SPECIALS], dtype=np.float64).T.copy()
    return rgb, np.array([b for _, b in SPECIALS], dtype=np.uint8)


def _e(x, memo):
    v = memo.get(x)
    if v is None:
        X = _mp.mpf(x)
        v = _C1292 * X if x <= _T else _C1055 * _mp.power(X, _P) - _C0055
        memo[x] = v
    return v


def exact_q(pixel, memo=None):
    """(q_0, q_1, q_2) of one pixel of three finite, non-negative Python floats, as mpf."""
    memo = {} if memo is None else memo
    e = [_e(x, memo) for x in pixel]
    peak = max(e) + _CPEAK
    assert abs(peak - _ONE) > _mp.mpf(2) ** -200  # (the comparison below is decided)
    if peak > _ONE:
        e = [v / peak for v in e]
    return [255 * min(max(v, _ZERO), _ONE) for v in e]


def classify(rgb, eps=EPS):
    """(lo, hi, floor(q)) as int arrays (n, 3) for linear RGB (3, n), float64."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.float64 or rgb.ndim != 2 or rgb.shape[0] != 3:
        raise ValueError("rgb must be float64 of shape (3, n)")
    if not np.isfinite(rgb).all() or (rgb < 0.0).any() or np.signbit(rgb).any():
        raise ValueError("non-finite and negative inputs are not classified: see SPECIALS")
    n = rgb.shape[1]
    lo, hi, fl = (np.empty((n, 3), dtype=np.int64) for _ in range(3))
    e = _mp.mpf(eps)
    memo = {}
    cols = rgb.T.tolist()
    for i, px in enumerate(cols):
        if len(memo) > 4096:
            memo.clear()
        for k, q in enumerate(exact_q(px, memo)):
            lo[i, k] = int(_mp.floor(max(q - e, _ZERO)))
            hi[i, k] = int(_mp.floor(q + e))
            fl[i, k] = int(_mp.floor(q))
    return lo, hi, fl


def bounds(rgb, eps=EPS):
    """(lo, hi): int arrays (n, 3); a value is ambiguous where lo != hi."""
    lo, hi, _ = classify(rgb, eps)
    return lo, hi


# ---- the boundary table -----------------------------------------------------------------------------------
OFFSETS = [0] + [s * (1 << b) for b in range(13) for s in (1, -1)]  # 0, +-1, +-2, +-4, ..., +-4096


def _smallest_reaching(k, guess, q_of):
    """The smallest double x with q_of(x) >= k (q_of monotone), from a guess a few ulps away."""
    x = float(guess)
    while q_of(x) >= k:
        x = float(np.nextafter(x, -np.inf))
    while q_of(x) < k:
        x = float(np.nextafter(x, np.inf))
    return x


def level_starts():
    """x_k for k = 1 .. 254: the smallest double whose exact q (alone in its pixel, or in all three channels:
    no normalisation below level 255) reaches k.  Levels <= LINEAR_LEVELS lie on the linear branch."""
    out = []
    for k in range(1, 255):
        K = _mp.mpf(k) / 255
        guess = K / _C1292 if k <= LINEAR_LEVELS else _mp.power((K + _C0055) / _C1055, 1 / _P)
        x = _smallest_reaching(k, guess, lambda v: exact_q((v, 0.0, 0.0))[0])
        assert (x <= _T) == (k <= LINEAR_LEVELS)
        out.append(x)
    return np.array(out)


BRIGHT = [16.0, 1e3, 1e6, 1e12, 1e20]  # far above 1 and still capped below 255 (never_255)


def table_values():
    """The doubles of the boundary table: every level's start and its neighbours at OFFSETS ulps, the branch
    point and its neighbours, 0, the smallest subnormal, 1, 1 - 1e-5 and its neighbours, 1e300, BRIGHT."""
    xs = level_starts()
    sp = np.spacing(xs)
    vals = [xs + o * sp for o in OFFSETS]
    t, c = 0.00304, 1.0 - 1e-5
    extra = [t, np.nextafter(t, 0.0), np.nextafter(t, 1.0), 0.0, 5e-324, 1.0, c, np.nextafter(c, 0.0),
             np.nextafter(c, 2.0), 1e300] + BRIGHT
    return np.concatenate(vals + [np.array(extra)])


def never_255(rgb):
    """The pixels (columns of rgb (3, n)) that cannot give a byte 255: the rule caps a finite pixel at
    255 m / (m + 1e-5) with m its largest e.  The cap is within EPS of 255 only from m ~ 5.1e9 on (an input
    ~ 2e23; in float64 m + 1e-5 == m from m ~ 9e10 on, and numpy's own result for 1e300 is 255), so every pixel
    of finite values <= 4e20 (m ~ 4e8) stays at 254 or below."""
    return np.isfinite(rgb).all(axis=0) & (rgb.max(axis=0) <= 4e20)


def branch_probes():
    """Pixels (M, x, 0) that pin the branch point 0.00304 itself.  Between 0.00304 and the sRGB standard's
    0.0031308 the two branches differ by ~1e-5 and q runs from 10.02 to 10.32 on either: alone in its pixel no
    byte tells them apart.  Divided by the right peak it does: M is chosen so that level 10 starts between
    255 * 12.92 x / peak and 255 * (1.055 x^(1/2.4) - 0.055) / peak.  The rule (power branch) gives 10, a branch
    point above x would give 9."""
    out = []
    for x in (float(np.nextafter(0.00304, 1.0)), 0.00305, 0.00308, 0.0031):
        mid = 0.5 * (12.92 * x + (1.055 * x ** (1.0 / 2.4) - 0.055))
        peak = 255.0 * mid / 10.0
        out.append((((peak - 0.00001 + 0.055) / 1.055) ** 2.4, x, 0.0))
    return np.array(out).T.copy()


NORMALISED_PEAK_INPUT = 4.0
NORMALISED_OFFSETS = [0, 1, -1, 16, -16, 4096, -4096]


def normalised_level_starts():
    """Pixels (4, x, 0) (3, n): the peak is e(4) + 1e-5 = 1.825, and x is, for k = 1 .. 254, the smallest double
    whose exact 255 e(x) / peak reaches k, and its neighbours at NORMALISED_OFFSETS ulps: the level boundaries of
    the normalised regime, where the byte depends on the division."""
    M = NORMALISED_PEAK_INPUT
    peak = _e(M, {}) + _CPEAK
    xs = []
    for k in range(1, 255):
        e = _mp.mpf(k) / 255 * peak
        guess = e / _C1292 if e <= _C1292 * _mp.mpf(_T) else _mp.power((e + _C0055) / _C1055, 1 / _P)
        xs.append(_smallest_reaching(k, guess, lambda v: exact_q((M, v, 0.0))[1]))
    xs = np.array(xs)
    assert (np.diff(xs) > 0).all() and xs[-1] < M
    x = np.concatenate([xs + o * np.spacing(xs) for o in NORMALISED_OFFSETS])
    return np.stack([np.full(len(x), M), x, np.zeros(len(x))])


def boundary_table():
    """Linear RGB (3, n): table_values() placed three ways -- alone in one channel (the channel rotating,
    the other two black), in all three channels, and as (4x, 2x, x), which is normalised (peak > 1) from
    x ~ 0.27 up and so divides the table's values by a peak -- then normalised_level_starts() and
    branch_probes()."""
    v = table_values()
    n = len(v)
    single = np.zeros((3, n))
    single[np.arange(n) % 3, np.arange(n)] = v
    with np.errstate(over="ignore"):
        scaled = np.stack([4.0 * v, 2.0 * v, v])
    scaled[~np.isfinite(scaled)] = 1e300  # (4e300 is finite; kept finite whatever the table holds)
    return np.ascontiguousarray(np.concatenate([single, np.stack([v, v, v]), scaled, normalised_level_starts(),
                                                branch_probes()], axis=1))


def random_pixels(seed=20240607, n=6000):
    """Seeded linear RGB (3, n): a third uniform in [0, 4), a third log-uniform from 1e-6 to 1e3, a third
    uniform in [0, 1) (where un-normalised pixels live)."""
    rng = np.random.default_rng(seed)
    m = n // 3
    a = rng.uniform(0.0, 4.0, (3, m))
    b = 10.0 ** rng.uniform(-6.0, 3.0, (3, m))
    c = rng.uniform(0.0, 1.0, (3, n - 2 * m))
    return np.ascontiguousarray(np.concatenate([a, b, c], axis=1))


# ---- one frame holding everything, classified once ----------------------------------------------------------
FRAME_W = 67
_FRAME = {}


def frame():
    """The boundary table, the random set and SPECIALS as one frame of width FRAME_W (the last row padded with
    zeros), classified once per process: {"rgb" (3, n), "W", "H", "table", "random", "special" (slices of the
    pixels), "finite" (mask (n,): the classified pixels), "lo", "hi", "floor" (n, 3; rows of the special pixels
    hold SPECIALS' bytes in all three), "special_bytes"}."""
    if _FRAME:
        return _FRAME
    tab, rnd = boundary_table(), random_pixels()
    spc, spc_bytes = specials()
    n0 = tab.shape[1] + rnd.shape[1] + spc.shape[1]
    H = (n0 + FRAME_W - 1) // FRAME_W
    n = H * FRAME_W
    rgb = np.zeros((3, n))
    rgb[:, :n0] = np.concatenate([tab, rnd, spc], axis=1)
    table = slice(0, tab.shape[1])
    random = slice(table.stop, table.stop + rnd.shape[1])
    special = slice(random.stop, n0)
    finite = np.ones(n, dtype=bool)
    finite[special] = False
    lo, hi, fl = (np.empty((n, 3), dtype=np.int64) for _ in range(3))
    lo[finite], hi[finite], fl[finite] = classify(np.ascontiguousarray(rgb[:, finite]))
    lo[special] = hi[special] = fl[special] = spc_bytes
    _FRAME.update(rgb=rgb, W=FRAME_W, H=H, table=table, random=random, special=special, finite=finite, lo=lo,
                  hi=hi, floor=fl, special_bytes=spc_bytes)
    return _FRAME


def check_bytes(u8, lo, hi, what=""):
    """lo <= u8 <= hi everywhere (so u8 == lo on every unambiguous value), reporting the first offenders.
    Returns the number of values that needed the band: u8 != lo."""
    u = np.asarray(u8).reshape(-1, 3).astype(np.int64)
    assert u.shape == lo.shape, (what, u.shape, lo.shape)
    bad = np.argwhere((u < lo) | (u > hi))
    assert len(bad) == 0, "%s: %d values outside [lo, hi], first (pixel, channel, byte, lo, hi): %s" % (
        what, len(bad), [(int(p), int(k), int(u[p, k]), int(lo[p, k]), int(hi[p, k])) for p, k in bad[:8]])
    unamb = lo == hi
    assert np.array_equal(u[unamb], lo[unamb]), what
    return int((u != lo).sum())
