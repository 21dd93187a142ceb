"""Corrupted blocks by second-difference level: the exact reference of si_burst_runs and the case builders of
tests/test_burst_ref.py and tests/test_gpu_burst.py.  A plain module, imported by name; importing it needs no GPU.

The contract, for one channel x[0 .. n) and h = half.  x is fp32, int16, or int32 holding 24-bit values (the device gets them packed):
    T         max(thr, fl32(rel * peak)): tests/dead_ref.py's threshold_ref (the peak over the finite samples; rel == 0: T = thr)
    d(k)      for 1 <= k <= n - 2 only.  PCM: x[k - 1] - 2 x[k] + x[k + 1] in integers, sq = d^2, an integer.
              fp32: D = fl64(fl64((double)x[k - 1] + (double)x[k + 1]) - 2 (double)x[k]), sq = fl64(D D): numpy float64 steps.
    bad(k)    any of x[k - 1], x[k], x[k + 1] is NaN or +-inf; sq counts as 0
    W(i)      [max(1, i - h), min(n - 2, i + h)], cnt(i) = |W(i)|, which may be 0
    E(i)      the sum of sq over W(i) -- here EXACT: Python integers (an fp32 D is a multiple of 2^-149, a float64 square of 2^-298 or
              its rounding, still a multiple of 2^-1074: everything is scaled by 2^1074)
    hot(i)    cnt(i) >= 1, no bad centre in W(i) and E(i) >= lim(i) = fl64((T T) cnt(i)): ONE float64 multiply of the exact square
    dead(j)   hot(i) for some i in [j - h, j + h] inside [0, n)
An interleaved file (n, ch): channel c is the column x[:, c], its peak its own; channel -1 is joint -- a time is dead when every column's
dead holds, against ONE threshold from the peak over all elements.

The device adds the squares in float64 in an order of its own; its E lies within cnt 2^-52 E of the exact one and equals it when every
partial sum is representable.  undecided() lists the samples whose exact E is that close to lim WITHOUT being a float64: there the
order of the additions could decide.  Every case builder asserts that its case has none -- the cap is zero, not a tolerance.

Every function takes bug=<name>, one of MISTAKES, which seeds that mistake into the reference: tests/test_burst_ref.py shows that each
one changes the expected rows of at least one case, i.e. that the cases can tell."""
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

from tests import dead_ref as R
from tests import detect_ref as D

CHUNK, TILE = D.CHUNK, D.CARRY_TILE
SHIFT = 1074
f32, f64 = np.float32, np.float64
S24 = np.int32                                       # the dtype that stands for packed 24-bit values in [-2^23, 2^23 - 1]
LO24, HI24 = -(1 << 23), (1 << 23) - 1
MISTAKES = ("window_from_0", "cnt_full", "first_difference", "coefficient_1", "adjacent_channel", "greater", "no_dilation", "int16_wrap",
            "int32_squares", "bad_centre_only", "fp32_D")
FULL = {np.float32: 1.0, np.int16: 32768.0, S24: 8388608.0}
THR = {t: float(f32(1.15 * fs)) for t, fs in FULL.items()}     # the documented starting point: 1.15 of full scale
HALVES = (0, 1, 7, 8, 48, 511, 512, 1023, 1024)
SIZES = (1, 2, 3, 4, "2h+1", "2h+2", "2h+3", 2047, 2048, 2049, 2050, 4101, 6144)
DTYPES = (np.float32, np.int16, S24)


def sizes(h):
    return sorted({2 * h + int(n[2:]) if isinstance(n, str) else n for n in SIZES})


def sweep():
    """The thinned product of the size sweep: every n meets h in {0, 1, 1024}, every h meets n in {2049, 4101}, the 2 h + k sizes
    meet their own h."""
    out = []
    for h in HALVES:
        for n in sizes(h):
            if h in (0, 1, 1024) or n in (2049, 4101) or n in (2 * h + 1, 2 * h + 2, 2 * h + 3):
                out.append((n, h))
    for h in (0, 1, 1024):                                             # the 2 h' + k sizes of the other halves meet these three too
        for g in HALVES:
            for n in (2 * g + 1, 2 * g + 2, 2 * g + 3):
                if (n, h) not in out:
                    out.append((n, h))
    return out


# ------------------------------------------------------------------------------------------------------------ the definition
def _window_sum(values, a, b):
    """sum(values[a[i] .. b[i]]) per i (empty when b[i] < a[i]) by integer prefix sums: exact, and so is their difference."""
    cs = np.concatenate([np.zeros(1, dtype=values.dtype), np.cumsum(values)])
    return np.where(b >= a, cs[np.maximum(b, a - 1) + 1] - cs[a], cs[:1])


def _squares(ext, bug):
    """Per element k of ext (a channel with whatever a mistake lets it see around it): the exact square of d(k) as an integer -- in
    units of 1 for PCM, of 2^-1074 for fp32 --, bad(k), and for bug="bad_centre_only" whether an unjudged neighbour makes the square
    +inf or NaN.  Entries 0 and len - 1 have no d and read 0."""
    m = ext.size
    z = np.zeros(m, dtype=np.int64)
    if m < 3:
        return z, 1, z.astype(bool), z.astype(bool), z.astype(bool)
    if ext.dtype != np.float32:
        a, b, c = (ext[s:m - 2 + s].astype(np.int64) for s in (0, 1, 2))
        d = c - b if bug == "first_difference" else a - b + c if bug == "coefficient_1" else a - 2 * b + c
        if bug == "int16_wrap":
            d = d.astype(np.int16).astype(np.int64)
        if bug == "int32_squares":
            with np.errstate(over="ignore"):
                sq = (d.astype(np.int32) * d.astype(np.int32)).astype(np.int64)
        else:
            sq = d * d                                                 # below 2^34 (int16) / 2^50 (24-bit)
        sq = np.concatenate([z[:1], sq, z[:1]])
        return (sq if ext.dtype == np.int16 or m < 8192 else sq.astype(object)), 1, z.astype(bool), z.astype(bool), z.astype(bool)   # m 2^50 < 2^63
    fin = np.isfinite(ext)
    a, b, c = (ext[s:m - 2 + s] for s in (0, 1, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        if bug == "fp32_D":
            Dv = ((a + c).astype(f32) - (f32(2) * b).astype(f32)).astype(f32).astype(f64)
        elif bug == "first_difference":
            Dv = c.astype(f64) - b.astype(f64)
        elif bug == "coefficient_1":
            Dv = (a.astype(f64) + c.astype(f64)) - b.astype(f64)
        else:
            Dv = (a.astype(f64) + c.astype(f64)) - f64(2) * b.astype(f64)     # two roundings: 2 b is exact
        sqf = Dv * Dv                                                  # one rounding
    three = fin[:-2] & fin[1:-1] & fin[2:]
    bad = ~(fin[1:-1] if bug == "bad_centre_only" else three)
    nanv = ~bad & np.isnan(sqf)                                        # only under a seeded mistake: the reference's squares are finite
    infv = ~bad & np.isinf(sqf)
    ok = ~bad & np.isfinite(sqf)
    pad = lambda v, fill: np.concatenate([np.full(1, fill, v.dtype), v, np.full(1, fill, v.dtype)])
    small = np.where(ok, sqf, 0.0) * 2.0 ** 40                         # a power of two: exact
    if np.all(small == np.rint(small)) and small.sum() < 2.0 ** 62:    # the builders' grid: squares are multiples of 2^-40, int64 holds their sums
        return pad(small.astype(np.int64), 0), 1 << 40, pad(bad, False), pad(infv, False), pad(nanv, False)
    ints = np.array([int(Fraction(float(v)) * (1 << SHIFT)) if k else 0 for v, k in zip(sqf.tolist(), ok.tolist())], dtype=object)
    return pad(ints, 0), 1 << SHIFT, pad(bad, False), pad(infv, False), pad(nanv, False)


def hot_column(col, h, T, before=None, after=None, bug=None, report=None):
    """hot(i) for one channel.  before: what lies in memory in front of col, oldest first; the reference never looks at it,
    bug="window_from_0" gives sample 0 a second difference with it (0 when nothing is given) and starts the windows at 0."""
    col = np.asarray(col)
    n, h = col.size, int(h)
    from0 = bug == "window_from_0"
    pre = (np.asarray(before, col.dtype).reshape(-1)[-1:] if before is not None else np.zeros(1, col.dtype)) if from0 else col[:0]
    ext, off = np.concatenate([pre, col]), pre.size
    sq, unit, bad, infv, nanv = _squares(ext, bug)
    i = np.arange(n)
    lo = 0 if from0 else 1
    a, b = np.maximum(i - h, lo), np.minimum(i + h, n - 2)
    cnt = np.maximum(b - a + 1, 0) if bug != "cnt_full" else np.full(n, 2 * h + 1)
    have = b >= a
    T2 = f64(f32(T)) * f64(f32(T))                                     # 24 x 24 bits: exact
    with np.errstate(over="ignore"):
        lim = T2 * cnt.astype(f64)                                     # one rounding
    E = _window_sum(sq, a + off, b + off)
    if E.dtype == object:
        Ef = np.array([e / unit for e in E.tolist()], dtype=f64)       # int / int: the correctly rounded quotient
    else:
        Ef = E.astype(f64) / f64(unit)                                 # int64 -> float64 rounds correctly; unit is a power of two
    hot = Ef > lim                                                     # rounding is monotonic: Ef > lim => E > lim, Ef < lim => E < lim
    for k in np.flatnonzero(Ef == lim):
        exact = Fraction(float(lim[k])) * unit
        hot[k] = int(E[k]) > exact if bug == "greater" else int(E[k]) >= exact
    if report is not None and col.dtype != np.int16:                   # int16: E < 2^46, every partial sum is a float64
        near = np.flatnonzero((np.abs(Ef - lim) <= 4.0 * cnt * 2.0 ** -52 * Ef) & (Ef > 0))
        for k in near:
            e, l = Fraction(int(E[k]), unit), Fraction(float(lim[k]))
            if Fraction(float(Ef[k])) != e and abs(e - l) <= cnt[k] * Fraction(1, 1 << 52) * e:
                report.append(int(k))
    count = lambda v: _window_sum(v.astype(np.int64), a + off, b + off)
    hot = (hot | (count(infv) > 0)) & (count(nanv) == 0)               # only a seeded mistake sets either
    return hot & have & (count(bad) == 0)


def dilate(hot, h):
    """dead(j) = some hot(i) with |i - j| <= h, i inside the array."""
    n = hot.size
    j = np.arange(n)
    return _window_sum(hot.astype(np.int64), np.maximum(j - h, 0), np.minimum(j + h, n - 1)) > 0


def _dead_column(col, h, T, before=None, after=None, bug=None, report=None):
    hot = hot_column(col, h, T, before, after, bug, report)
    return hot if bug == "no_dilation" else dilate(hot, h)


def burst_mask(x, half, thr=0.0, rel=0.0, channel=None, before=None, after=None, bug=None, report=None):
    """dead(j) per sample time.  x (n,) with channel None, or (n, ch) with channel = a column or -1 (joint).  before / after: the sample
    times in memory in front of x and behind it ((k,) or (k, ch); read only by a seeded mistake)."""
    x = np.asarray(x)
    T = R.threshold_ref(x, thr, rel, channel)
    if x.ndim == 1:
        return _dead_column(x, half, T, before, after, bug, report)
    n, ch = x.shape
    cols = list(range(ch)) if channel < 0 else [channel]
    if bug == "adjacent_channel":                                      # the neighbours are the adjacent ELEMENTS of the file
        dead = _dead_column(x.reshape(-1), half, T).reshape(n, ch)
        return np.all(dead[:, cols], axis=1)
    pick = lambda rows, c: None if rows is None else np.asarray(rows).reshape(-1, ch)[:, c]
    return np.all(np.stack([_dead_column(x[:, c], half, T, pick(before, c), pick(after, c), bug, report) for c in cols], axis=1), axis=1)


def burst_runs_ref(x, half, thr=0.0, rel=0.0, min_len=1, channel=None, before=None, after=None, bug=None):
    return R.runs_of(burst_mask(x, half, thr, rel, channel, before, after, bug), min_len)


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    """One call of si_burst_runs and what surrounds its input in memory.  x (n,) or (n, ch); before / after: sample times planted in
    front of the base and behind the input, (k,) or (k, ch), oldest first (zeros and full-scale values: neither may be read)."""
    name: str
    x: np.ndarray
    half: int
    thr: float = 0.0
    rel: float = 0.0
    min_len: int = 1
    channel: Optional[int] = None
    before: Optional[np.ndarray] = None
    after: Optional[np.ndarray] = None

    def mask(self, bug=None, report=None):
        return burst_mask(self.x, self.half, self.thr, self.rel, self.channel, self.before, self.after, bug, report)

    def rows(self, bug=None):
        if bug is None:                                                # computed once: the reference is shared and left unchanged
            if not hasattr(self, "_rows"):
                self._rows = R.runs_of(self.mask(), self.min_len)
            return self._rows
        return R.runs_of(self.mask(bug), self.min_len)

    def threshold(self):
        return R.threshold_ref(self.x, self.thr, self.rel, self.channel)

    def undecided(self):
        report = []
        self.mask(report=report)
        return report

    def memory(self):
        """(flat elements: before | x | after, the element index x starts at)."""
        ch = 1 if self.x.ndim == 1 else self.x.shape[1]
        part = lambda r: np.zeros(0, self.x.dtype) if r is None else np.asarray(r, self.x.dtype).reshape(-1)
        pre = part(self.before)
        assert pre.size % ch == 0 and part(self.after).size % ch == 0
        return np.concatenate([pre, self.x.reshape(-1), part(self.after)]), pre.size


def decided(case):
    """The builders' gate: no sample of the case depends on the order of the additions."""
    und = case.undecided()
    assert und == [], (case.name, und[:8])
    return case


def _grid(dtype):
    """Integers times this are the dtype's values: fp32 cases live on a 2^-16 grid with |x| <= 1, so every D is a multiple of 2^-16 up
    to 4, every square one of 2^-32 up to 16, and any sum of up to 2049 of them is a float64."""
    return f32(2.0 ** -16) if dtype is np.float32 else 1


def _amp(dtype):
    return {np.float32: 1 << 16, np.int16: 32768, S24: 1 << 23}[dtype]


def clean(n, dtype, seed):
    """Speech's stand-in: a slow oscillation at 0.6 of full scale, period ~200 samples, whose second difference stays under 0.001 of
    full scale -- no window of it is hot at THR."""
    ph = np.random.default_rng(seed).uniform(0, 6.28)
    v = np.rint(0.6 * _amp(dtype) * np.sin(ph + np.arange(n) * (2 * np.pi / 197.3)))
    return (v.astype(f64).astype(f32) * _grid(dtype)).astype(f32) if dtype is np.float32 else v.astype(dtype)


def garbage(n, dtype, seed, alternate=False):
    """A corrupted block: uniformly random values over the whole range (RMS of d = sqrt(6) of the value RMS = sqrt(2) of full scale),
    or, alternate=True, +A, -A, +A ... at A = half of full scale: |d| = 4 A = 2 full scales at every centre inside it."""
    A = _amp(dtype)
    if alternate:
        v = np.where(np.arange(n) % 2 == 0, A // 2, -(A // 2))
    else:
        v = np.random.default_rng(seed).integers(-A, A, n)
    return (v.astype(f64).astype(f32) * _grid(dtype)).astype(f32) if dtype is np.float32 else v.astype(dtype)


def full_scale(k, dtype, ch=None):
    hi, lo = {np.float32: (1.0, -1.0), np.int16: (32767, -32768), S24: (HI24, LO24)}[dtype]
    v = np.full(k if ch is None else (k, ch), hi, dtype=dtype)
    v[1::2] = lo
    return v


def size_cases(n, h, dtype):
    """The layouts of the size sweep at n samples and half window h: garbage blocks (random and alternating) on, off and across every
    chunk seam, at sample 1 and ending at n - 2, at both file ends, one window long.  Full-scale alternation -- the loudest second
    difference there is -- is planted in front of the base and behind the input in the even layouts, zeros in the odd ones."""
    thr, L = THR[dtype], 2 * h + 1
    seams = [s for s in range(CHUNK, n + 1, CHUNK)]
    fit = lambda runs: [(max(a, 0), min(b, n)) for a, b in runs if min(b, n) > max(a, 0)]
    layouts = [("clean throughout", []), ("garbage throughout", [(0, n)]),
               ("from sample 1 and to sample n - 2", fit([(1, h + 6), (n - h - 5, n - 1)])),
               ("both file ends", fit([(0, h + 5), (n - h - 3, n)])),
               ("across the seams", fit([(s - h - 37, s + h + 41) for s in seams] + [(100, 100 + L + 3)])),
               ("ending on and starting on the seams", fit([(s - L - 9, s) for s in seams[0::2]] + [(s, s + L + 5) for s in seams[1::2]] + [(7, 7 + L)])),
               ("one window beside each seam", fit([(s - L, s) for s in seams] + [(s + 2 * L + 3, s + 3 * L + 2) for s in seams]
                                                    + [(3, 3 + L), (9 + 2 * L, 8 + 3 * L)]))]
    out = []
    for k, (name, runs) in enumerate(layouts):
        x = clean(n, dtype, 1000 * k + n + h)
        for r, (a, b) in enumerate(runs):
            x[a:b] = garbage(b - a, dtype, a + b, alternate=r % 2 == 1)
        pad = 2 * h + 8
        plant = np.zeros(pad, dtype) if k % 2 else full_scale(pad, dtype)
        out.append(decided(Case(f"{name}, n {n}, h {h}, {np.dtype(dtype).name}", x, h, thr, 0.0, 1 if k % 3 else max(1, h // 2), None, plant, plant)))
    return out


def value_cases(h, dtype):
    """The value edges at half window h (any h >= 0), each with what it must give asserted here."""
    n, L = 6 * (2 * h + 1) + 40, 2 * h + 1
    fp = dtype is np.float32
    g = _grid(dtype)
    E = []

    def add(name, x, want, thr, **kw):
        x = np.asarray(x).astype(dtype)
        pad = 2 * h + 4
        c = decided(Case(f"{name}, h {h}, {np.dtype(dtype).name}", x, h, thr, kw.pop("rel", 0.0), kw.pop("min_len", 1), None,
                         full_scale(pad, dtype), full_scale(pad, dtype)))
        got = c.rows().tolist()
        assert want is None or got == [list(w) for w in want], (c.name, got, want)
        E.append(c)
        return c

    alt = lambda a: np.where(np.arange(n) % 2 == 0, a, -a)            # |d| = 4 a at every centre
    whole = [(0, n)] if h else [(1, n - 2)]                           # every centre hot: without a dilation samples 0 and n - 1 stay out
    up = lambda t: float(np.nextafter(f32(t), f32(np.inf)))
    # E == lim exactly, at full and at truncated windows; one step over T finds nothing
    add("|d| = 12 everywhere at T = 12", alt(3) * g, whole, 12.0 * float(g))
    add("|d| = 12 everywhere one step over T = 12", alt(3) * g, [], up(12.0 * float(g)))
    hi, lo = {np.float32: (1.0, -1.0), np.int16: (32767, -32768), S24: (HI24, LO24)}[dtype]
    x = np.where(np.arange(n) % 2 == 0, hi, lo)
    big = float(f32(2 * (float(hi) - float(lo))))                     # the largest |d|: 131 070 for int16; fl32 of 2^25 - 2 for 24-bit is 2^25
    if dtype is S24:
        add("HI / LO alternation: |d| = 2^25 - 2 at T = 2^25 - 4", x, whole, 33554428.0)
        add("HI / LO alternation at T = 2^25", x, [], 33554432.0)
    else:
        add("full-scale alternation: the largest |d| at T = |d|", x, whole, big)
        add("full-scale alternation one step over", x, [], up(big))
    add("full-scale alternation, T from the peak with rel = 4", x, None, 0.0, rel=4.0)
    # the truncated count: garbage of |d| = 12 from sample 0 on for h + 1 samples; its first windows hold h .. centres, not 2 h + 1
    base = np.zeros(n)
    s = 2 * L + 5
    if h >= 1:
        x = base.copy(); x[:h + 2] = alt(3)[:h + 2]
        c = add("a block at the file's start: the truncated count", x * g, None, 8.0 * float(g))
        assert c.rows()[0].tolist()[0] == 0
        x = base.copy(); x[n - h - 2:] = alt(3)[:h + 2]
        c = add("a block at the file's end: the truncated count", x * g, None, 8.0 * float(g))
        assert sum(c.rows()[-1].tolist()) == n
    # a lone spike v at p: d = v, -2 v, v at p - 1, p, p + 1.  With 5 v^2 < T^2 (2 h + 1) <= 6 v^2 only the 2 h - 1 windows that hold all
    # three are hot, and the dead samples are [p + 1 - 2 h, p - 1 + 2 h]; at h = 0 and T = 1.5 v only centre p is
    v = 3000
    T = float(f32((1.5 if h == 0 else np.sqrt(5.5 / L)) * v * float(g)))
    x = base.copy(); x[s] = v
    add("a lone spike", x * g, [(s, 1)] if h == 0 else [(s + 1 - 2 * h, 4 * h - 1)], T)
    if h >= 1:                                                        # two of them: the last hot window of one and the first of the other
        for apart, want in ((2 * h, 1), (2 * h + 1, 1), (2 * h + 2, 2)):
            q = s + apart + 2 * h - 2                                  # (q + 1 - h) - (s - 1 + h) = apart
            x = base.copy(); x[s] = v; x[q] = -v
            c = add(f"two spikes, hot windows {apart - 2 * h} more than 2 h apart", x * g, None, T)
            assert len(c.rows()) == want, (c.name, c.rows().tolist())
    if fp:
        nan, inf = np.nan, np.inf
        z = base.copy(); z[s:s + L + 2] = alt(0.5)[:L + 2]            # centres s + 1 .. s + L have all three samples in the block
        thr = 2.0
        want = burst_runs_ref(z.astype(f32), h, thr).tolist()
        assert len(want) == 1
        for what, v in (("NaN", nan), ("+inf", inf), ("-inf", -inf)):
            for pos, where in ((s + L + 4, "two past the block"), (s + L + 2, "one past the block: a neighbour of the centre behind the windows"),
                               (s + L + 1, "at the block's last sample: the last centre's neighbour"), (s + L, "at the last centre"),
                               (s + 1 + h, "at the middle centre"), (s, "at the block's first sample"), (s - 2, "two in front of the block")):
                x = z.copy(); x[pos] = v
                add(f"{what} {where}", x, None, thr)
        x = z.copy(); x[0] = nan; x[n - 1] = inf
        add("NaN at sample 0 and inf at sample n - 1", x, want, thr)
        x = z.copy(); x[3] = nan; x[5] = inf; x[n - 9] = 3.0e38        # the peak skips NaN and inf; rel * peak stays finite
        c = add("T from the peak, 3e38", x, None, 0.0, rel=2.0 ** -127)
        assert c.threshold() == f32(3.0e38) * f32(2.0 ** -127)
        # D is formed in float64: 1 + 3 2^-24 is not an fp32
        x = base.copy(); x[s - 1] = 1.0; x[s] = 0.5; x[s + 1] = 3 * 2.0 ** -24
        add("a second difference of 3 2^-24 between 1, 0.5 and 3 2^-24", x, None, 3.5 * 2.0 ** -24)
    return E


def channel_cases(ch, dtype, h=7):
    """An (n, ch) file of two chunks and 77 times (six chunks for h > 8): a common block in all channels, one across the seam, channel c's own block where its
    neighbours c - 1 and c + 1 are clean, and a stretch where the CHANNELS alternate while each of them is constant (loud between adjacent
    elements, silent along a channel).  One case per channel and the joint one; then the peak."""
    n, thr, L = (2 if h <= 8 else 6) * CHUNK + 77, THR[dtype], 2 * h + 1
    own = lambda c: CHUNK + 4 * L + 4 * L * c
    assert own(ch - 1) + 2 * L < n - 6 * L
    cols = []
    for c in range(ch):
        x = clean(n, dtype, 50 * ch + c)
        for a, b in [(200, 200 + 6 * L), (CHUNK - 3 * L - c, CHUNK + 2 * L + c), (own(c), own(c) + 2 * L)]:
            x[a:b] = garbage(b - a, dtype, a, alternate=a == own(c))   # the seed is the position; the channel's own block alternates
        A = _amp(dtype) // 2
        x[n - 5 * L:n - L] = np.asarray((A if c % 2 == 0 else -A) * _grid(dtype)).astype(dtype)
        cols.append(x)
    x = R.interleave(cols)
    before, after = full_scale(2 * h + 3, dtype, ch), np.zeros((2 * h + 3, ch), dtype)
    out = []
    for c in list(range(ch)) + [-1]:
        case = decided(Case(f"{ch} channels, channel {c}, h {h}, {np.dtype(dtype).name}", x, h, thr, 0.0, 2, c, before, after))
        if c >= 0:
            assert np.array_equal(case.mask(), burst_mask(np.ascontiguousarray(x[:, c]), h, thr)), case.name
            assert any(a <= own(c) and a + l >= own(c) + 2 * L for a, l in case.rows().tolist()), case.name
        else:
            first = case.rows()[0].tolist()                            # the common block; every channel's own block is clean in the others
            assert first[0] <= 200 and sum(first) >= 200 + 6 * L and not any(case.mask()[own(k) + L] for k in range(ch)), case.rows().tolist()
        out.append(case)
    low = x.copy()
    low[:] = (low.astype(f64) / 4).astype(dtype) if dtype is not np.float32 else (low / f32(4))
    low[7, ch - 1] = f32(0.875) if dtype is np.float32 else dtype(int(0.875 * _amp(dtype)))
    for c in (0, ch - 1, -1):
        out.append(decided(Case(f"{ch} channels, peak of channel {c}, {np.dtype(dtype).name}", low, h, 0.0, 0.4, 1, c, full_scale(2 * h + 3, dtype, ch),
                                full_scale(2 * h + 3, dtype, ch))))
    assert out[-3].threshold() < out[-2].threshold() == out[-1].threshold()
    return out


def long_case(h=48):
    """An int16 file of 1026 chunks and 5 samples, 1027 workgroups: the carry scan and the peak's final reduce take two tiles.  A
    garbage block spans the tile seam with whole dead chunks on both sides of it; the peak lies in the last chunk."""
    seam = TILE * CHUNK
    n = seam + 2 * CHUNK + 5
    x = (clean(n, np.int16, 5) // 2).astype(np.int16)
    x[n - 3] = 32767
    x[5000:5400] = garbage(400, np.int16, 1)
    x[seam - CHUNK - 1000:seam + CHUNK + 200] = garbage(2 * CHUNK + 1200, np.int16, 2)
    c = decided(Case("1027 chunks", x, h, 0.0, 1.15, 64, None, full_scale(2 * h + 2, np.int16), full_scale(2 * h + 2, np.int16)))
    rows = c.rows().tolist()
    assert c.threshold() == f32(1.15) * f32(32767) and len(rows) == 2, rows
    assert rows[0][0] <= 5000 and sum(rows[0]) >= 5400 and rows[1][0] <= seam - CHUNK - 1000 and sum(rows[1]) >= seam + CHUNK + 200
    assert -(-n // CHUNK) == TILE + 3
    return c


BLOCKS = ((8000, 4410), (24000, 2205))


def seg22():
    import os
    x = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lj001_resample.npz"))["seg22"].copy()
    assert x.dtype == np.int16 and x.shape == (39690,) and np.abs(x.astype(np.int32)).max() == 20176
    return x


def seg22_scaled():
    """The fixture scaled so that its peak is 32 767."""
    return np.rint(seg22().astype(f64) * (32767.0 / 20176.0)).astype(np.int16)


def seg22_damaged():
    """The issue's measurement: seg22 with [8000, 12410) replaced by default_rng(0).integers(-32768, 32768, 4410) and [24000, 26205)
    byte-swapped."""
    x = seg22()
    x[8000:12410] = np.random.default_rng(0).integers(-32768, 32768, 4410).astype(np.int16)
    x[24000:26205] = x[24000:26205].byteswap()
    return x


def all_cpu_cases():
    """Every case a CPU test walks (the long one and the big sizes apart)."""
    out = []
    for dtype in DTYPES:
        for h in (0, 1, 7, 48):
            out += value_cases(h, dtype)
            for n in (3, 4, 2 * h + 3, 2049):
                out += size_cases(n, h, dtype)
        for ch in (2, 3):
            out += channel_cases(ch, dtype)
    return out
