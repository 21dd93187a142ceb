"""Dropouts by windowed RMS level: the exact reference of si_level_runs and the case builders of
tests/test_level_ref.py and tests/test_gpu_level.py.  A plain module, imported by name; importing it needs no GPU.

The contract, for one channel x[0 .. n) (fp32 or int16) and h = half:
    T         max(thr, fl32(rel * peak)): tests/dead_ref.py's threshold_ref (the peak over the finite samples; rel == 0: T = thr)
    sq(k)     x[k]^2, exact; bad(k): x[k] is NaN or +-inf
    W(i)      [max(0, i - h), min(n - 1, i + h)], cnt(i) = |W(i)|
    E(i)      the sum of sq over W(i) -- here EXACT: int64 for int16, Python integers scaled by 2^298 for fp32 (an fp32 is a multiple of
              2^-149, its square of 2^-298)
    low(i)    no bad sample in W(i) and E(i) <= lim(i) = fl64((T T) cnt(i)): ONE float64 multiply of the exact square
    dead(j)   low(i) for some i in [j - h, j + h] inside [0, n)
An interleaved file (n, ch): channel c is the column x[:, c], its peak its own; channel -1 is joint -- a time is dead when every column's
dead holds, each by its own windows, against ONE threshold from the peak over all elements.

The device adds the squares in float64 in an order of its own; its E lies within cnt 2^-52 E of the exact one and equals it when E is
representable.  undecided() lists the samples whose exact E is that close to lim WITHOUT being a float64: there the order of the
additions could decide.  Every case builder asserts that its case has none -- the cap is zero, not a tolerance.

Every function takes bug=<name>, one of MISTAKES, which seeds that mistake into the reference: tests/test_level_ref.py shows that each
one changes the expected rows of at least one case, i.e. that the cases can tell."""
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

from tests import dead_ref as R
from tests import detect_ref as D

CHUNK, TILE = D.CHUNK, D.CARRY_TILE
SCALE = 1 << 298
f32, f64 = np.float32, np.float64
MISTAKES = ("past_n", "before_0", "cnt_full", "no_dilation", "dilate_2h", "adjacent_channel", "nan_zero", "prefix_diff", "int32_squares")
THR = {np.float32: 2.0 ** -10, np.int16: 16.0}      # the thresholds the builders are written for
HALVES = (0, 1, 7, 8, 48, 511, 512, 1023, 1024)


def sizes(h):
    """The sample counts of the size sweep at half window h."""
    return sorted({n for n in (1, 2, 2 * h, 2 * h + 1, 2047, 2048, 2049, 4101, 6144) if n >= 1})


# ------------------------------------------------------------------------------------------------------------ the definition
def _window_sum(values, a, b):
    """sum(values[a[i] .. b[i]]) per i by integer prefix sums (int64 or Python integers: exact, and so is their difference)."""
    cs = np.concatenate([np.zeros(1, dtype=values.dtype), np.cumsum(values)])
    return cs[b + 1] - cs[a]


def low_column(col, h, T, before=None, after=None, bug=None, report=None):
    """low(i) for one channel.  before / after: what lies in memory in front of col and behind it, oldest first (any number of
    samples); the reference never looks at them, bug="before_0" / "past_n" lets the windows reach into them.
    report: a list that receives the undecided samples (see the module's text)."""
    col = np.asarray(col)
    n, h = col.size, int(h)
    pre = np.asarray(before, col.dtype).reshape(-1) if (bug == "before_0" and before is not None) else col[:0]
    post = np.asarray(after, col.dtype).reshape(-1) if (bug == "past_n" and after is not None) else col[:0]
    ext, off = np.concatenate([pre, col, post]), pre.size
    i = np.arange(n)
    a, b = np.maximum(i - h, -pre.size) + off, np.minimum(i + h, n - 1 + post.size) + off       # the window, in ext
    cnt = (np.minimum(i + h, n - 1) - np.maximum(i - h, 0) + 1) if bug != "cnt_full" else np.full(n, 2 * h + 1)
    T2 = f64(f32(T)) * f64(f32(T))                                     # 24 x 24 bits: exact
    lim = T2 * cnt.astype(f64)                                         # one rounding
    if col.dtype == np.int16:
        if bug == "int32_squares":
            with np.errstate(over="ignore"):
                sq = ext.astype(np.int32) * ext.astype(np.int32)
                cs = np.concatenate([np.zeros(1, np.int32), np.cumsum(sq, dtype=np.int32)])
                E = (cs[b + 1] - cs[a]).astype(np.int64)              # a 32-bit accumulator wraps
        else:
            E = _window_sum(ext.astype(np.int64) ** 2, a, b)          # < 2^42: a float64 holds it
        return E.astype(f64) <= lim
    ext = ext.astype(f32)
    bad = ~np.isfinite(ext)
    if bug == "prefix_diff":                                           # float64 running sums, one subtracted from the other
        with np.errstate(invalid="ignore", over="ignore"):
            cs = np.concatenate([np.zeros(1), np.cumsum(ext.astype(f64) ** 2)])
            return cs[b + 1] - cs[a] <= lim                           # a NaN poisons everything behind it
    ints = np.array([0 if bd else int(float(v) * 2.0 ** 149) for v, bd in zip(ext.tolist(), bad.tolist())], dtype=object)
    E = _window_sum(ints * ints, a, b)                                 # Python integers: x^2 2^298, exact
    Ef = np.array([e / SCALE for e in E.tolist()], dtype=f64)          # int / int: the correctly rounded quotient
    low = Ef < lim                                                     # rounding is monotonic: Ef < lim => E < lim, Ef > lim => E > lim
    for k in np.flatnonzero(Ef == lim):
        low[k] = E[k] <= Fraction(float(lim[k])) * SCALE
    if report is not None:
        near = np.flatnonzero((np.abs(Ef - lim) <= 4.0 * cnt * 2.0 ** -52 * Ef) & (Ef > 0))
        for k in near:
            e, l = Fraction(int(E[k]), SCALE), Fraction(float(lim[k]))
            if Fraction(float(Ef[k])) != e and abs(e - l) <= cnt[k] * Fraction(1, 1 << 52) * e:
                report.append(int(k))
    if bug != "nan_zero":
        low &= _window_sum(bad.astype(np.int64), a, b) == 0
    return low


def dilate(low, h):
    """dead(j) = some low(i) with |i - j| <= h, i inside the array."""
    n = low.size
    j = np.arange(n)
    return _window_sum(low.astype(np.int64), np.maximum(j - h, 0), np.minimum(j + h, n - 1)) > 0


def _dead_column(col, h, T, before=None, after=None, bug=None, report=None):
    low = low_column(col, h, T, before, after, bug, report)
    return low if bug == "no_dilation" else dilate(low, 2 * h if bug == "dilate_2h" else h)


def level_mask(x, half, thr=0.0, rel=0.0, channel=None, before=None, after=None, bug=None, report=None):
    """dead(j) per sample time.  x (n,) with channel None, or (n, ch) with channel = a column or -1 (joint).  before / after: the sample
    times in memory in front of x and behind it ((k,) or (k, ch); read only by a seeded mistake)."""
    x = np.asarray(x)
    T = R.threshold_ref(x, thr, rel, channel)
    if x.ndim == 1:
        return _dead_column(x, half, T, before, after, bug, report)
    n, ch = x.shape
    cols = list(range(ch)) if channel < 0 else [channel]
    if bug == "adjacent_channel":                                      # the window runs over the adjacent ELEMENTS of the file
        dead = _dead_column(x.reshape(-1), half, T).reshape(n, ch)
        return np.all(dead[:, cols], axis=1)
    pick = lambda rows, c: None if rows is None else np.asarray(rows).reshape(-1, ch)[:, c]
    return np.all(np.stack([_dead_column(x[:, c], half, T, pick(before, c), pick(after, c), bug, report) for c in cols], axis=1), axis=1)


def level_runs_ref(x, half, thr=0.0, rel=0.0, min_len=1, channel=None, before=None, after=None, bug=None):
    return R.runs_of(level_mask(x, half, thr, rel, channel, before, after, bug), min_len)


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    """One call of si_level_runs and what surrounds its input in memory.  x (n,) or (n, ch); before / after: sample times planted in
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
        return level_mask(self.x, self.half, self.thr, self.rel, self.channel, self.before, self.after, bug, report)

    def rows(self, bug=None):
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


def loud(n, dtype, seed):
    """Samples no window of which is low at THR: fp32 multiples of 2^-20 with 0.25 <= |x| < 1 (any sum of up to 2049 squares is a
    float64: the grid is 2^-40 and the sum stays below 2^12), int16 magnitudes of 8000 .. 32767."""
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1, 1], n)
    if dtype is np.float32:
        return (rng.integers(1 << 18, 1 << 20, n) * sign).astype(f64).astype(f32) * f32(2.0 ** -20)
    return (rng.integers(8000, 32768, n) * sign).astype(np.int16)


def floor_noise(n, dtype, seed):
    """A noise floor under THR: fp32 multiples of 2^-20 with |x| <= 2^-11, int16 rint(N(0, 4)) clipped to +-10; a few samples reach
    above THR itself, which no sample-wise detector survives."""
    rng = np.random.default_rng(seed)
    if dtype is np.float32:
        return rng.integers(-512, 513, n).astype(f64).astype(f32) * f32(2.0 ** -20)
    return np.clip(np.rint(rng.normal(0, 4, n)), -10, 10).astype(np.int16)


def full_scale(k, dtype, ch=None):
    v = np.full(k if ch is None else (k, ch), 32767 if dtype is np.int16 else 1.0, dtype=dtype)
    v[1::2] = -32768 if dtype is np.int16 else -1.0
    return v


def size_cases(n, h, dtype):
    """The layouts of the size sweep at n samples and half window h: dropouts (exact zeros and noise floors) on, off and across every
    chunk seam, at both file ends where the windows are truncated, 2 h + 1 long (one low window) and one sample shorter (none).
    Full-scale samples are planted in front of the base and behind the input in the even layouts, zeros in the odd ones."""
    thr, L = THR[dtype], 2 * h + 1
    seams = [s for s in range(CHUNK, n + 1, CHUNK)]
    fit = lambda runs: [(max(a, 0), min(b, n)) for a, b in runs if min(b, n) > max(a, 0)]
    layouts = [("loud throughout", []), ("a dropout throughout", [(0, n)]),
               ("both file ends", fit([(0, h + 5), (n - h - 3, n)])),
               ("both file ends, one sample short of a truncated window", fit([(1, h + 1), (n - h - 1, n - 1)])),
               ("across the seams", fit([(s - h - 37, s + h + 41) for s in seams] + [(100, 100 + L + 3)])),
               ("ending on and starting on the seams", fit([(s - L - 9, s) for s in seams[0::2]] + [(s, s + L + 5) for s in seams[1::2]] + [(7, 7 + L)])),
               ("exactly one low window beside each seam, and one short of it", fit([(s - L, s) for s in seams] + [(s + 2 * L + 3, s + 3 * L + 2) for s in seams]
                                                                                      + [(3, 3 + L), (9 + 2 * L, 8 + 3 * L)]))]
    out = []
    for k, (name, runs) in enumerate(layouts):
        x = loud(n, dtype, 1000 * k + n + h)
        for r, (a, b) in enumerate(runs):
            x[a:b] = 0 if r % 2 == 0 else floor_noise(b - a, dtype, a + b)
        pad = 2 * h + 8
        plant = np.zeros(pad, dtype) if k % 2 else full_scale(pad, dtype)
        out.append(decided(Case(f"{name}, n {n}, h {h}", x, h, thr, 0.0, 1 if k % 3 else max(1, h), None, plant, plant)))
    return out


def value_cases(h, dtype):
    """The value edges at half window h (any h >= 0), each with what it must give asserted here."""
    n, L = 6 * (2 * h + 1) + 40, 2 * h + 1
    int16 = dtype is np.int16
    E = []

    def add(name, x, want, thr, **kw):
        x = np.asarray(x, dtype=dtype)
        pad = 2 * h + 4
        c = decided(Case(f"{name}, h {h}", x, h, thr, kw.pop("rel", 0.0), kw.pop("min_len", 1), None, full_scale(pad, dtype), full_scale(pad, dtype)))
        got = c.rows().tolist()
        assert want is None or got == [list(w) for w in want], (c.name, got, want)
        E.append(c)
        return c

    # E == lim exactly, at full and at truncated windows; one step under finds nothing
    add("all samples 3 at T = 3", np.full(n, 3), [(0, n)], 3.0)
    add("all samples 3 one step under T = 3", np.full(n, 3), [], float(np.nextafter(f32(3), f32(0))))
    add("all samples -3 at T = 3", np.full(n, -3), [(0, n)], 3.0)
    if int16:
        add("all samples -32768 at T = 32768", np.full(n, -32768), [(0, n)], 32768.0)
        add("all samples -32768 at T = 32767", np.full(n, -32768), [], 32767.0)
    if h >= 4:                                                        # 16 cnt <= 9 (2 h + 1) only for the untruncated count
        add("all samples 4 at T = 3: the truncated count", np.full(n, 4), [], 3.0)
    big = 30000 if int16 else 3.0e38
    base = np.zeros(n)
    s = 2 * L + 5
    x = base.copy(); x[s - 1] = big; x[s + L:] = 20000 if int16 else 1.0       # one huge sample at p, zeros behind it, loud again: the run starts at p + 1
    add("a huge sample followed by zeros", x, [(0, s - 1), (s, L)], THR[dtype])
    x = base.copy(); x[s] = big                                       # a lone spike blocks 2 h + 1 centres: one sample is not dead
    add("a lone spike: low windows 2 h + 1 apart", x, [(0, s), (s + 1, n - s - 1)], 1.0)
    if h >= 1:
        a = int(np.sqrt(9 * L))                                       # a^2 <= 9 (2 h + 1) < 2 a^2: only the 2 h windows over BOTH are not low
        assert a * a <= 9 * L < 2 * a * a
        x = base.copy(); x[s] = x[s + 1] = a
        add("a pair: low windows 2 h apart merge", x, [(0, n)], 3.0)
    if not int16:
        nan, inf = np.nan, np.inf
        lo = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)               # loud, a zero run of exactly one window at [s, s + 2 h]
        z = lo.copy(); z[s:s + L] = 0
        add("one window of zeros", z, [(s, L)], 2.0 ** -10)
        for what, v in (("NaN", nan), ("+inf", inf), ("-inf", -inf)):
            x = z.copy(); x[s + L] = v
            add(f"{what} one past the window", x, [(s, L)], 2.0 ** -10)
            x = z.copy(); x[s - 1] = v
            add(f"{what} one in front of the window", x, [(s, L)], 2.0 ** -10)
            x = z.copy(); x[s + L - 1] = v
            add(f"{what} at the window's last sample", x, [], 2.0 ** -10)
            x = z.copy(); x[s] = v
            add(f"{what} at the window's first sample", x, [], 2.0 ** -10)
            x = z.copy(); x[s + h] = v
            add(f"{what} at the window's centre", x, [], 2.0 ** -10)
            x = base.copy(); x[s] = v                                 # in a long dropout: as the lone spike
            add(f"{what} inside a long dropout", x, [(0, s), (s + 1, n - s - 1)], 2.0 ** -10)
        x = base.copy(); x[0] = nan; x[n - 1] = inf
        add("NaN at sample 0 and inf at sample n - 1", x, [(1, n - 2)], 0.5)
        x = z.copy(); x[s + L] = 3.0e38; x[s - 1] = -3.0e38           # the peak skips NaN and inf, rel * peak stays finite
        x[3] = nan; x[5] = inf
        c = add("T from the peak, 3e38", x, None, 0.0, rel=2.0 ** -100)     # T = 2.4e8: the +-1 samples are low, the 3e38 ones, NaN and inf are not
        assert c.threshold() == f32(3.0e38) * f32(2.0 ** -100) and len(c.rows()) >= 2
    return E


def half0_cases(dtype):
    """half = 0 is the sample-wise detector: low(i) <=> |x[i]| <= T, squares on both sides.  -> cases whose rows are dead_ref's QUIET rows."""
    out = []
    for n in (1, 9, 2049, 4101):
        for name, q, min_len in D.seam_cases(n)[::3]:
            x = D.materialize(q, dtype, n)
            for rel in (0.0, 2.0 ** -9):
                c = decided(Case(f"half 0: {name}, n {n}, rel {rel}", x, 0, D.THR[dtype], rel, min_len))
                assert np.array_equal(c.rows(), R.dead_runs_ref(x, R.QUIET, D.THR[dtype], rel, 0.0, min_len)), c.name
                out.append(c)
    return out


def channel_cases(ch, dtype, h=7):
    """An (n, ch) file, n = two chunks and 77 times (six chunks for h > 8): every channel its own dropouts (a common one in all), channel c's dropout where
    its neighbours c - 1 and c + 1 are loud and the same noise floor planted in adjacent channels.  One case per channel, and the joint
    one; then the peak: one column's is its own, the joint one is the file's."""
    n, thr, L = (2 if h <= 8 else 6) * CHUNK + 77, THR[dtype], 2 * h + 1
    own = lambda c: CHUNK + 4 * L + 4 * L * c
    assert own(ch - 1) + 2 * L < n - h - 2 - ch
    cols = []
    for c in range(ch):
        x = loud(n, dtype, 50 * ch + c)
        for a, b in [(200, 200 + 6 * L), (CHUNK - 3 * L - c, CHUNK + 2 * L + c), (own(c), own(c) + 2 * L), (n - h - 2 - c, n)]:
            x[a:b] = floor_noise(b - a, dtype, a)                      # the seed is the position: adjacent channels hold equal values
        cols.append(x)
    x = R.interleave(cols)
    before, after = full_scale(2 * h + 3, dtype, ch), np.zeros((2 * h + 3, ch), dtype)
    out = []
    for c in list(range(ch)) + [-1]:
        case = decided(Case(f"{ch} channels, channel {c}, h {h}", x, h, thr, 0.0, 2, c, before, after))
        if c >= 0:
            assert np.array_equal(case.mask(), level_mask(np.ascontiguousarray(x[:, c]), h, thr)), case.name
            assert [own(c), 2 * L] in case.rows().tolist(), case.name
        else:
            assert case.rows().tolist() == [[200, 6 * L], [CHUNK - 3 * L, 5 * L], [n - h - 2, h + 2]], case.rows().tolist()
        out.append(case)
    quiet = x.copy()
    quiet[np.abs(quiet.astype(f64)) > (0.5 if dtype is np.float32 else 16000)] = 0
    quiet[7, ch - 1] = f32(0.875) if dtype is np.float32 else np.int16(28000)
    for c in (0, ch - 1, -1):
        out.append(decided(Case(f"{ch} channels, peak of channel {c}", quiet, h, 0.0, 2.0 ** -9, 1, c, full_scale(2 * h + 3, dtype, ch), full_scale(2 * h + 3, dtype, ch))))
    assert out[-3].threshold() < out[-2].threshold() == out[-1].threshold()
    return out


def long_case(h=48):
    """An int16 file of 1026 chunks and 5 samples, 1027 workgroups: the carry scan and the peak's final reduce take two tiles.  A
    noise-floor dropout spans the tile seam with whole dead chunks on both sides of it; the peak lies in the last chunk."""
    seam = TILE * CHUNK
    n = seam + 2 * CHUNK + 5
    x = loud(n, np.int16, 5) // 2
    x[n - 3] = 32767
    x[5000:5400] = floor_noise(400, np.int16, 1)
    x[seam - CHUNK - 1000:seam + CHUNK + 200] = floor_noise(2 * CHUNK + 1200, np.int16, 2)
    c = decided(Case("1027 chunks", x, h, 0.0, 2.0 ** -11, 64, None, full_scale(2 * h + 2, np.int16), full_scale(2 * h + 2, np.int16)))
    assert c.threshold() == f32(32767 * 2.0 ** -11) and c.rows().tolist() == [[5000, 400], [seam - CHUNK - 1000, 2 * CHUNK + 1200]]
    assert -(-n // CHUNK) == TILE + 3
    return c


def seg22_damaged():
    """The issue's measurement: tests/golden/lj001_resample.npz: seg22 (39 690 int16 samples, peak 20 176) with two 200 ms stretches,
    [8000, 12410) and [24000, 28410), replaced by rint(N(0, 12)) from default_rng(7)."""
    import os
    x = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lj001_resample.npz"))["seg22"].copy()
    assert x.dtype == np.int16 and x.shape == (39690,) and np.abs(x.astype(np.int32)).max() == 20176
    rng = np.random.default_rng(7)
    for a in (8000, 24000):
        x[a:a + 4410] = np.rint(rng.normal(0, 12, 4410))
    return x


def all_cpu_cases():
    """Every case a CPU test walks (the long one and the big sizes apart)."""
    out = []
    for dtype in (np.float32, np.int16):
        for h in (0, 1, 7, 48):
            out += value_cases(h, dtype)
            for n in (1, 2, 2 * h + 1, 2049):
                out += size_cases(n, h, dtype)
        out += half0_cases(dtype)
        for ch in (2, 3):
            out += channel_cases(ch, dtype)
    return out
