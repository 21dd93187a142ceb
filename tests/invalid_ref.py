"""NaN, inf and out-of-range samples: the exact reference of si_invalid_runs and of the three _valid feeds, and the case
builders of tests/test_invalid_ref.py, tests/test_gpu_invalid.py and tests/test_gpu_invalid_feed.py.  A plain module, imported by
name; importing it needs no GPU.  numpy, exact: there is no tolerance anywhere.

The contract, for a ceiling c > 0 (+inf allowed).  x is fp32, int16, or int32 holding 24-bit values (the device gets them packed):
    invalid(v, c)   fp32: not (|v| <= min(c, FLT_MAX)) -- NaN of any payload and sign, +-inf, |v| > c; -0.0 and subnormals are valid.
                    PCM:  not (fl32(|v|) <= c), the magnitude in a wider integer (|-32768| = 32768, |-2^23| = 2^23, both exact in fp32);
                    c counts the file's own steps
    dead(i)         invalid(x[i], c) for 0 <= i < n: what lies in front of the base or at / past n is never judged
    runs            every maximal run of dead samples of at least min_len samples, (start, len) rows sorted by start
    clean(x, c)     where(invalid, +0.0, x): what the feeds stage
An interleaved file (n, ch): channel c is the column x[:, c]; channel -1 is joint -- a time is dead when EVERY column's element is.

Every function takes bug=<name>, one of MISTAKES, which seeds that mistake: tests/test_invalid_ref.py shows that each one changes the
rows of some case or some cleaned sample, i.e. that the cases can tell."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from tests import dead_ref as R
from tests import detect_ref as D

CHUNK, TILE = D.CHUNK, D.CARRY_TILE
f32 = np.float32
S24 = np.int32                                       # the dtype that stands for packed 24-bit values in [-2^23, 2^23 - 1]
LO24, HI24 = -(1 << 23), (1 << 23) - 1
FLT_MAX = float(np.finfo(f32).max)
INF = float("inf")
DTYPES = (np.float32, np.int16, S24)
FULL = {np.float32: 1.0, np.int16: 32768.0, S24: 8388608.0}
MISTAKES = ("inf_valid", "nan_valid", "greater_equal", "pcm_own_width", "pcm_full_scale", "adjacent_channel", "sample_at_n", "minus_zero")
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)      # quiet and signalling NaNs of both signs, as in tests/io_ref.py
SIZES = (1, 2, 7, 8, 9, 2047, 2048, 2049, 4101)


def bits(words):
    """fp32 values from their bit patterns: payloads survive (np.float32(np.nan) would give one NaN only)."""
    return np.asarray(words, dtype=np.uint32).view(f32)


# ------------------------------------------------------------------------------------------------------------ the definition
def invalid_mask(v, c, bug=None, dtype=None):
    """invalid(v, c) element by element.  v: fp32, int16 or S24 values (dtype says which when v is given as S24 = int32)."""
    v = np.asarray(v)
    dtype = v.dtype.type if dtype is None else dtype
    c = f32(c)
    assert c > 0, c
    if dtype is np.float32:
        a = np.abs(v.astype(f32))
        lim = c if bug == "inf_valid" else min(c, f32(FLT_MAX))         # inf_valid: |inf| <= inf counts as valid
        with np.errstate(invalid="ignore"):
            if bug == "nan_valid":
                return a > lim                                          # v > c for !(v <= c): NaN compares false
            if bug == "greater_equal":
                return ~(a < lim)
            return ~(a <= lim)
    if bug == "pcm_own_width":                                          # the magnitude in the sample's own width: -32768 / -2^23 wrap to themselves
        if dtype is np.int16:
            a = np.abs(v.astype(np.int16)).astype(np.int64)             # numpy wraps: |-32768| = -32768
        else:
            w = v.astype(np.int64)
            a = np.where(w == LO24, LO24, np.abs(w))
    else:
        a = np.abs(v.astype(np.int64))
    if bug == "pcm_full_scale":                                         # the ceiling of a PCM file read in full-scale units
        c = f32(c * f32(FULL[dtype]))
    af = a.astype(f32)                                                  # exact: below 2^24, or exactly 2^15 / 2^23
    if bug == "greater_equal":
        return ~(af < c)
    if bug == "nan_valid":
        return af > c
    return ~(af <= c)


def dead_mask(x, c, channel=None, after=None, bug=None):
    """dead(i) per sample time.  x (n,) with channel None, or (n, ch) with channel = a column or -1 (joint).  after: the sample times in
    memory behind x ((k,) or (k, ch)), read only by the seeded mistake "sample_at_n", which judges the one at n as well (and, finding it
    dead, lets the last run reach it: the mask comes back one longer than n only there)."""
    x = np.asarray(x)
    dtype = x.dtype.type
    if x.ndim == 1:
        m = invalid_mask(x, c, bug, dtype)
        if bug == "sample_at_n" and after is not None and np.asarray(after).size:
            m = np.concatenate([m, invalid_mask(np.asarray(after, x.dtype).reshape(-1)[:1], c, None, dtype)])
        return m
    n, ch = x.shape
    cols = list(range(ch)) if channel < 0 else [channel]
    if bug == "adjacent_channel":                                      # element i ch + c + 1 judged in place of i ch + c
        flat = np.concatenate([x.reshape(-1)[1:], x.reshape(-1)[:1]]).reshape(n, ch)
        m = invalid_mask(flat, c, None, dtype)
    else:
        m = invalid_mask(x, c, bug, dtype)
    m = np.all(m[:, cols], axis=1)
    if bug == "sample_at_n" and after is not None and np.asarray(after).size:
        nxt = invalid_mask(np.asarray(after, x.dtype).reshape(-1, ch)[:1], c, None, dtype)
        m = np.concatenate([m, np.all(nxt[:, cols], axis=1)])
    return m


def invalid_runs_ref(x, c=INF, min_len=1, channel=None, after=None, bug=None):
    return R.runs_of(dead_mask(x, c, channel, after, bug), min_len)


def clean(x, c=INF, bug=None):
    """where(invalid, +0.0, x): fp32 keeps every other sample's bits; PCM gives the integers with 0 at the invalid ones."""
    x = np.asarray(x)
    m = invalid_mask(x, c, None if bug == "minus_zero" else bug)
    if x.dtype == np.float32:
        out = x.copy()
        out[m] = f32(-0.0) if bug == "minus_zero" else f32(0.0)
        return out
    out = x.copy()
    out[m] = 0
    return out


# ------------------------------------------------------------------------------------------------------------ the hand-checked table
def value_table():
    """(name, dtype, value(s), ceiling, invalid?) rows, each checked by hand."""
    nf = lambda v, up: float(np.nextafter(f32(v), f32(np.inf if up else -np.inf)))
    sub = float(bits([0x00000001])[0])                                  # the smallest subnormal
    T = []
    for w in NAN_BITS:
        for c in (INF, 1.0, FLT_MAX):
            T.append((f"NaN {w:#010x} at c = {c}", np.float32, bits([w]), c, True))
    for c in (INF, 1.0, FLT_MAX):
        T.append((f"+inf at c = {c}", np.float32, f32([np.inf]), c, True))
        T.append((f"-inf at c = {c}", np.float32, f32([-np.inf]), c, True))
    T += [("+FLT_MAX at c = inf", np.float32, f32([FLT_MAX]), INF, False), ("-FLT_MAX at c = inf", np.float32, f32([-FLT_MAX]), INF, False),
          ("+FLT_MAX at c = FLT_MAX", np.float32, f32([FLT_MAX]), FLT_MAX, False), ("-FLT_MAX at c = FLT_MAX", np.float32, f32([-FLT_MAX]), FLT_MAX, False),
          ("FLT_MAX at c = 1", np.float32, f32([FLT_MAX]), 1.0, True), ("3e38 at c = inf", np.float32, f32([3e38]), INF, False),
          ("3e38 at c = 1e20", np.float32, f32([3e38]), 1e20, True), ("1e20 at c = 1", np.float32, f32([1e20]), 1.0, True),
          ("|v| == c = 1", np.float32, f32([1.0]), 1.0, False), ("-|v| == c = 1", np.float32, f32([-1.0]), 1.0, False),
          ("one step over c = 1", np.float32, f32([nf(1.0, True)]), 1.0, True), ("minus one step over c = 1", np.float32, f32([-nf(1.0, True)]), 1.0, True),
          ("one step under c = 1", np.float32, f32([nf(1.0, False)]), 1.0, False),
          ("|v| == c = 0.75", np.float32, f32([0.75]), 0.75, False), ("one step over c = 0.75", np.float32, f32([nf(0.75, True)]), 0.75, True),
          ("one step under c = 0.75", np.float32, f32([-nf(0.75, False)]), 0.75, False),
          ("-0.0 at c = inf", np.float32, f32([-0.0]), INF, False), ("-0.0 at the smallest ceiling", np.float32, f32([-0.0]), sub, False),
          ("a subnormal at c = inf", np.float32, f32([sub]), INF, False), ("a subnormal at c = 1", np.float32, f32([-sub]), 1.0, False),
          ("0 at c = 1", np.float32, f32([0.0]), 1.0, False)]
    T += [("int16 -32768 at c = 32767", np.int16, np.int16([-32768]), 32767.0, True), ("int16 -32768 at c = 32768", np.int16, np.int16([-32768]), 32768.0, False),
          ("int16 32767 at c = 32767", np.int16, np.int16([32767]), 32767.0, False), ("int16 32767 at c = 32766", np.int16, np.int16([32767]), 32766.0, True),
          ("int16 -32767 at c = 32766", np.int16, np.int16([-32767]), 32766.0, True), ("int16 32766 at c = 32766", np.int16, np.int16([-32766]), 32766.0, False),
          ("int16 -32768 at c = inf", np.int16, np.int16([-32768]), INF, False), ("int16 0 at c = 0.5", np.int16, np.int16([0]), 0.5, False),
          ("int16 1 at c = 0.5", np.int16, np.int16([1]), 0.5, True), ("int16 1 at c = 1 (full scale is no PCM ceiling)", np.int16, np.int16([-1]), 1.0, False),
          ("int16 2 at c = 1", np.int16, np.int16([2]), 1.0, True)]
    T += [("s24 -2^23 at c = 2^23 - 1", S24, S24([LO24]), float(HI24), True), ("s24 -2^23 at c = 2^23", S24, S24([LO24]), 8388608.0, False),
          ("s24 2^23 - 1 at c = 2^23 - 1", S24, S24([HI24]), float(HI24), False), ("s24 2^23 - 1 at c = 2^23 - 2", S24, S24([HI24]), float(HI24 - 1), True),
          ("s24 2^23 - 2 at c = 2^23 - 2", S24, S24([-(HI24 - 1)]), float(HI24 - 1), False), ("s24 -2^23 at c = inf", S24, S24([LO24]), INF, False),
          ("s24 2 at c = 1", S24, S24([2]), 1.0, True), ("s24 1 at c = 1", S24, S24([1]), 1.0, False)]
    return T


def table_values(dtype):
    """Every value of the table's rows of `dtype`, whatever ceiling its row has, as one array (fp32: bit patterns kept)."""
    vals = np.concatenate([np.asarray(v).reshape(-1) for _, d, v, _, _ in value_table() if d is dtype])
    return vals.astype(dtype) if dtype is not np.float32 else vals.view(np.uint32).view(f32)


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    """One call of si_invalid_runs and what surrounds its input in memory.  x (n,) or (n, ch); before / after: sample times planted in
    front of the base and behind the input, (k,) or (k, ch): NaN or full scale, never read."""
    name: str
    x: np.ndarray
    ceiling: float = INF
    min_len: int = 1
    channel: Optional[int] = None
    before: Optional[np.ndarray] = None
    after: Optional[np.ndarray] = None

    def mask(self, bug=None):
        return dead_mask(self.x, self.ceiling, self.channel, self.after, bug)

    def rows(self, bug=None):
        if bug is None:                                                # computed once: the reference is shared and left unchanged
            if not hasattr(self, "_rows"):
                self._rows = R.runs_of(self.mask(), self.min_len)
            return self._rows
        return R.runs_of(self.mask(bug), self.min_len)

    def memory(self):
        """(flat elements: before | x | after, the element index x starts at)."""
        ch = 1 if self.x.ndim == 1 else self.x.shape[1]
        part = lambda r: np.zeros(0, self.x.dtype) if r is None else np.asarray(r, self.x.dtype).reshape(-1)
        pre = part(self.before)
        assert pre.size % ch == 0 and part(self.after).size % ch == 0
        return np.concatenate([pre, self.x.reshape(-1), part(self.after)]), pre.size


def finite_ceiling(dtype):
    """The finite ceilings the builders plant against: 1.0 (full scale) for fp32, 32766 / 2^23 - 2 for PCM (clipped samples)."""
    return {np.float32: 1.0, np.int16: 32766.0, S24: float(HI24 - 1)}[dtype]


def speech(n, dtype, seed, ch=None):
    """Valid samples under every ceiling the builders use: uniform in (-0.5, 0.5) of full scale, never 0 x sign trouble."""
    rng = np.random.default_rng(seed)
    shape = (n,) if ch is None else (n, ch)
    if dtype is np.float32:
        return (rng.integers(-(1 << 15), 1 << 15, shape).astype(np.float64) * 2.0 ** -16).astype(f32)
    return rng.integers(-int(FULL[dtype]) // 2, int(FULL[dtype]) // 2, shape).astype(dtype)


def bad_values(dtype, c):
    """The values a builder plants as invalid at ceiling c, cycled through: for fp32 the four NaNs, +-inf (and 3e38, 1e20 and one step
    over c under a finite c); for PCM the full-scale values above a finite c.  Each is asserted invalid here."""
    if dtype is np.float32:
        v = np.concatenate([bits(NAN_BITS), f32([np.inf, -np.inf])])
        if c < FLT_MAX:
            v = np.concatenate([v, f32([3e38, -1e20, float(np.nextafter(f32(c), f32(np.inf)))])])
    else:
        hi, lo = (32767, -32768) if dtype is np.int16 else (HI24, LO24)
        v = np.asarray([hi, lo, -hi], dtype=dtype)
    assert np.all(invalid_mask(v, c, None, dtype)), (dtype, c)
    return v


def trap(k, dtype, ch=None):
    """What is planted outside the input: NaN for fp32, full scale for PCM -- invalid under every finite ceiling (NaN under all)."""
    shape = (k,) if ch is None else (k, ch)
    if dtype is np.float32:
        return np.full(shape, 0xFFC00000, np.uint32).view(f32)
    return np.full(shape, -32768 if dtype is np.int16 else LO24, dtype=dtype)


def plant(x, runs, c, seed=0):
    """x with the sample times of `runs` ((start, end) pairs) replaced by invalid values (every channel of an (n, ch) x)."""
    v = bad_values(x.dtype.type, c)
    k = seed
    for a, b in runs:
        for i in range(a, b):
            x[i] = v[k % v.size]
            k += 1
    return x


def seam_runs(n):
    """Invalid samples at 0 and n - 1, on both sides of every thread seam (8) near the start and of every chunk seam (2048), and runs
    across each chunk seam."""
    runs = [(0, 1), (n - 1, n)]
    for s in (8, 16, 256):
        runs += [(s - 1, s), (s + 1, s + 2)] if s % 16 else [(s, s + 1), (s - 2, s - 1)]
    for s in range(CHUNK, n + 1, CHUNK):
        runs += [(s - 40, s - 38), (s - 9, s - 8), (s - 3, s + 5), (s + 7, s + 9), (s + 100, s + 101)]
        if s == 2 * CHUNK:
            runs += [(s - 1, s), (s + 20, s + 21)]                      # ends exactly on the seam; the next chunk starts valid
    return sorted({(max(a, 0), min(b, n)) for a, b in runs if min(b, n) > max(a, 0)})


def size_cases(n, dtype):
    """The layouts at n samples: the seam runs, nothing invalid, everything invalid, each at c = inf (fp32) and at the dtype's finite
    ceilings; traps in front of the base and past n."""
    cs = (INF, 1.0, FLT_MAX) if dtype is np.float32 else ((32766.0, 32767.0) if dtype is np.int16 else (float(HI24 - 1),))
    out = []
    for k, c in enumerate(cs):
        for name, runs in (("seams", seam_runs(n)), ("none", []), ("all", [(0, n)])):
            x = speech(n, dtype, 31 * n + k)
            if dtype is np.int16 and c == 32767.0:                      # only -32768 is invalid there
                for a, b in runs:
                    x[a:b] = -32768
            else:
                x = plant(x, runs, c, seed=n + k)
            t = trap(11, dtype)
            case = Case(f"{name}, n {n}, c {c}, {np.dtype(dtype).name}", x, c, 1 if k % 2 == 0 else 2, None, t, t)
            if name == "all":
                assert case.rows().tolist() == ([[0, n]] if n >= case.min_len else []), case.name
            if name == "none":
                assert len(case.rows()) == 0, case.name
            out.append(case)
    return out


def table_cases(dtype):
    """Every value of the hand-checked table in one array per ceiling, valid samples between them."""
    cs = (INF, 1.0, FLT_MAX, 0.75, 1e20) if dtype is np.float32 else ((32766.0, 32767.0, 32768.0, INF, 1.0, 0.5) if dtype is np.int16
                                                                       else (float(HI24 - 1), float(HI24), 8388608.0, INF, 1.0))
    vals = table_values(dtype)
    x = np.zeros(3 * vals.size + 5, dtype=dtype)
    x[2:2 + 3 * vals.size:3] = vals
    x[3:3 + 3 * vals.size:3] = vals                                     # each value twice in a row: runs of two, a valid sample between
    return [Case(f"table values at c = {c}, {np.dtype(dtype).name}", x.copy(), c, 1, None, trap(5, dtype), trap(5, dtype)) for c in cs]


def channel_cases(ch, dtype):
    """An (n, ch) file of two chunks and 77 times: a block invalid in every channel (across the seam), channel c's own block where its
    neighbours are valid, and a single invalid element in ONE channel only.  One case per channel and the joint one."""
    n, c = 2 * CHUNK + 77, finite_ceiling(dtype)
    x = speech(n, dtype, 7 * ch, ch)
    plant(x, [(300, 340), (CHUNK - 5, CHUNK + 6)], c, seed=ch)
    own = lambda k: 600 + 30 * k
    v = bad_values(dtype, c)
    for k in range(ch):
        x[own(k):own(k) + 12, k] = v[k % v.size]
    x[1000, ch - 1] = v[0]                                              # NaN (full scale) in one channel only
    before, after = trap(4, dtype, ch), trap(4, dtype, ch)
    out = []
    for k in list(range(ch)) + [-1]:
        case = Case(f"{ch} channels, channel {k}, {np.dtype(dtype).name}", x, c, 1, k, before, after)
        rows = case.rows().tolist()
        if k >= 0:
            assert np.array_equal(case.mask(), dead_mask(np.ascontiguousarray(x[:, k]), c)), case.name
            assert [own(k), 12] in rows and ([1000, 1] in rows) == (k == ch - 1), (case.name, rows)
        else:
            assert rows == [[300, 40], [CHUNK - 5, 11]], rows
        out.append(case)
    return out


def long_case():
    """An fp32 file of 1026 chunks and 5 samples, 1027 workgroups: the carry scan takes two tiles.  A NaN run spans the tile seam with
    whole dead chunks on both sides of it."""
    seam = TILE * CHUNK
    n = seam + 2 * CHUNK + 5
    x = speech(n, np.float32, 5)
    x[5000:5400] = np.nan
    x[seam - CHUNK - 1000:seam + CHUNK + 200] = np.inf
    x[n - 1] = -np.inf
    c = Case("1027 chunks", x, INF, 2, None, trap(8, np.float32), trap(8, np.float32))
    assert c.rows().tolist() == [[5000, 400], [seam - CHUNK - 1000, 2 * CHUNK + 1200]] and -(-n // CHUNK) == TILE + 3
    return c


def all_cpu_cases():
    out = []
    for dtype in DTYPES:
        out += table_cases(dtype)
        for n in SIZES:
            out += size_cases(n, dtype)
        for ch in (2, 3):
            out += channel_cases(ch, dtype)
    return out
