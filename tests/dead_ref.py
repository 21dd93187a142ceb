"""Held-sample and peak-relative dropouts: the numpy reference of si_dead_runs and the case builders of
tests/test_dead_ref.py and tests/test_gpu_dead.py.  A plain module, imported by name; importing it needs no GPU.

The contract, for one channel x[0 .. n) (fp32 or int16):
    peak      the largest |x[i]| over the finite samples (int16 magnitudes in int32); 0 when there is none
    T         max(thr, fl32(rel * peak)), one fp32 multiply; rel == 0: T = thr and the peak is not looked at
    quiet(i)  |x[i]| <= T                        (tests/detect_ref.py's quiet_mask: NaN loud, -0.0 quiet)
    link(i)   |x[i] - x[i - 1]| <= tol for 1 <= i < n; fp32: one fp32 subtraction, int16: the subtraction in int32
    held(i)   link(i) or link(i + 1)
    dead(i)   (kind & QUIET and quiet(i)) or (kind & HELD and held(i))
An interleaved file (n, ch): channel c is the column x[:, c], its peak its own; channel -1 is joint -- a time is dead when every column
is, each by its own links, against ONE threshold from the peak over all elements.

Every function takes bug=<name>, one of MISTAKES, which seeds that mistake into the reference: tests/test_dead_ref.py shows that each one
changes the expected rows of at least one case, i.e. that the cases can tell."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from tests import detect_ref as D

QUIET, HELD, ANY = 1, 2, 3
CHUNK, TILE = D.CHUNK, D.CARRY_TILE          # DT_CHUNK and DT_TILE of detect_kernels.hip (the peak's final reduce walks the same tiles)
THR = D.THR                                  # the absolute thresholds the builders are written for: 2^-7 and 3, both exact in fp32
MISTAKES = ("link_across_n", "adjacent_channel", "int16_wrap", "peak_inf", "held_left_only")
f32 = np.float32


def _mag(x):
    x = np.asarray(x)
    return np.abs(x.astype(np.int32)).astype(f32) if x.dtype == np.int16 else np.abs(x.astype(f32))


def peak_ref(x, channel=None, bug=None):
    """The largest finite magnitude as fp32.  x (n,), or (n, ch) with channel = a column, or -1 for all elements."""
    x = np.asarray(x)
    col = x if x.ndim == 1 or channel is None or channel < 0 else x[:, channel]
    m = _mag(col).reshape(-1)
    keep = ~np.isnan(m) if bug == "peak_inf" else np.isfinite(m)
    return f32(m[keep].max()) if keep.any() else f32(0)


def threshold_ref(x, thr, rel, channel=None, bug=None):
    """T as fp32: max(thr, fl32(rel * peak)); rel == 0 gives thr without a peak."""
    if float(rel) == 0.0:
        return f32(thr)
    with np.errstate(over="ignore", invalid="ignore"):
        return max(f32(thr), f32(rel) * peak_ref(x, channel, bug))


def link_mask(col, tol, before=None, after=None, bug=None):
    """n + 1 booleans: entry i is link(i) -- between samples i - 1 and i -- for i = 0 .. n; entries 0 and n are False (no such link).
    before / after: what lies in memory at times -1 and n.  The reference never looks at them; bug="link_across_n" does."""
    col = np.asarray(col)
    n = col.size
    ext = np.concatenate(([col[0] if before is None else before], col, [col[-1] if after is None else after])).astype(col.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if col.dtype == np.int16:
            d = (ext[1:] - ext[:-1]) if bug == "int16_wrap" else (ext[1:].astype(np.int32) - ext[:-1].astype(np.int32))
            link = np.abs(d.astype(np.int32)).astype(f32) <= f32(tol)
        else:
            link = np.abs(ext[1:].astype(f32) - ext[:-1].astype(f32)) <= f32(tol)
    if not (bug == "link_across_n" and before is not None):
        link[0] = False
    if not (bug == "link_across_n" and after is not None):
        link[n] = False
    return link


def _dead_column(col, kind, T, tol, before=None, after=None, bug=None):
    dead = np.zeros(col.size, dtype=bool)
    if kind & QUIET:
        dead |= D.quiet_mask(col, T)
    if kind & HELD:
        link = link_mask(col, tol, before, after, bug)
        dead |= link[:-1] if bug == "held_left_only" else (link[:-1] | link[1:])
    return dead


def dead_mask(x, kind, thr=0.0, rel=0.0, tol=0.0, channel=None, before=None, after=None, bug=None):
    """dead(i) per sample time.  x (n,) with channel None, or (n, ch) with channel = a column or -1 (joint).  before / after: the
    elements in memory in front of x and behind it (one sample time each; read only by a seeded mistake)."""
    x = np.asarray(x)
    assert kind in (QUIET, HELD, ANY)
    T = threshold_ref(x, thr, rel, channel, bug)
    if x.ndim == 1:
        return _dead_column(x, kind, T, tol, before, after, bug)
    n, ch = x.shape
    cols = range(ch) if channel < 0 else [channel]
    if bug == "adjacent_channel":                                      # the neighbours are the adjacent ELEMENTS of the file
        flat = x.reshape(-1)
        dead = _dead_column(flat, kind, T, tol).reshape(n, ch)
        return np.all(dead[:, list(cols)], axis=1)
    pick = lambda row, c: None if row is None else np.asarray(row).reshape(-1)[c]
    return np.all(np.stack([_dead_column(x[:, c], kind, T, tol, pick(before, c), pick(after, c), bug) for c in cols], axis=1), axis=1)


def runs_of(mask, min_len):
    """A boolean mask -> its maximal runs of at least min_len as int32 (start, len) rows (tests/detect_ref.py's extraction)."""
    return D.quiet_runs_ref(np.where(mask, f32(0), f32(1)), 0.0, min_len)


def dead_runs_ref(x, kind, thr=0.0, rel=0.0, tol=0.0, min_len=1, channel=None, before=None, after=None, bug=None):
    return runs_of(dead_mask(x, kind, thr, rel, tol, channel, before, after, bug), min_len)


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    """One call of si_dead_runs and what surrounds its input in memory.  x (n,) or (n, ch); before / after: one sample time of
    elements planted in front of the base and behind the input (the halo traps: equal to x[0] / x[n - 1], or larger than the peak)."""
    name: str
    x: np.ndarray
    kind: int
    thr: float = 0.0
    rel: float = 0.0
    tol: float = 0.0
    min_len: int = 1
    channel: Optional[int] = None
    before: Optional[np.ndarray] = None
    after: Optional[np.ndarray] = None

    def args(self):
        return dict(kind=self.kind, thr=self.thr, rel=self.rel, tol=self.tol, channel=self.channel)

    def mask(self, bug=None):
        return dead_mask(self.x, before=self.before, after=self.after, bug=bug, **self.args())

    def rows(self, bug=None):
        return runs_of(self.mask(bug), self.min_len)

    def threshold(self):
        return threshold_ref(self.x, self.thr, self.rel, self.channel)

    def memory(self):
        """(flat elements: before | x | after, the index x starts at)."""
        ch = 1 if self.x.ndim == 1 else self.x.shape[1]
        row = lambda r: np.zeros(ch, self.x.dtype) if r is None else np.asarray(r, self.x.dtype).reshape(ch)
        return np.concatenate([row(self.before), self.x.reshape(-1), row(self.after)]), ch


def materialize(quiet_only, held, dtype, seed=0):
    """Two disjoint boolean masks -> (samples, {kind: the dead mask they realise}) under THR[dtype] and tol = 0.
    held: runs of at least two samples each, one constant per run -- loud for the even-numbered runs, quiet for the odd ones; a run's
    neighbours differ from it.  quiet_only: quiet samples that differ from both neighbours (0, +-thr, subnormals ... in a cycle).
    Everything else is loud and differs from both neighbours: random, with NaN, +-inf and the first value above thr planted.
    The three masks are asserted against dead_mask."""
    quiet_only, held = np.asarray(quiet_only, dtype=bool), np.asarray(held, dtype=bool)
    assert not (quiet_only & held).any()
    n = held.size
    rng = np.random.default_rng(seed)
    thr = THR[dtype]
    if dtype is np.float32:
        t = f32(thr)
        q_vals = np.array([0.0, t, -t, t / 2, -0.0, 1e-40, -1e-40, np.nextafter(t, f32(0))], dtype=f32)
        l_vals = np.array([np.nan, np.inf, -np.inf, np.nextafter(t, f32(1)), -np.nextafter(t, f32(1))], dtype=f32)
        x = ((rng.random(n) * 0.9 + 0.02) * rng.choice([-1.0, 1.0], n)).astype(f32)
        held_val = lambda k: f32(0.5 + (k % 16) / 64.0) * (1 if k % 4 else -1) if k % 2 == 0 else f32([t / 4, -t / 4, 3e-39][(k // 2) % 3])
    else:
        q_vals = np.array([0, 3, -3, 1, -2, 2], dtype=np.int16)
        l_vals = np.array([-32768, 32767, 4, -4], dtype=np.int16)
        x = (rng.integers(5, 32767, n) * rng.choice([-1, 1], n)).astype(np.int16)
        held_val = lambda k: np.int16([1000 + k % 16, -32768, 32767, -(2000 + k % 16)][(k // 2) % 4]) if k % 2 == 0 else np.int16([-1, 0, 3][(k // 2) % 3])
    loud = ~quiet_only & ~held
    li = np.flatnonzero(loud)
    x[li[::3]] = l_vals[np.arange(li[::3].size) % l_vals.size]        # every third loud sample is a special one
    qi = np.flatnonzero(quiet_only)
    x[qi] = q_vals[np.arange(qi.size) % q_vals.size]
    held_quiet = np.zeros(n, dtype=bool)
    for k, (a, l) in enumerate(runs_of(held, 1).tolist()):
        assert l >= 2, ("a held run of one sample does not exist", a)
        x[a:a + l] = held_val(k)
        held_quiet[a:a + l] = k % 2 == 1
    for i in np.flatnonzero(~held):                                    # no link by accident: another quiet value, a loud one moved a little
        near = [x[j] for j in (i - 1, i + 1) if 0 <= j < n]
        if x[i] in near:
            pool = q_vals if quiet_only[i] else ([x[i] * f32(0.75), x[i] * f32(0.5)] if dtype is np.float32 else [x[i] // 2 + 9 * d for d in (1, 2, 3)])
            x[i] = [v for v in pool if v not in near][0]
    want = {QUIET: quiet_only | held_quiet, HELD: held, ANY: quiet_only | held}
    for kind, m in want.items():
        got = dead_mask(x, kind, thr)
        assert np.array_equal(got, m), (kind, np.flatnonzero(got != m)[:8].tolist())
    return x, want


SEAM_N = (1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4101, 6144)
MIN_LEN = 5


def seam_masks(n):
    """(name, quiet_only mask, held mask, min_len) per placement at n samples: held runs of exactly two samples straddling every
    multiple of 8 (thread seam), 512 (wave seam) and 2048 (chunk seam) that fits; runs ending on, starting on and crossing each wave and
    chunk seam; whole held chunks inside a run (the carry); lengths MIN_LEN - 1, MIN_LEN, MIN_LEN + 1; held pairs at (0, 1) and at
    (n - 2, n - 1); and quiet runs beside them."""
    z = lambda: np.zeros(n, dtype=bool)
    m = D.mask_of
    fit = lambda runs: [(a, b) for a, b in runs if a >= 0 and b <= n and b - a >= 2]
    out = [("nothing held", z(), z(), 1), ("alternating quiet", np.arange(n) % 2 == 0, z(), 1)]
    if n >= 2:
        out += [("all held", z(), np.ones(n, dtype=bool), 1), ("all held, min_len n + 1", z(), np.ones(n, dtype=bool), n + 1),
                ("a pair at each end", m(n, [(3, 4)]) if n > 6 else z(), m(n, fit([(0, 2), (n - 2, n)])), 1)]
    for phase in (0, 1, 2):                                            # pairs across every third multiple of 8, so that they stay apart
        pairs = fit([(s - 1, s + 1) for s in range(8 * (phase + 1), n, 24)])
        if pairs:
            out.append((f"pairs across the multiples of 8, phase {phase}", z(), m(n, pairs), 2))
    seams = sorted({s for s in list(range(512, n + 1, 512))})
    for s in seams:
        what = "chunk" if s % CHUNK == 0 else "wave"
        out += [(f"crossing the {what} seam {s}", m(n, [(s - 30, s - 25)]), m(n, fit([(s - 8, min(s + 12, n))])), 1),
                (f"ending on the last sample before {s}", m(n, [(s, s + 1)]), m(n, fit([(s - 48, s)])), 1),
                (f"starting on sample {s}", m(n, [(s - 1, s)]), m(n, fit([(s, min(s + 52, n))])), 1),
                (f"a pair on each side of {s}", z(), m(n, fit([(s - 2, s), (s + 1, s + 3)])), 1),
                (f"a pair across {s}", z(), m(n, fit([(s - 1, s + 1)])), 2)]
    if n > CHUNK:                                                     # whole chunks inside one held run: the carry
        out += [("whole chunks inside a held run from chunk 0", z(), m(n, [(CHUNK - 1, n)]), 1),
                ("whole chunks inside a held run that ends early", m(n, [(0, 3)]), m(n, [(5, n - 3)]), 1),
                ("a held run of exactly the chunks 1 ..", z(), m(n, fit([(CHUNK, n)])), 1)]
    runs, a = [], 3                                                    # lengths 4, 5, 6 in a chunk and across each chunk seam
    for _ in range(3):
        for l in (MIN_LEN - 1, MIN_LEN, MIN_LEN + 1):
            runs.append((a, a + l))
            a += l + 2
    for k in range(1, n // CHUNK + 1):
        for i, l in enumerate((MIN_LEN - 1, MIN_LEN, MIN_LEN + 1)):
            runs.append((k * CHUNK - 2 - 40 * i, k * CHUNK - 2 - 40 * i + l))
        runs += [(k * CHUNK - 2, k * CHUNK + 2), (k * CHUNK + 10, k * CHUNK + 15), (k * CHUNK + 100 - 3, k * CHUNK + 100 + 3)]
    runs = fit(runs)
    if runs:
        hm = m(n, runs[0::2])
        qm = m(n, runs[1::2]) & ~hm
        out += [(f"lengths 4, 5, 6 at min_len {ml}", qm, hm, ml) for ml in (MIN_LEN, 1, MIN_LEN + 2)]
    return out


def trap_rows(x, peak_trap=False):
    """The elements to plant in front of x and behind it: copies of x[0] and x[n - 1] (a link to either would extend a run), or, for
    the peak, a magnitude above everything in x."""
    x = np.asarray(x)
    if peak_trap:
        big = np.int16(-32768) if x.dtype == np.int16 else f32(3.0e38)
        return np.full(x[0].shape, big, x.dtype), np.full(x[0].shape, big, x.dtype)
    return x[0].copy(), x[-1].copy()


def seam_cases(n, dtype):
    """Case objects of seam_masks(n) for kinds 1, 2 and 3 on the same samples, x[-1] == x[0] and x[n] == x[n - 1] planted around them."""
    out = []
    for k, (name, qm, hm, min_len) in enumerate(seam_masks(n)):
        x, want = materialize(qm, hm, dtype, seed=n + k)
        before, after = trap_rows(x)
        for kind in (QUIET, HELD, ANY):
            c = Case(f"{name}, kind {kind}", x, kind, THR[dtype], 0.0, 0.0, min_len, None, before, after)
            assert np.array_equal(c.mask(), want[kind]), c.name
            out.append(c)
    return out


def value_cases():
    """The value edges, each with its expected mask written out by hand."""
    nan, inf = f32(np.nan), f32(np.inf)
    t = f32(0.25)
    up = np.nextafter(t, f32(1))
    E = []

    def add(name, x, kind, want, **kw):
        c = Case(name, np.asarray(x), kind, **kw)
        assert c.mask().tolist() == [bool(v) for v in want], (name, c.mask().astype(int).tolist())
        E.append(c)

    add("pairs at both ends", f32([1, 1, 2, 3, 4, 4]), HELD, [1, 1, 0, 0, 1, 1])
    add("n = 1 is never held", f32([0.5]), HELD, [0])
    add("n = 1 is quiet", f32([0.0]), ANY, [1])
    add("|diff| == tol and the next float above", f32([1.0, 1.0 + t, 3.0, 0.0, up, 5.0, 5.0 - t, 7.0]), HELD, [1, 1, 0, 0, 0, 1, 1, 0], tol=float(t))
    add("0.0 against -0.0", f32([1.0, 0.0, -0.0, 2.0]), HELD, [0, 1, 1, 0])
    add("NaN and inf - inf", f32([nan, nan, 1, inf, inf, 2, -inf, -inf, inf, 3, 3]), HELD, [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1])
    add("inf - inf under an infinite tol", f32([inf, inf, 1, 2, nan, 3]), HELD, [0, 1, 1, 1, 0, 0], tol=float("inf"))
    add("subnormal steps are steps", f32([1e-40, 2e-40, 2e-40, 0.0]), HELD, [0, 1, 1, 0])
    add("32767 | -32768 in int16", np.int16([32767, -32768, 5, -32768, 32767, 9]), HELD, [0, 0, 0, 0, 0, 0], tol=1.0)
    add("32767 | -32768 at tol 65535", np.int16([32767, -32768]), HELD, [1, 1], tol=65535.0)
    add("int16 steps of tol and tol + 1", np.int16([10, 12, 15, 17, 20, 23]), HELD, [1, 1, 1, 1, 0, 0], tol=2.0)
    add("any = quiet or held", f32([0, 1, 5, 5, 2, 0.25, 0.3]), ANY, [1, 0, 1, 1, 0, 1, 0], thr=0.25)
    add("kind quiet ignores held_tol", f32([0, 1, 5, 5, 2, 0.25, 0.3]), QUIET, [1, 0, 0, 0, 0, 1, 0], thr=0.25, tol=9.0)
    # T: rel * peak in fp32, the peak over the finite samples
    pk = f32(0.9)
    while f32(1e-3) * pk == f32(1e-3 * float(pk)):                     # a peak whose fp32 product is not the rounded exact product
        pk = np.nextafter(pk, f32(1))
    T = f32(1e-3) * pk
    x = f32([0.7, -pk, nan, inf, -inf, T, -np.nextafter(T, f32(1)), np.nextafter(T, f32(0)), 0.0])
    c = Case("rel 1e-3: T is the fp32 product", x, QUIET, 0.0, 1e-3)
    assert c.threshold().tobytes() == T.tobytes() and T != f32(1e-3 * float(pk))
    assert c.mask().tolist() == [False] * 5 + [True, False, True, True]
    E.append(c)
    add("thr above rel * peak wins", f32([1.0, 0.01, 0.02, 0.001]), QUIET, [0, 1, 0, 1], thr=0.01, rel=1e-3)
    add("all NaN: peak 0, T = thr", f32([nan, nan, nan]), ANY, [0, 0, 0], thr=0.5, rel=1.0)
    assert peak_ref(f32([nan, nan])) == 0 and threshold_ref(f32([nan, inf]), 0.5, 1.0) == f32(0.5)
    add("rel = 1: the peak itself is quiet", f32([0.5, -2.0, inf, 1.0]), QUIET, [1, 1, 0, 1], rel=1.0)
    add("int16 peak 32768", np.int16([-32768, 32, 33, -32, 0]), QUIET, [0, 1, 0, 1, 1], rel=2.0 ** -10)
    add("the seeded peak mistake shows", f32([1.0, inf, 0.0005, 0.5]), QUIET, [0, 0, 1, 0], rel=1e-3)
    return E


def peak_position_cases(dtype):
    """The peak at the first sample, at the last sample and in a partial last chunk; a larger magnitude planted on both sides of x."""
    out = []
    n = 2 * CHUNK + 300
    amp = 0.01 if dtype is np.float32 else 300                         # the floor: magnitudes in [amp / 10, amp]
    top = f32(0.8) if dtype is np.float32 else np.int16(-30000)
    for name, at in (("first sample", 0), ("last sample", n - 1), ("partial last chunk", 2 * CHUNK + 17), ("last sample of chunk 0", CHUNK - 1)):
        rng = np.random.default_rng(at)
        x = ((rng.random(n) * 0.9 + 0.1) * amp * rng.choice([-1.0, 1.0], n)).astype(dtype)
        x[at] = top
        x[100:160] = (x[100:160].astype(np.float64) / 64).astype(dtype)          # a mute at 1 / 64 of the floor: found only through the peak
        before, after = trap_rows(x, peak_trap=True)
        rel = 2.0 ** -10
        c = Case(f"peak at the {name}", x, QUIET, 0.0, rel, 0.0, 8, None, before, after)
        assert peak_ref(x) == _mag(np.asarray([top]))[0] and c.rows().tolist() == [[100, 60]] and c.mask().sum() == 60
        out.append(c)
    return out


def interleave(cols):
    return np.ascontiguousarray(np.stack(cols, axis=1))


def channel_cases(ch, dtype):
    """An (n, ch) file, n = two chunks and 77 times: every channel its own materialized masks, equal values planted in ADJACENT
    channels of one sample time and across the time seam (element (i, ch - 1) == element (i + 1, 0)) at loud, unheld samples.
    One case per channel and kind, and the joint ones; the per-channel cases carry the column's own expected mask."""
    n = 2 * CHUNK + 77
    thr = THR[dtype]
    cols, wants = [], []
    for c in range(ch):
        hm = D.mask_of(n, [(8 * c + 5, 8 * c + 7), (CHUNK - 3 - c, CHUNK + 4 + c), (3000, 3400), (n - 2 - c % 2, n), (500, 520)])
        qm = D.mask_of(n, [(40 + c, 60 + c), (CHUNK + 100, CHUNK + 130 + c), (530, 540)]) & ~hm
        if c == 1:
            hm = D.mask_of(n, [(500, 520), (3100, 3300)])             # (one channel with little in common with the others)
            qm = D.mask_of(n, [(530, 540), (45, 50)])
        x, want = materialize(qm, hm, dtype, seed=100 * ch + c)
        cols.append(x)
        wants.append(want)
    x = interleave(cols)
    plain = np.ones(n, dtype=bool)
    for w in wants:
        plain &= ~w[ANY]
    for w in wants:                                                    # also keep the neighbouring times clear: nothing else changes
        for s in (-1, 1):
            plain &= ~np.roll(w[ANY], s)
    spots = np.flatnonzero(plain)[10::97]
    assert spots.size >= 20
    planted = 0
    for k, i in enumerate(spots):                                      # only finite loud values are copied
        c = k % ch
        if not np.isfinite(float(x[i, c])):
            continue
        ti, tc = (i, c + 1) if c + 1 < ch else (i + 1, 0)             # adjacent channels of one sample time | across the time seam
        if 0 < ti < n - 1 and plain[ti] and x[i, c] not in (x[ti - 1, tc], x[ti + 1, tc]):
            x[ti, tc] = x[i, c]
            planted += 1
    assert planted >= 15
    out = []
    before, after = trap_rows(x)
    for kind in (QUIET, HELD, ANY):
        for c in range(ch):
            case = Case(f"{ch} channels, channel {c}, kind {kind}", x, kind, thr, 0.0, 0.0, 2, c, before, after)
            assert np.array_equal(case.mask(), wants[c][kind]) and np.array_equal(case.mask(), dead_mask(x[:, c].copy(), kind, thr)), case.name
            out.append(case)
        joint = Case(f"{ch} channels, joint, kind {kind}", x, kind, thr, 0.0, 0.0, 2, -1, before, after)
        assert np.array_equal(joint.mask(), np.all([w[kind] for w in wants], axis=0)), joint.name
        out.append(joint)
    # the held masks the columns were built from survive the planting: the common run [500, 520) is in every joint answer
    assert [500, 20] in out[2 * (ch + 1) - 1].rows().tolist()
    # the peak: one column's is its own, the joint one is the file's
    loud = x.copy()
    fin = np.isfinite(loud.astype(np.float64))
    loud[~fin] = 0
    loud[(_mag(loud) > (0.5 if dtype is np.float32 else 16000))] = 0
    loud[7, ch - 1] = f32(0.9) if dtype is np.float32 else np.int16(30000)
    for c in (0, ch - 1, -1):
        case = Case(f"{ch} channels, peak of channel {c}", loud, QUIET, 0.0, 2.0 ** -6, 0.0, 1, c, *trap_rows(loud, peak_trap=True))
        out.append(case)
    assert out[-3].threshold() < out[-2].threshold() == out[-1].threshold()
    return out


def long_case(dtype):
    """1026 chunks and 5 samples, 1027 workgroups: the peak's final reduce and the carry take two tiles.  A held run spans chunks 1023 | 1024 with whole
    held chunks on both sides of the tile seam, the peak lies in the last chunk, and a mute at a fraction of the noise floor is found
    through it."""
    seam = TILE * CHUNK
    n = seam + 2 * CHUNK + 5
    rng = np.random.default_rng(5)
    if dtype is np.float32:
        x = ((rng.random(n) * 0.9 + 0.1) * 0.01 * rng.choice([-1.0, 1.0], n)).astype(f32)
        x[n - 3] = f32(0.75)
        x[5000:5400] = x[5000:5400] / f32(4096)
        x[seam - CHUNK - 1000:seam + CHUNK + 200] = f32(0.004)
    else:
        x = ((rng.integers(15, 150, n) * 2 + np.arange(n) % 2) * rng.choice([-1, 1], n)).astype(np.int16)   # odd | even: no two neighbours equal
        x[n - 3] = 16384
        x[5000:5400] = rng.integers(-1, 2, 400)
        x[seam - CHUNK - 1000:seam + CHUNK + 200] = 120
    c = Case("1027 chunks", x, ANY, 0.0, 2.0 ** -12, 0.0, 64, None, *trap_rows(x, peak_trap=True))
    rows = c.rows().tolist()
    assert [seam - CHUNK - 1000, 2 * CHUNK + 1200] in rows and [5000, 400] in rows and len(rows) == 2, rows[:8]
    assert -(-n // CHUNK) == TILE + 3
    return c


def all_cpu_cases():
    """Every case a CPU test walks (the long one apart)."""
    out = list(value_cases())
    for dtype in (np.float32, np.int16):
        for n in (1, 2, 9, 513, 2049, 4101):
            out += seam_cases(n, dtype)
        out += peak_position_cases(dtype)
        for ch in (2, 3):
            out += channel_cases(ch, dtype)
    return out
