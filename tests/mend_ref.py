"""The reference of si_mend_runs: least-squares autoregressive interpolation over short runs, with the row statuses,
written from the definition.  Pure Python / numpy, no GPU.

The arithmetic is Python's float -- IEEE float64, one rounding per operation -- or, with exact=True, mpmath at 60 digits: the SAME
code, so the difference of the two is the rounding error of the float64 evaluation and nothing else.  Sums run in index order.

A file is a numpy array (n,) or interleaved (n, ch): float32 in full-scale units, int16, or S24 = int32 values in [-2^23, 2^23 - 1]
that stand for packed 24-bit PCM.  `bug` names one seeded mistake (MISTAKES); None is the definition."""
import math
from dataclasses import dataclass, field

import numpy as np

LONG, AR, LINE, EDGE, NEAR, NONFINITE, BADROW = 0, 1, 2, 3, 4, 5, 6
NAMES = ("LONG", "AR", "LINE", "EDGE", "NEAR", "NONFINITE", "BADROW")
MAX_LEN, MAX_ORDER, MAX_CONTEXT, MAX_RUNS = 64, 32, 1024, 65536
S24 = np.int32
RANGE = {np.int16: (-32768, 32767), S24: (-8388608, 8388607)}
FULL = {np.float32: 1.0, np.int16: 32768.0, S24: 8388608.0}
RIDGE = 1.0 + 1e-9
MISTAKES = ("cross_gap", "no_ridge", "d_sign", "d_left_only", "band_p_minus_1", "b_from_r", "line_inside", "trunc", "near_strict", "edge_strict",
            "adjacent_channel")


# ------------------------------------------------------------------------------------------------------------ statuses from the table
def row_status(runs, i, n, max_len, K, bug=None):
    """The status row i takes from the table alone, or None: the row goes on to the samples."""
    s, m = int(runs[i][0]), int(runs[i][1])
    e = s + m
    if s < 0 or m < 1 or e > n:
        return BADROW
    if m > max_len:
        return LONG
    if (s - K <= 0 or e + K >= n) if bug == "edge_strict" else (s - K < 0 or e + K > n):
        return EDGE
    if i > 0:
        pe = int(runs[i - 1][0]) + int(runs[i - 1][1])
        if (pe >= s - K) if bug == "near_strict" else (pe > s - K):
            return NEAR
    if i + 1 < len(runs):
        ns = int(runs[i + 1][0])
        if (ns <= e + K) if bug == "near_strict" else (ns < e + K):
            return NEAR
    return None


# ------------------------------------------------------------------------------------------------------------ the model
def _num(exact):
    if not exact:
        return float, math.sqrt, math.isfinite
    import mpmath
    mpmath.mp.dps = 60
    return mpmath.mpf, mpmath.sqrt, mpmath.isfinite


def line(xa, xb, m, F=float):
    """u_i = xa + (i + 1) / (m + 1) * (xb - xa)."""
    return [xa + (F(i + 1) / F(m + 1)) * (xb - xa) for i in range(m)]


def solve(w, K, m, p, exact=False, bug=None):
    """w: the window x[s - K .. e + K) as exact numbers (the entries [K, K + m) are not read) -> (AR or LINE, u (m numbers), E_p / r[0] or
    None when the recursion did not finish)."""
    F, sqrt, finite = _num(exact)
    w = [F(float(v)) for v in w]
    W = 2 * K + m
    assert len(w) == W
    known = lambda t: t < K or t >= K + m
    xa, xb = (w[K], w[K + m - 1]) if bug == "line_inside" else (w[K - 1], w[K + m])
    r = []
    for k in range(p + 1):
        acc = F(0.0)
        if bug == "cross_gap":
            for t in range(W - k):
                if known(t) and known(t + k):
                    acc = acc + w[t] * w[t + k]
        else:
            for t in range(K - k):
                acc = acc + w[t] * w[t + k]
            for t in range(K + m, W - k):
                acc = acc + w[t] * w[t + k]
        r.append(acc)
    if bug != "no_ridge":
        r[0] = r[0] * F(RIDGE)
    if r[0] == 0:
        return LINE, line(xa, xb, m, F), None
    a, E = [F(1.0)] + [F(0.0)] * p, r[0]
    for i in range(1, p + 1):
        acc = r[i]
        for j in range(1, i):
            acc = acc + a[j] * r[i - j]
        kap = -acc / E
        old = list(a)
        for j in range(1, i):
            a[j] = old[j] + kap * old[i - j]
        a[i] = kap
        E = E * (F(1.0) - kap * kap)
        if not E > 0 or not finite(E):
            return LINE, line(xa, xb, m, F), None
    ratio = float(E / r[0])
    if bug == "b_from_r":
        b = list(r)
    else:
        b = []
        for k in range(p + 1):
            acc = F(0.0)
            for j in range(p - k + 1):
                acc = acc + a[j] * a[j + k]
            b.append(acc)
    band = p - 1 if bug == "band_p_minus_1" else p
    B = [[b[abs(i - j)] if abs(i - j) <= band else F(0.0) for j in range(m)] for i in range(m)]
    d = []
    for i in range(m):
        c, acc = K + i, F(0.0)
        for t in range(max(c - band, 0), min(c + band, W - 1) + 1):
            if known(t) and not (bug == "d_left_only" and t >= K):
                acc = acc + b[abs(t - c)] * w[t]
        d.append(acc if bug == "d_sign" else -acc)
    L = [[F(0.0)] * m for _ in range(m)]
    for j in range(m):
        piv = B[j][j]
        for k in range(j):
            piv = piv - L[j][k] * L[j][k]
        if not piv > 0:
            return LINE, line(xa, xb, m, F), ratio
        L[j][j] = sqrt(piv)
        for i in range(j + 1, m):
            v = B[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    u = [F(0.0)] * m
    for i in range(m):
        v = d[i]
        for k in range(i):
            v = v - L[i][k] * u[k]
        u[i] = v / L[i][i]
    for i in range(m - 1, -1, -1):
        v = u[i]
        for k in range(i + 1, m):
            v = v - L[k][i] * u[k]
        u[i] = v / L[i][i]
    return AR, u, ratio


# ------------------------------------------------------------------------------------------------------------ the store rule
def store(u, dtype, bug=None):
    """One float64 result as the sample that is stored: fp32 rounds once; PCM is rint, ties to even, clamped to the type's range."""
    if dtype is np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            return np.float32(u)
    lo, hi = RANGE[dtype]
    v = math.trunc(u) if bug == "trunc" else round(u)              # Python's round(float) is to nearest, ties to even, exact
    return dtype(min(max(v, lo), hi))


def result_finite(u, dtype):
    return bool(np.isfinite(store(u, dtype))) if dtype is np.float32 else math.isfinite(u)


def sample_type(x):
    t = x.dtype.type
    assert t in (np.float32, np.int16, S24), x.dtype
    return t


# ------------------------------------------------------------------------------------------------------------ the call
@dataclass
class Result:
    y: np.ndarray                                     # the repaired file, x's dtype and shape
    status: np.ndarray                                # int32 (R,)
    u: list = field(default_factory=list)             # per row: the m unrounded results (float64, or mpf when exact) or None
    ratio: list = field(default_factory=list)         # per row: E_p / r[0] of the fit, or None
    peak: list = field(default_factory=list)          # per row: P = max |window| over the 2 K context samples, or None


def mend(x, runs, max_len=64, order=32, context=512, channel=None, exact=False, bug=None):
    """si_mend_runs on a host array: -> Result.  x is not modified.  runs: (R, 2) rows (start, len)."""
    assert 1 <= max_len <= MAX_LEN and 2 <= order <= MAX_ORDER and 4 * order <= context <= MAX_CONTEXT
    dtype = sample_type(x)
    y = x.copy()
    col = x if x.ndim == 1 else x[:, ((channel + 1) % x.shape[1]) if bug == "adjacent_channel" else channel]
    out = y if y.ndim == 1 else y[:, channel]
    n, p, K = x.shape[0], int(order), int(context)
    runs = [(int(s), int(m)) for s, m in np.asarray(runs).reshape(-1, 2)]
    res = Result(y, np.zeros(len(runs), np.int32))
    for i, (s, m) in enumerate(runs):
        st = row_status(runs, i, n, max_len, K, bug)
        u = ratio = peak = None
        if st is None:
            win = col[s - K:s + m + K]
            ctx = np.concatenate([win[:K], win[K + m:]])
            if dtype is np.float32 and not np.all(np.isfinite(ctx)):
                st = NONFINITE
            else:
                peak = float(np.max(np.abs(ctx.astype(np.float64))))
                st, u, ratio = solve([float(v) for v in win], K, m, p, exact, bug)     # the damaged samples ride along; only a mistake reads them
                if not all(result_finite(float(v), dtype) for v in u):
                    st = NONFINITE
                else:
                    for k in range(m):
                        out[s + k] = store(float(u[k]), dtype, bug)
        res.status[i] = st
        res.u.append(u)
        res.ratio.append(ratio)
        res.peak.append(peak)
    return res


def check_runs(runs, n):
    """The host-list rule of engine.mend_runs: sorted, disjoint and in range, or a ValueError naming the row."""
    end = 0
    for i, (s, m) in enumerate(runs):
        if m < 1 or s < 0 or s + m > n:
            raise ValueError(f"row {i}")
        if s < end:
            raise ValueError(f"row {i}")
        end = s + m


# ------------------------------------------------------------------------------------------------------------ signals
def three_sines(n):
    """The quality signal of DESIGN.md 4.31: three sinusoids, peak about 1.9."""
    t = np.arange(n, dtype=np.float64)
    return np.sin(0.0731 * t + 0.3) + 0.6 * np.sin(0.2113 * t + 1.1) + 0.3 * np.sin(0.4907 * t + 2.0)


def voiced(n, seed, noise=0.02):
    """Voiced speech-like: harmonics of a slowly moving pitch plus white noise, |x| <= 0.3, float64."""
    g = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f0 = 0.02 + 0.004 * g.random()
    x = sum(g.uniform(0.3, 1.0) / h * np.sin(2 * np.pi * f0 * h * t + g.uniform(0, 6.28)) for h in range(1, 7))
    x = x / np.max(np.abs(x)) * 0.27 + noise * g.standard_normal(n).clip(-1.5, 1.5)
    return np.clip(x, -0.3, 0.3)


def ar2(n, seed):
    """An AR(2) resonance driven by white noise, scaled to |x| <= 0.3, float64."""
    g = np.random.default_rng(seed)
    e = g.standard_normal(n + 200)
    x = np.zeros(n + 200)
    for t in range(2, n + 200):
        x[t] = 1.6 * x[t - 1] - 0.81 * x[t - 2] + e[t]
    x = x[200:]
    return x / np.max(np.abs(x)) * 0.3


def as_type(x64, dtype):
    """A float64 signal in full-scale units as a file of `dtype`: fp32 rounds, PCM scales by full scale and rounds."""
    if dtype is np.float32:
        return x64.astype(np.float32)
    lo, hi = RANGE[dtype]
    return np.clip(np.rint(x64 * FULL[dtype]), lo, hi).astype(dtype)
