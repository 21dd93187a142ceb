"""Clicks and pops by locally scaled AR prediction error: the reference of si_impulse_runs and si_impulse_residual and
the case builders of tests/test_impulse_ref.py and tests/test_gpu_impulse.py.  A plain module, imported by name; importing it needs no GPU.

The contract, for one channel x[0 .. n), p = order, h = half, g = guard, blocks of B = 512.  x is fp32, int16, or int32 holding 24-bit
values (the device gets them packed); values enter as the file's own numbers in float64.
    T         max(thr, fl32(rel * peak)): tests/dead_ref.py's threshold_ref.  T = 0 is allowed.
    F_b       the fit window of block b = [b B, min(n, (b + 1) B)): [max(0, b B - 256), min(n, (b + 1) B + 256))
    r[k]      sum of w[t] w[t + k] over F_b, k = 0 .. p, as EIGHT INTERLEAVED PARTIAL SUMS (partial q: t = q, q + 8, ... from F_b's first
              sample, in index order, from +0.0) added in the order q = 0 .. 7; then r[0] *= 1 + 1e-9
    a         Levinson-Durbin as tests/mend_ref.py states it; (1, 0, ..., 0) when |F_b| <= p, r[0] == 0, or E <= 0 / non-finite at a step
    badblk    a NaN or +-inf lies in F_b: every t of the block is bad
    e(t)      p <= t < n: a_0 x[t] + a_1 x[t - 1] + ... + a_p x[t - p], added in this order, block(t)'s model; sq = fl64(e e)
    L, R      [max(p, t - h), t - g - 1], [t + g + 1, min(n - 1, t + h)]; cnt = |L| + |R|; S = the sum of sq over both, by additions only
    hot(t)    t >= p, cnt >= h - g, no bad sample at t or in L or R, sq > fl64(T T), fl64(sq cnt) > fl64(fl64(ratio ratio) S)
    dead(j)   hot(t) for some |t - j| <= pad inside [0, n)
An interleaved file (n, ch): channel c is the column x[:, c], its peak its own; channel -1 is joint -- a time is dead when every column's
dead holds, against ONE threshold from the peak over all elements.

The arithmetic is numpy float64, one rounding per operation, in the stated orders -- or, with exact=True, mpmath at 60 digits through the
scalar code (`_lags`, `levinson` and the residual loop of `column`), which with Python floats gives the numpy path's bits (tests/test_impulse_ref.py holds them
together).  The device adds the window's squares in an order of its own, so S is pinned only to cnt 2^-52 S; `Result.margin` is the
smallest relative distance from equality of either comparison over the samples the other conditions admit, and every case builder
asserts it above 2^-20: the decisions then cannot depend on that order.

Every function takes bug=<name>, one of MISTAKES, which seeds that mistake into the reference: tests/test_impulse_ref.py shows that each
one changes the rows or the residuals of at least one case, i.e. that the cases can tell."""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import dead_ref as R
from tests import mend_ref as M

f32, f64 = np.float32, np.float64
S24 = np.int32
BLOCK, WING, PARTS = 512, 256, 8
MAX_ORDER, MAX_HALF, MAX_GUARD, MAX_PAD = 32, 1024, 64, 16
RIDGE = 1.0 + 1e-9
FULL = {np.float32: 1.0, np.int16: 32768.0, S24: 8388608.0}
DTYPES = (np.float32, np.int16, S24)
MISTAKES = ("fit_block_only", "fit_unclipped_n", "no_ridge", "guard_included", "cnt_untruncated", "greater_equal", "no_T", "prev_model_first_p",
            "adjacent_channel", "dilate_one_sided", "model_fp32", "running_sums")
MARGIN = 2.0 ** -20


# ------------------------------------------------------------------------------------------------------------ the model
def _num(exact):
    if not exact:
        return float, math.isfinite
    import mpmath
    mpmath.mp.dps = 60
    return mpmath.mpf, mpmath.isfinite


def _lags(w, p, F):
    """r[0 .. p] of the window w (a list of F numbers) in the stated order, before the correction of r[0]."""
    W, r = len(w), []
    for k in range(p + 1):
        parts = []
        for q in range(PARTS):
            acc = F(0.0)
            for t in range(q, W - k, PARTS):
                acc = acc + w[t] * w[t + k]
            parts.append(acc)
        acc = parts[0]
        for q in range(1, PARTS):
            acc = acc + parts[q]
        r.append(acc)
    return r


def _lags_np(w, p):
    """The same additions in numpy float64: ufunc.accumulate adds strictly in order, and a trailing + 0.0 changes nothing."""
    W, r = w.size, []
    for k in range(p + 1):
        m = max(W - k, 0)
        prod = np.zeros(-(-max(m, 1) // PARTS) * PARTS, f64)
        prod[:m] = w[:m] * w[k:k + m]
        parts = np.add.accumulate(prod.reshape(-1, PARTS), axis=0)[-1]
        acc = parts[0]
        for q in range(1, PARTS):
            acc = acc + parts[q]
        r.append(float(acc))
    return r


def levinson(r, p, W, F=float, finite=math.isfinite, bug=None):
    """-> (a (p + 1 numbers), E_p / r[0] as a float, or None for the delta model)."""
    delta = [F(1.0)] + [F(0.0)] * p
    r = list(r)
    if bug != "no_ridge":
        r[0] = r[0] * F(RIDGE)
    if W <= p or r[0] == 0:
        return delta, None
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
            return delta, None
    return a, float(E / r[0])


def _levinson_fp32(w, p):
    """The seeded mistake "model_fp32": products, sums and the recursion in fp32."""
    w = w.astype(f32)
    r = [f32(np.add.accumulate((w[:w.size - k] * w[k:]).astype(f32))[-1]) if w.size > k else f32(0) for k in range(p + 1)]
    r[0] = f32(r[0] * f32(RIDGE))
    if w.size <= p or r[0] == 0:
        return [1.0] + [0.0] * p, None
    a, E = [f32(1)] + [f32(0)] * p, r[0]
    with np.errstate(all="ignore"):
        for i in range(1, p + 1):
            acc = r[i]
            for j in range(1, i):
                acc = f32(acc + f32(a[j] * r[i - j]))
            kap = f32(-acc / E)
            old = list(a)
            for j in range(1, i):
                a[j] = f32(old[j] + f32(kap * old[i - j]))
            a[i] = kap
            E = f32(E * f32(f32(1) - f32(kap * kap)))
            if not E > 0 or not np.isfinite(E):
                return [1.0] + [0.0] * p, None
    return [float(v) for v in a], float(E / r[0])


@dataclass
class Result:
    e: np.ndarray                                     # float64 (n,): the residual; 0.0 for t < p, NaN for a bad sample
    hot: np.ndarray                                   # bool (n,)
    dead: np.ndarray                                  # bool (n,)
    A: np.ndarray                                     # float64 (n,): sum_j |a_j| |x[t - j]|, the scale of the residual's rounding error
    ratios: list = field(default_factory=list)        # per block: E_p / r[0], or None (the delta model, or a bad block)
    margin: float = math.inf                          # the smallest relative distance from equality of either comparison
    e_exact: list = None                              # exact=True: the residuals as mpf (None where there is none)


def _windows(sq, n, h, gw, exact, bug):
    """(SL, SR) per t over the zero-padded squares: positions [t - h, t - gw - 1] and [t + gw + 1, t + h]."""
    wl = h - gw
    if exact:
        import mpmath
        cs = [mpmath.mpf(0)]
        for v in [mpmath.mpf(0)] * h + list(sq) + [mpmath.mpf(0)] * h:
            cs.append(cs[-1] + v)
        win = lambda i: cs[i + wl] - cs[i]                             # 60 digits: the difference is the sum
        return [win(t) for t in range(n)], [win(t + gw + 1 + h) for t in range(n)]
    pad = np.concatenate([np.zeros(h), np.asarray(sq, f64), np.zeros(h)])
    if bug == "running_sums":
        cs = np.concatenate([np.zeros(1), np.cumsum(pad)])
        win = cs[wl:] - cs[:-wl]
    else:
        win = np.lib.stride_tricks.sliding_window_view(pad, wl).sum(axis=1)   # additions only
    t = np.arange(n)
    return win[t], win[t + gw + 1 + h]


def column(col, order, half, guard, pad, ratio, T, exact=False, bug=None, after=None):
    """One channel -> Result.  after: what lies in memory behind col; only bug="fit_unclipped_n" looks at it (zeros when not given)."""
    col = np.asarray(col)
    n, p, h, g = col.size, int(order), int(half), int(guard)
    F, finite = _num(exact)
    fin = np.isfinite(col) if col.dtype == np.float32 else np.ones(n, bool)
    xv = np.where(fin, col, 0).astype(f64)
    tail = np.zeros(BLOCK + WING, f64)
    if after is not None:
        av = np.asarray(after).reshape(-1)[:tail.size]
        tail[:av.size] = np.where(np.isfinite(av.astype(f64)), av, 0).astype(f64)
    ext = np.concatenate([xv, tail])
    nb = -(-n // BLOCK)
    models, ratios, badblk = [], [], []
    for b in range(nb):
        lo, hi = max(0, b * BLOCK - WING), min(n, (b + 1) * BLOCK + WING)
        badblk.append(not fin[lo:hi].all())
        if bug == "fit_block_only":
            lo, hi = b * BLOCK, min(n, (b + 1) * BLOCK)
        elif bug == "fit_unclipped_n":
            hi = (b + 1) * BLOCK + WING
        w = ext[lo:hi]
        if badblk[-1] or (not exact and bug != "model_fp32" and not w.any()):      # an all-zero window: r[0] == 0, the delta model
            a, rt = [F(1.0)] + [F(0.0)] * p, None
        elif False:
            a, rt = [F(1.0)] + [F(0.0)] * p, None
        elif bug == "model_fp32":
            a, rt = _levinson_fp32(w, p)
        elif exact:
            a, rt = levinson(_lags([F(float(v)) for v in w], p, F), p, w.size, F, finite, bug)
        else:
            a, rt = levinson(_lags_np(w, p), p, w.size, float, math.isfinite, bug)
        models.append(a)
        ratios.append(rt)
    bad = np.zeros(n, bool)
    for b in range(nb):
        if badblk[b]:
            bad[b * BLOCK:(b + 1) * BLOCK] = True
    model_of = lambda t: models[t // BLOCK - 1] if bug == "prev_model_first_p" and t >= BLOCK and t % BLOCK < p else models[t // BLOCK]
    e, A, e_exact = np.zeros(n, f64), np.zeros(n, f64), None
    if exact:
        xs = [F(float(v)) for v in xv]
        e_exact = [None] * n
        for t in range(p, n):
            if not bad[t]:
                a = model_of(t)
                acc = a[0] * xs[t]
                for j in range(1, p + 1):
                    acc = acc + a[j] * xs[t - j]
                e_exact[t] = acc
                e[t] = float(acc)
        sq = [v * v if v is not None else F(0.0) for v in e_exact]
    else:
        for b in range(nb):
            lo, hi = max(b * BLOCK, p), min(n, (b + 1) * BLOCK)
            if hi <= lo:
                continue
            for t0, t1, a in ([(lo, min(hi, b * BLOCK + p), models[b - 1]), (max(lo, b * BLOCK + p), hi, models[b])]
                              if bug == "prev_model_first_p" and b >= 1 else [(lo, hi, models[b])]):
                if t1 <= t0:
                    continue
                t = np.arange(t0, t1)
                acc = f64(a[0]) * xv[t]
                for j in range(1, p + 1):
                    acc = acc + f64(a[j]) * xv[t - j]
                e[t] = acc
        e[bad] = 0.0
        sq = e * e
    for b in range(nb):
        lo, hi = max(b * BLOCK, p), min(n, (b + 1) * BLOCK)
        if hi > lo:
            t = np.arange(lo, hi)
            A[t] = sum(abs(float(models[b][j])) * np.abs(xv[t - j]) for j in range(p + 1))
    # ---- the windows
    gw = 0 if bug == "guard_included" else g
    t = np.arange(n)
    la, rz = np.maximum(t - h, p), np.minimum(t + h, n - 1)
    cl, cr = np.maximum(t - gw - la, 0), np.maximum(rz - t - gw, 0)
    cnt = np.full(n, 2 * (h - gw)) if bug == "cnt_untruncated" else cl + cr
    bc = np.concatenate([np.zeros(1, np.int64), np.cumsum(bad & (t >= p))])
    span = lambda a, b: np.where(b >= a, bc[np.clip(np.maximum(b, a - 1) + 1, 0, n)] - bc[np.clip(a, 0, n)], 0)
    nbad = bad.astype(np.int64) + span(la, t - gw - 1) + span(np.minimum(t + gw + 1, n), rz)
    ok = (t >= p) & (cnt >= h - g) & (nbad == 0)
    SL, SR = _windows(sq, n, h, gw, exact, bug)
    T2 = f64(f32(T)) * f64(f32(T))
    R2 = f64(f32(ratio)) * f64(f32(ratio))
    hot, margin = np.zeros(n, bool), math.inf
    ge = bug == "greater_equal"
    if exact:
        for k in np.flatnonzero(ok):
            s, c = sq[k], F(int(cnt[k]))
            lhs, rhs = s * c, F(float(R2)) * (SL[k] + SR[k])
            over_T = True if bug == "no_T" else (s >= F(float(T2)) if ge else s > F(float(T2)))
            hot[k] = over_T and (lhs >= rhs if ge else lhs > rhs)
            for u, v in ((s, F(float(T2))), (lhs, rhs)):
                if not (u == 0 and v == 0):
                    margin = min(margin, float(abs(u - v) / max(u, v)))
    else:
        S = SL + SR
        with np.errstate(over="ignore", invalid="ignore"):
            lhs, rhs = sq * cnt.astype(f64), R2 * S
            over_T = np.ones(n, bool) if bug == "no_T" else (sq >= T2 if ge else sq > T2)
            hot = ok & over_T & (lhs >= rhs if ge else lhs > rhs)
            for u, v in ((sq, np.full(n, T2)), (lhs, rhs)):
                m = ok & ~((u == 0) & (v == 0))
                if m.any():
                    margin = min(margin, float(np.min(np.abs(u[m] - v[m]) / np.maximum(u[m], v[m]))))
    dead = np.zeros(n, bool)
    for k in np.flatnonzero(hot):
        dead[(k if bug == "dilate_one_sided" else max(k - pad, 0)):min(k + pad, n - 1) + 1] = True
    out_e = e.copy()
    out_e[bad & (t >= p)] = np.nan
    return Result(out_e, hot, dead, A, ratios, margin, e_exact)


def _column_of(x, channel, bug):
    x = np.asarray(x)
    if x.ndim == 1:
        return x
    return x[:, (channel + 1) % x.shape[1]] if bug == "adjacent_channel" else x[:, channel]


def impulse_mask(x, order=16, half=256, guard=4, pad=2, ratio=10.0, thr=0.0, rel=0.0, channel=None, exact=False, bug=None, after=None,
                 results=None):
    """dead(j) for a file: (mask, T).  results, when a list, receives each column's Result."""
    x = np.asarray(x)
    T = R.threshold_ref(x, thr, rel, channel)
    cols = [_column_of(x, c, bug) for c in range(x.shape[1])] if x.ndim == 2 and (channel is None or channel < 0) else [_column_of(x, channel, bug)]
    mask = np.ones(x.shape[0], bool)
    for c in cols:
        res = column(c, order, half, guard, pad, ratio, T, exact, bug, after)
        mask &= res.dead
        if results is not None:
            results.append(res)
    return mask, T


def impulse_runs_ref(x, order=16, half=256, guard=4, pad=2, ratio=10.0, thr=0.0, rel=0.0, min_len=1, channel=None, exact=False, bug=None,
                     after=None, results=None):
    """-> (rows int32 (R, 2), T fp32)."""
    mask, T = impulse_mask(x, order, half, guard, pad, ratio, thr, rel, channel, exact, bug, after, results)
    return R.runs_of(mask, min_len), T


def residual_ref(x, order=16, channel=None, exact=False, bug=None):
    """si_impulse_residual: the Result of one channel (its e is the call's output; half, guard, pad and T are not read by it)."""
    return column(_column_of(x, channel, bug), order, 8, 0, 0, 10.0, 0.0, exact, bug)


def score(x, order=16, half=254, guard=4):
    """|e| sqrt(cnt / S) per sample (0 where hot's other conditions fail or S is 0): what `ratio` is compared with."""
    res = column(x, order, half, guard, 0, 1.0, 0.0)
    n, p = np.asarray(x).size, order
    t = np.arange(n)
    la, rz = np.maximum(t - half, p), np.minimum(t + half, n - 1)
    cnt = np.maximum(t - guard - la, 0) + np.maximum(rz - t - guard, 0)
    e = np.nan_to_num(res.e)
    SL, SR = _windows(e * e, n, half, guard, False, None)
    S = SL + SR
    ok = (t >= p) & (cnt >= half - guard) & (S > 0)
    return np.where(ok, np.abs(e) * np.sqrt(cnt / np.where(S > 0, S, 1.0)), 0.0)


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    x: np.ndarray
    kw: dict                                          # order, half, guard, pad, ratio, thr, rel, channel, min_len
    after: np.ndarray = None                          # what the test plants behind the file (and, mirrored, in front of it)


def check(case, exact=False):
    """The builders' three conditions on a case -> (rows, T, results).  exact=True also holds the float64 decisions to mpmath's."""
    results = []
    kw = {k: v for k, v in case.kw.items() if k != "min_len"}
    rows, T = impulse_runs_ref(case.x, min_len=case.kw.get("min_len", 1), results=results, **kw)
    for res in results:
        assert all(rt is None or rt > 1e-6 for rt in res.ratios), (case.name, res.ratios)
        assert res.margin > MARGIN, (case.name, res.margin)
    if exact:
        ex = []
        impulse_mask(case.x, exact=True, results=ex, **kw)
        for a, b in zip(results, ex):
            assert np.array_equal(a.hot, b.hot), case.name
            assert b.margin > MARGIN, (case.name, b.margin)
    return rows, T, results


def signal(n, dtype, seed, kind="voiced"):
    """A seeded voiced-plus-noise or AR(2) signal of tests/mend_ref.py as a file of `dtype`, |x| <= 0.3 of full scale."""
    x64 = M.voiced(n, seed) if kind == "voiced" else M.ar2(n, seed)
    return M.as_type(x64, dtype)


def plant(x, at, amp=0.5, width=1, sign=1):
    """A click: `width` samples from `at` on set to +-amp of full scale, alternating (in range for every type).  In place; -> x."""
    dtype = x.dtype.type
    for k in range(width):
        if 0 <= at + k < x.shape[0]:
            v = sign * (-1) ** k * amp * FULL[dtype]
            x[at + k] = v if dtype is np.float32 else int(round(v * 0.999))
    return x


def base_kw(**kw):
    out = dict(order=16, half=254, guard=4, pad=2, ratio=10.0, thr=0.0, rel=0.0, channel=None, min_len=1)
    out.update(kw)
    return out


def zeros_click(n, t, dtype=np.float32, **kw):
    """An all-zero file with one non-zero sample at t."""
    x = np.zeros(n, dtype)
    plant(x, t)
    return Case(f"zeros_click(n={n}, t={t}, {np.dtype(dtype).name})", x, base_kw(**kw))


def cnt_cases(p=2, h=8, g=1):
    """cnt = h - g - 1 against h - g: a click in zeros at the file's last sample t, whose right window is empty and whose left one is
    [p, t - g - 1]: cnt = t - g - p, so t = h + p - 1 is not hot and t = h + p is."""
    return [zeros_click(t + 1, t, order=p, half=h, guard=g, pad=0) for t in (h + p - 1, h + p)]


def nan_cases():
    """A NaN at the last sample of block 1's fit window [256, 1280), and one past it."""
    out = []
    for at in (1279, 1280):
        x = signal(2048, np.float32, 3)
        x[at] = np.nan
        out.append(Case(f"nan at {at}", x, base_kw(half=64)))
    return out


def clicked(n, dtype, seed, at, kind="voiced", amp=0.5, width=1, ch=None, **kw):
    """A seeded signal with clicks at the positions `at` (those outside [0, n) are dropped)."""
    x = signal(n, dtype, seed, kind)
    for t in at:
        plant(x, t, amp, width)
    return Case(f"{kind}(n={n}, {np.dtype(dtype).name}, seed={seed}, at={list(at)}, {kw})", x, base_kw(**kw))


def loud_then_quiet():
    """A full-scale stretch in front of a quiet one with a click in it: a difference of running sums loses the quiet squares."""
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(-1, 1, 1024), 1e-9 * rng.standard_normal(3072)]).astype(np.float32)
    x[3000] = 1e-6
    return Case("loud_then_quiet", x, base_kw(half=64, order=8))


def stereo_case(dtype=np.float32):
    a, b = clicked(1500, dtype, 5, (700,), half=64), clicked(1500, dtype, 6, (900,), half=64)
    return Case("stereo", np.stack([a.x, b.x], axis=1), base_kw(half=64, channel=0))


def cpu_cases():
    """The small cases tests/test_impulse_ref.py walks, the exact (mpmath) evaluation included."""
    out = [Case("zeros", np.zeros(700, np.float32), base_kw(half=32)), zeros_click(700, 300, half=32), zeros_click(700, 1, half=32),
           zeros_click(700, 699, np.int16, half=32)]
    out += cnt_cases()
    out += [clicked(1300, np.float32, 1, (511, 800), half=64), clicked(1300, np.int16, 2, (512, 1000), "ar2", half=64, order=8),
            clicked(1100, S24, 3, (513,), half=40, guard=2, pad=1, order=2), clicked(900, np.float32, 4, (600,), width=3, half=100, ratio=6.0)]
    out += [Case("constant", np.full(1200, 0.25, np.float32), base_kw(half=64)), stereo_case(), loud_then_quiet()]
    tail = Case("loud after n", signal(900, np.float32, 8), base_kw(half=64), after=np.resize(np.array([1.0, -1.0], np.float32), 768))
    plant(tail.x, 850)
    out.append(tail)
    floor = clicked(1300, np.float32, 9, (640,), amp=0.4, half=64)
    floor.kw["thr"] = 0.9
    floor.name = "T above the click"
    out.append(floor)
    return out


# The worst |e64 - e_exact| / A(t) over cpu_cases() (tests/test_impulse_ref.py measures it and holds it under this), A(t) = sum |a_j| |x[t - j]|;
# the device gets 16 times that for its own order inside the 1024-term lag sums, capped at 2^-24 so that a model formed in fp32 fails.
C_MEASURED = 2.0 ** -46
C_DEVICE = min(16.0 * C_MEASURED, 2.0 ** -24)


def seg22():
    import os
    x = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lj001_resample.npz"))["seg22"].copy()
    assert x.dtype == np.int16 and x.shape == (39690,) and np.abs(x.astype(np.int32)).max() == 20176
    return x


def seg22_scaled():
    """The fixture scaled so that its peak is 32 767."""
    return np.rint(seg22().astype(f64) * (32767.0 / 20176.0)).astype(np.int16)


CLICK_EVERY, CLICKS = 997, 37


def seg22_clicked(amp, seed=0):
    """seg22 with 37 clicks of 1 to 3 samples planted, one every 997 samples from sample 997 on: each sample of a click has +-amp int16
    steps ADDED (a seeded sign per sample), clipped to the int16 range.  -> (x, [(start, len)])."""
    x = seg22().astype(np.int32)
    rng = np.random.default_rng(seed)
    clicks = []
    for k in range(CLICKS):
        s, m = CLICK_EVERY * (k + 1), int(rng.integers(1, 4))
        x[s:s + m] += rng.choice((-1, 1), m) * int(amp)
        clicks.append((s, m))
    return np.clip(x, -32768, 32767).astype(np.int16), clicks


def click_table(amp, half=256, pad=2, ratio=10.0, order=16, guard=4):
    """One row of DESIGN.md 4.33's planted-click table: (found, fully covered, false hot samples, longest run)."""
    x, clicks = seg22_clicked(amp)
    results = []
    rows, _ = impulse_runs_ref(x, order, half, guard, pad, ratio, results=results)
    hot = results[0].hot
    near = np.zeros(x.size, bool)
    found = covered = 0
    for s, m in clicks:
        near[s:s + m + 5] = True                                       # hot samples lie at offsets 0 .. 4 from a click's first sample
        found += bool(hot[s:s + m + 5].any())
        covered += any(r0 <= s and s + m <= r0 + rl for r0, rl in rows.tolist())
    return found, covered, int((hot & ~near).sum()), int(rows[:, 1].max()) if rows.size else 0
