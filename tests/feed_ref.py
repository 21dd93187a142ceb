"""The definition of DESIGN.md 4.17 in numpy float64: sample j of a recording's 22.05 kHz axis, interpolated straight from the file's own
samples at the exact rational time j Q / P -- the reference of si_cut_rate (pure numpy, no GPU).

(P, Q) = (22050, sr) / gcd.  n, r = divmod(j Q, P); frac = scale (r / P); the left wing weighs x[n - k] by win[off + k step] +
eta dwin[off + k step] for k < min(n + 1, (nwin - off) / step), with off, eta = split(frac num_table); the right wing does the same from
scale - frac on x[n + 1 + k] for k < min(n_file - n - 1, (nwin - off') / step).  The tables are audio.design_kaiser_best(sr, 22050, .)
(win carries the ratio when down-sampling; time_reg is not read).  Weights and the sum are float64, in that order (left ascending, then
right ascending); the result is rounded once to fp32 by the caller.  An int16 sample enters as (float)v / 32768.
`mistake` seeds one wrong reading of the definition, for the tests that show each of them is caught.
"""
import numpy as np

from speech_inpainting_amd import audio
from speech_inpainting_amd import gaps as G

MISTAKES = ("pq_swapped", "right_limit_off_by_one", "ratio_scaling_missing", "time_fp32", "wings_other_order")
_TABLES = {}


def tables(sr):
    """audio.design_kaiser_best(sr, 22050, .): win, dwin, num_table, step, scale (time_reg is not used)."""
    if sr not in _TABLES:
        _TABLES[sr] = audio.design_kaiser_best(int(sr), 22050, 1)
    return _TABLES[sr]


def reach(sr):
    """H = ceil(nwin / step): taps per wing."""
    f = tables(sr)
    return -(-f["win"].size // f["step"])


def n22(n_file, sr):
    """The recording's samples on the 22.05 kHz axis: ceil(n_file P / Q)."""
    P, Q = G.rate_ratio(sr)
    return -(-int(n_file) * P // Q)


def as_f64(x):
    """The file's samples as the kernel reads them: fp32, or int16 as (float)v / 32768 (exact)."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return (x.astype(np.float32) / np.float32(32768.0)).astype(np.float64)
    return x.astype(np.float32).astype(np.float64)


def at_times(x, n, frac, sr, mistake=None, win=None):
    """The two wings at integer parts n (int64 array) and table fractions frac (float64 array, scale * (time - n)) over the file x
    (float64).  -> (y float64 before the rounding to fp32, A = sum |c x|, S = scale num_table sum max(|dwin[w]|, |dwin[w +- 1]|) |x|: the
    slope of y in the time, in file samples)."""
    f = tables(sr)
    if win is None:
        win, dwin = f["win"], f["dwin"]
    else:                                                              # a seeded mistake's table
        dwin = np.zeros_like(win)
        dwin[:-1] = np.diff(win)
    nwin, ntab, step, scale = win.size, f["num_table"], f["step"], f["scale"]
    ad = np.abs(dwin)
    slope = np.maximum(ad, np.maximum(np.concatenate([ad[:1], ad[:-1]]), np.concatenate([ad[1:], ad[-1:]])))
    n = np.asarray(n, dtype=np.int64)
    frac = np.asarray(frac, dtype=np.float64)
    n_file, H = x.size, -(-nwin // step)
    k = np.arange(H)[None, :]
    halves = []
    for fr, sign, first, room in ((frac, -1, n, n + 1), (scale - frac, 1, n + 1, n_file - n - 1)):
        if mistake == "right_limit_off_by_one" and sign > 0:
            room = room - 1
        idx = fr * ntab
        off = idx.astype(np.int64)
        eta = idx - off
        taps = np.minimum(room, (nwin - off) // step)
        w = off[:, None] + k * step
        live = k < taps[:, None]
        wc = np.clip(w, 0, nwin - 1)
        c = win[wc] + eta[:, None] * dwin[wc]
        xi = first[:, None] + sign * k
        if np.any(live & ((xi < 0) | (xi >= n_file))):
            raise IndexError("a tap the counts allow lies outside the file")
        xv = x[np.clip(xi, 0, n_file - 1)]
        halves.append((np.where(live, c * xv, 0.0), np.where(live, slope[wc] * np.abs(xv), 0.0)))
    if mistake == "wings_other_order":
        halves = halves[::-1]
    t = np.concatenate([h[0] for h in halves], axis=1)
    y = np.cumsum(t, axis=1)[:, -1]                                    # cumsum: the sequential sum, in the definition's order (+ 0.0 is exact)
    A = np.abs(t).sum(axis=1)
    S = scale * ntab * np.concatenate([h[1] for h in halves], axis=1).sum(axis=1)
    return y, A, S


def samples(x, j, sr, mistake=None):
    """-> (y, A, S) float64 arrays at the 22.05 kHz samples j (any integers in [0, n22)) of the file x (fp32 or int16) at `sr` Hz."""
    f = tables(sr)
    P, Q = G.rate_ratio(sr)
    if mistake == "pq_swapped":
        P, Q = Q, P
    j = np.asarray(j, dtype=np.int64).reshape(-1)
    xf = as_f64(x)
    win = None
    if mistake == "ratio_scaling_missing" and f["ratio"] < 1:
        win = f["win"] / f["ratio"]
    if mistake == "time_fp32":
        time = (j.astype(np.float32) * np.float32(Q) / np.float32(P)).astype(np.float32)
        n = time.astype(np.int64)
        frac = f["scale"] * (time.astype(np.float64) - n)
    else:
        t = j * Q
        n = t // P
        frac = f["scale"] * ((t - n * P) / P)                          # int64 / int64: true division of exact values
    if mistake is None and j.size and (j.min() < 0 or n.max() >= xf.size):
        raise IndexError(f"22.05 kHz sample {int(j.max())} sits at or past the file's {xf.size} samples")
    n = np.clip(n, 0, xf.size - 1)
    parts = [at_times(xf, n[a:a + 4096], frac[a:a + 4096], sr, mistake, win) for a in range(0, j.size, 4096)]      # (4096, 2 H) at a time
    if not parts:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def clips(x, sr, starts, L, mistake=None):
    """si_cut_rate's output in float64: -> (y, A, S), each (C, L): row c = 22.05 kHz samples [starts[c], starts[c] + L)."""
    starts = [int(s) for s in starts]
    j = np.concatenate([np.arange(s, s + int(L), dtype=np.int64) for s in starts]) if starts else np.zeros(0, dtype=np.int64)
    y, A, S = samples(x, j, sr, mistake)
    shape = (len(starts), int(L))
    return y.reshape(shape), A.reshape(shape), S.reshape(shape)


def kernel_bound(y, A, sr):
    """What an fp32 output may differ from y by: its own rounding and the fma chain against numpy's separate multiply and add."""
    return 2.0 ** -24 * np.abs(y) + (2 * reach(sr) + 2) * 2.0 ** -52 * A
