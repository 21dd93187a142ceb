"""The definition of DESIGN.md 4.26 in numpy float64: both clip sets of a pass cut straight from a file -- the reference of si_cut_pair
(pure numpy, no GPU).

A clip starts on the 20 ms frame grid: frame f is 22.05 kHz sample 441 f and 16 kHz sample 320 f.  The 22.05 kHz row is tests/feed_ref.py's
definition, word for word.  The 16 kHz row is the same definition towards 16 000 Hz: (P16, Q16) = (16000, sr) / gcd, sample j at file
position j Q16 / P16, n, r = divmod(j Q16, P16) in int64, frac = scale (r / P16), the two wings, tap counts and summation order of 4.17
on the tables audio.design_kaiser_best(sr, 16000, .) (time_reg is not read).  The recording has N16 = ceil(n_file P16 / Q16) samples at
16 kHz; an output with j >= N16 is +0.0.  A 16 kHz file's row is the file's own samples: no filter is applied.
`samples(x, j, sr, target)` is written for ANY target, so that target = 22050 can be held against feed_ref bit for bit.
`mistake` seeds one wrong reading of the definition, for the tests that show each of them is caught.
"""
import math

import numpy as np

from speech_inpainting_amd import audio
from speech_inpainting_amd import gaps as G
from tests import feed_ref as F

MISTAKES = ("filters_swapped", "start_441", "filter_at_16k", "past_end_not_zeroed", "ratio_scaling_missing", "right_limit_off_by_one")
_TABLES = {}


def tables(sr, target):
    """audio.design_kaiser_best(sr, target, .): win, dwin, num_table, step, scale (time_reg is not used)."""
    if (sr, target) not in _TABLES:
        _TABLES[sr, target] = audio.design_kaiser_best(int(sr), int(target), 1)
    return _TABLES[sr, target]


def ratio(sr, target):
    """(P, Q) = (target, sr) / gcd: sample j of the target axis sits at file position j Q / P."""
    if target == 22050:
        return G.rate_ratio(sr)
    assert target == 16000
    return G.rate_ratio16(sr)


def reach(sr, target):
    """H = ceil(nwin / step): taps per wing; 0 for a 16 kHz file's 16 kHz row, which has no filter."""
    if sr == target:
        return 0
    f = tables(sr, target)
    return -(-f["win"].size // f["step"])


def n_axis(n_file, sr, target):
    """The recording's samples on the target axis: ceil(n_file P / Q)."""
    P, Q = ratio(sr, target)
    return -(-int(n_file) * P // Q)


def lim16(n_file, sr):
    """Where a clip's 16 kHz row may end: ceil(N22 320 / 441), the engine's L16 rule; N16 or N16 + 1."""
    return -(-n_axis(n_file, sr, 22050) * 320 // 441)


def _wings(x, n, frac, f, mistake=None):
    """feed_ref.at_times on the tables f: -> (y, A, S)."""
    win, dwin = f["win"], f["dwin"]
    if mistake == "ratio_scaling_missing" and f["ratio"] < 1:
        win = win / f["ratio"]
        dwin = np.zeros_like(win)
        dwin[:-1] = np.diff(win)
    nwin, ntab, step, scale = win.size, f["num_table"], f["step"], f["scale"]
    ad = np.abs(dwin)
    slope = np.maximum(ad, np.maximum(np.concatenate([ad[:1], ad[:-1]]), np.concatenate([ad[1:], ad[-1:]])))
    n_file, H = x.size, -(-nwin // step)
    k = np.arange(H)[None, :]
    terms, slopes = [], []
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
        terms.append(np.where(live, c * xv, 0.0))
        slopes.append(np.where(live, slope[wc] * np.abs(xv), 0.0))
    t = np.concatenate(terms, axis=1)
    y = np.cumsum(t, axis=1)[:, -1]                                    # the sequential sum, in the definition's order (+ 0.0 is exact)
    return y, np.abs(t).sum(axis=1), scale * ntab * np.concatenate(slopes, axis=1).sum(axis=1)


def samples(x, j, sr, target, mistake=None, table_target=None):
    """-> (y, A, S) float64 at the samples j (integers in [0, n_axis)) of the file's `target` axis.  table_target: the tables of another
    target (the swapped-filters mistake)."""
    f = tables(sr, target if table_target is None else table_target)
    P, Q = ratio(sr, target)
    j = np.asarray(j, dtype=np.int64).reshape(-1)
    xf = F.as_f64(x)
    t = j * Q
    n = t // P
    frac = f["scale"] * ((t - n * P) / P)                              # int64 / int64: true division of exact values
    if mistake is None and j.size and (j.min() < 0 or n.max() >= xf.size):
        raise IndexError(f"{target} Hz sample {int(j.max())} sits at or past the file's {xf.size} samples")
    n = np.clip(n, 0, xf.size - 1)
    parts = [_wings(xf, n[a:a + 4096], frac[a:a + 4096], f, mistake) for a in range(0, j.size, 4096)]
    if not parts:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def samples16(x, j, sr, mistake=None):
    """The 16 kHz axis at ANY integers j >= 0: zero at and past N16, the file's own samples for a 16 kHz file.  -> (y, A, S)."""
    j = np.asarray(j, dtype=np.int64).reshape(-1)
    xf = F.as_f64(x)
    N16 = n_axis(xf.size, sr, 16000)
    y, A, S = np.zeros(j.size), np.zeros(j.size), np.zeros(j.size)
    live = j < N16
    if mistake == "past_end_not_zeroed":                              # every j is computed, its n clipped into the file
        live = np.ones(j.size, dtype=bool)
    if sr == 16000 and mistake != "filter_at_16k":
        y[live] = xf[np.minimum(j[live], xf.size - 1)]
        return y, A, S
    swap = 22050 if mistake == "filters_swapped" else None
    if live.any():
        y[live], A[live], S[live] = samples(x, j[live], sr, 16000, mistake, swap)
    return y, A, S


def clips(x, sr, frames, L22, L16, mistake=None):
    """si_cut_pair's output in float64 -> dict(y22, A22, y16, A16, S16), (C, L22) and (C, L16): row c = 22.05 kHz samples 441 frames[c] +
    [0, L22) and 16 kHz samples 320 frames[c] + [0, L16)."""
    frames = [int(f) for f in frames]
    C = len(frames)
    j22 = np.concatenate([441 * f + np.arange(int(L22), dtype=np.int64) for f in frames]) if C else np.zeros(0, dtype=np.int64)
    step16 = 441 if mistake == "start_441" else 320
    j16 = np.concatenate([step16 * f + np.arange(int(L16), dtype=np.int64) for f in frames]) if C else np.zeros(0, dtype=np.int64)
    if mistake == "filters_swapped":
        y22, A22, _ = samples(x, j22, sr, 22050, None, 16000 if sr != 16000 else None)
    else:
        y22, A22, _ = samples(x, j22, sr, 22050, mistake if mistake in ("ratio_scaling_missing", "right_limit_off_by_one") else None)
    y16, A16, S16 = samples16(x, j16, sr, mistake)
    s22, s16 = (C, int(L22)), (C, int(L16))
    return dict(y22=y22.reshape(s22), A22=A22.reshape(s22), y16=y16.reshape(s16), A16=A16.reshape(s16), S16=S16.reshape(s16))


def kernel_bound(y, A, sr, target=16000):
    """What an fp32 output may differ from y by: its own rounding and the fma chain against numpy's separate multiply and add --
    2^-24 |y| + (2 H + 2) 2^-52 A, feed_ref.kernel_bound with the target's taps per wing.  Zero where A is (a sample past the end, a
    16 kHz file's own sample: exact)."""
    return 2.0 ** -24 * np.abs(y) * (A > 0) + (2 * reach(sr, target) + 2) * 2.0 ** -52 * A


def lds_floats(sr, frames_per_tile):
    """The floats one workgroup stages: ceil(F sr / 50) + 2 + 2 max(H22, H16)."""
    return -(-frames_per_tile * sr // 50) + 2 + 2 * max(reach(sr, 22050), reach(sr, 16000))


assert math.gcd(22050, 16000) == 50                                    # the 20 ms frame grid is the only one the two rates share
