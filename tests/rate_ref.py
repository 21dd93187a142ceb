"""The definition of DESIGN.md 4.16 in numpy float64: the generated sample at a FILE sample, the blend weights on the file axis and
the composed output -- the reference of si_patch_rate (pure numpy, no GPU).

File sample i sits at i * P / Q on the 22.05 kHz axis ((P, Q) = (22050, sr) / gcd).  n, r = divmod(i P, Q); frac = scale (r / Q);
the left wing weighs x[n - k] by win[off + k step] + eta dwin[off + k step] for k < min(n + 1, (nwin - off) / step), with
off, eta = split(frac num_table); the right wing does the same from scale - frac on x[n + 1 + k].  Weights and the sum are float64, in
that order (left ascending, then right ascending); the result is rounded once to fp32.  Taps before recording sample 0 or at / past
`lim22` read as zero; every other tap must lie in the row, which is CHECKED here (an IndexError), never assumed.
`mistake` seeds one wrong reading of the definition, for the tests that show each of them is caught.
"""
import math

import numpy as np

from speech_inpainting_amd import audio
from speech_inpainting_amd import gaps as G

MISTAKES = ("pq_swapped", "time_off_by_one", "wings_swapped", "eta_dropped")
_TABLES = {}


def tables(sr):
    """audio.design_kaiser_best(22050, sr, .): win, dwin, num_table, step, scale (time_reg is not used)."""
    if sr not in _TABLES:
        _TABLES[sr] = audio.design_kaiser_best(22050, int(sr), 1)
    return _TABLES[sr]


def reach(sr):
    f = tables(sr)
    return G.rate_reach(f["win"].size, f["step"])


def sample(row, row_start, i, sr, lim22, mistake=None):
    """-> (y float64 before the rounding to fp32, A = sum |c x|) at file sample i.  row: 22.05 kHz samples [row_start, row_start +
    len(row)) of the recording's generated audio."""
    f = tables(sr)
    win, dwin, nwin, ntab, step, scale = f["win"], f["dwin"], f["win"].size, f["num_table"], f["step"], f["scale"]
    P, Q = G.rate_ratio(sr)
    if mistake == "pq_swapped":
        P, Q = Q, P
    n, r = divmod(int(i) * P, Q)
    if mistake == "time_off_by_one":
        n += 1
    frac = scale * (r / Q)
    terms = []
    wings = ((frac, -1, n), (scale - frac, 1, n + 1))
    if mistake == "wings_swapped":
        wings = ((scale - frac, -1, n), (frac, 1, n + 1))
    for fr, sign, first in wings:
        idx = fr * ntab
        off = int(idx)
        eta = 0.0 if mistake == "eta_dropped" else idx - off
        taps = (nwin - off) // step
        if sign < 0:
            taps = min(n + 1, taps)
        if taps <= 0:
            continue
        k = np.arange(taps)
        j = first + sign * k
        c = win[off + k * step] + eta * dwin[off + k * step]
        live = (j >= 0) & (j < lim22)
        o = j - row_start
        if np.any(live & ((o < 0) | (o >= len(row)))):
            bad = j[live & ((o < 0) | (o >= len(row)))]
            raise IndexError(f"file sample {i}: tap at 22.05 kHz sample {int(bad[0])} is outside the row [{row_start}, {row_start + len(row)})")
        xv = np.where(live, np.asarray(row, dtype=np.float64)[np.clip(o, 0, len(row) - 1)], 0.0)
        terms.append(c * xv)
    if not terms:
        return 0.0, 0.0
    t = np.concatenate(terms)
    return float(np.cumsum(t)[-1]), float(np.abs(t).sum())         # cumsum: the sequential sum, in the definition's order


def weights(spans, fade_f, n_file):
    """spans = (start, len, window, lim_f) rows in file samples -> (w fp32 (n_file), owner int (n_file)): the maximum over the spans
    of rise / 1 / mirrored fall, 0 at and past the span's lim_f; owner = the FIRST span of that greatest weight, -1 where w = 0."""
    ramp = G.fade_ramp(fade_f)
    w = np.zeros(n_file, dtype=np.float32)
    owner = np.full(n_file, -1, dtype=np.int64)
    for k, (s, l, _, lim) in enumerate(spans):
        a, b = max(s - fade_f, 0), min(s + l + fade_f, lim, n_file)
        for m in range(a, b):
            d = m - s
            wk = ramp[d + fade_f] if d < 0 else np.float32(1.0) if d < l else ramp[fade_f - 1 - (d - l)]
            if wk > w[m]:
                w[m], owner[m] = wk, k
    return w, owner


def interpolate(sr, spans, windows, gen_rows, fade_f, n_file):
    """The part of the definition that does not depend on the file's samples: -> dict(w fp32, owner, y (float64, before the rounding
    to fp32), A = sum |c x|, ctx = the context of the owner's window), each (n_file); computed once and shared between sample types."""
    w, owner = weights(spans, fade_f, n_file)
    y, A, ctx = np.zeros(n_file), np.zeros(n_file), np.zeros(n_file, dtype=np.int64)
    for m in np.flatnonzero(owner >= 0):
        wi = spans[owner[m]][2]
        c, ws, wl, wlim = windows[wi]
        y[m], A[m] = sample(np.asarray(gen_rows[wi])[:wl], ws, m, sr, wlim)
        ctx[m] = c
    return {"w": w, "owner": owner, "y": y, "A": A, "ctx": ctx}


def blend(orig, it, gain):
    """orig: the file's samples, fp32 or int16; it: `interpolate`'s result; gain: per context fp32 or None.  g = fl32(gain y32); the
    output is g where w = 1, else fma(w, g, fl32((1 - w) orig)); int16 samples enter as (float)v / 32768.
    -> (out float64 (n_file): the fp32 result, orig where nothing is written; E (n_file) = 7 * 2^-24 * (|orig| + |gain| A); written)."""
    orig = np.asarray(orig)
    o32 = orig.astype(np.float32) / np.float32(32768.0) if orig.dtype == np.int16 else orig.astype(np.float32)
    w, wr = it["w"], it["owner"] >= 0
    g0 = np.ones(o32.size, dtype=np.float32) if gain is None else np.asarray(gain, dtype=np.float32)[it["ctx"]]
    g = (g0 * it["y"].astype(np.float32)).astype(np.float32)
    t = ((np.float32(1.0) - w) * o32).astype(np.float32)
    # fma: w g is exact in float64 (24 x 24 bits); its sum with t is rounded to 53 bits and then to 24, far inside E
    mixed = (w.astype(np.float64) * g.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    v = np.where(w == np.float32(1.0), g, mixed)
    out = np.where(wr, v, o32).astype(np.float64)
    E = np.where(wr, 7.0 * 2.0 ** -24 * (np.abs(o32.astype(np.float64)) + np.abs(g0.astype(np.float64)) * it["A"]), 0.0)
    return out, E, wr


def compose(orig, sr, spans, windows, gen_rows, gain, fade_f):
    """The whole definition: spans = (start, len, window, lim_f) (file samples); windows = (context, first 22.05 kHz sample, samples,
    lim22); gen_rows[w]: the row of window w (fp32).  -> `blend`'s triple."""
    return blend(orig, interpolate(sr, spans, windows, gen_rows, fade_f, np.asarray(orig).size), gain)


def pcm16(v):
    """si_pcm16's arithmetic on float64 values that are fp32 results: `* 32768`, truncated toward zero, clamped."""
    return np.clip(np.trunc(np.asarray(v, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)
