"""The far end of the longest files the file kernels accept: the geometry table, the planted tails, the shift law and
the host model of a wrapped offset, for tests/test_far_host.py and tests/test_gpu_far.py.  A plain module, imported by name; importing
it needs no GPU, and nothing here is larger than a tail.

A FAR file is a body of one repeated value (`fill`) with a tail of K sample times behind it; the SHORT file is `lead` >= Z sample times
of the same fill in front of the same tail.  Every file kernel is local but for the global peak, which sits in the tail, so what a call
gives on the far file is what it gives on the short file moved by shift = n - (lead + K): `lift` for run tables, plain addition for
clip starts, spans and mend rows.  Only the short file ever goes through a float64 reference.

The mistakes a far test has to catch are modelled here on a VIRTUAL far file (fill below the tail, the tail above it, fill outside):
`seen` gives the short file as a reader sees it whose offset wrapped to int32, to uint32, or whose packed 24-bit byte offset 3 e wrapped
to uint32; `footprint` gives the elements a writer with that offset touches."""
from dataclasses import dataclass

import numpy as np

from speech_inpainting_amd import gaps as G

f32 = np.float32
S24 = np.int32                                     # the dtype that stands for packed 24-bit values, as in tests/mend_ref.py
K = 16384                                          # sample times of the tail
Z = 8192                                           # the short file's lead of fill, at least; the largest reach used is checked against it
CHUNK = 2048                                       # DT_CHUNK of detect_kernels.hip
MAX_REC = 2 ** 31 - 1 - 2048                       # SI_MAX_REC of api.hip
MAX_HALF = G.LEVEL_MAX_HALF
AMP = {np.float32: 1 << 16, np.int16: 1 << 15, S24: 1 << 23}      # full scale in grid steps; the fp32 grid is 2^-16 (tests/burst_ref.py's)
BYTES = {np.float32: 4, np.int16: 2, S24: 3}
WRAPS = ("int32", "uint32", "bytes24")
LONG_RUN = (K - 9000, K - 6000)                    # "dead" tails: zeros in every channel, longer than the largest window


# ------------------------------------------------------------------------------------------------------------ geometries
@dataclass(frozen=True)
class Geometry:
    name: str
    dtype: type
    ch: int
    n: int
    sr: int = 48000                                # the file rate the cutters are run at

    @property
    def elements(self):
        return self.n * self.ch

    @property
    def bytes(self):
        return self.elements * BYTES[self.dtype]

    def crosses(self, wrap):
        """Does the LAST element's offset wrap under `wrap`?"""
        last = self.elements - 1
        if wrap == "int32":
            return last >= 2 ** 31
        if wrap == "uint32":
            return last >= 2 ** 32
        return self.dtype is S24 and 3 * last >= 2 ** 32


def _low_n(sr=16000):
    P, Q = G.rate_ratio(sr)
    return MAX_REC * Q // P                        # the largest n with ceil(n P / Q) <= MAX_REC


GEOMETRIES = {g.name: g for g in (
    Geometry("E31", np.int16, 8, 2 ** 28 + 5),
    Geometry("E32", np.int16, 8, 2 ** 29 + 5),
    Geometry("CAP", np.int16, 1, MAX_REC),
    Geometry("S24", S24, 2, 2 ** 30 + 3),
    Geometry("F32", np.float32, 2, 2 ** 30 + 3),
    Geometry("LOW", np.int16, 1, _low_n(), 16000),
    Geometry("R22", np.float32, 1, MAX_REC, 22050),
    Geometry("M24", S24, 1, 2 ** 30 + 3),          # the mono files of mend_runs' other two sample types
    Geometry("M32", np.float32, 1, 2 ** 30 + 3),
    Geometry("W32", np.int16, 8, 2 ** 29 + 64),    # mend_runs' stores past element offset 2^32: a mended run ends >= 8 sample times before n
)}


def check_geometries():
    """What each geometry crosses, as DESIGN.md 4.32 lists it."""
    g = GEOMETRIES
    assert (g["E31"].n - 5) * 8 == 2 ** 31 and g["E31"].crosses("int32") and not g["E31"].crosses("uint32")
    assert (g["E32"].n - 5) * 8 == 2 ** 32 and g["E32"].crosses("uint32") and g["E32"].bytes < 9 * 10 ** 9
    cap = g["CAP"]
    assert cap.n == MAX_REC and cap.n % CHUNK == CHUNK - 1 and -(-cap.n // CHUNK) == 2 ** 20 - 1 and not cap.crosses("int32")
    assert cap.n + CHUNK == 2 ** 31 - 1 and 4.2e9 < cap.bytes < 4.3e9      # one chunk of headroom, to the last value of an int32
    for name in ("S24", "F32"):
        assert (g[name].n - 3) * 2 == 2 ** 31 and g[name].crosses("int32") and not g[name].crosses("uint32")
    assert g["S24"].crosses("bytes24") and 3 * (g["S24"].n - K) * 2 >= 2 ** 32 and 6.4e9 < g["S24"].bytes < 6.5e9
    assert 8.5e9 < g["F32"].bytes < 8.6e9 and 8.5e9 < g["E32"].bytes < 8.6e9 and 4.2e9 < g["E31"].bytes < 4.3e9
    low = g["LOW"]
    P, Q = G.rate_ratio(low.sr)
    assert (P, Q) == (441, 320) and -(-low.n * P // Q) <= MAX_REC < -(-(low.n + 1) * P // Q) and low.n < MAX_REC and 3.1e9 < low.bytes < 3.2e9
    assert g["R22"].n == MAX_REC and 8.5e9 < g["R22"].bytes < 8.6e9
    for mono, two in (("M24", "S24"), ("M32", "F32")):                # the table's bytes for ch = 1
        assert g[mono].n >= 2 ** 30 + 3 and g[mono].ch == 1 and g[mono].bytes * 2 == g[two].bytes
    assert (g["W32"].n - 64) * 8 == 2 ** 32 and (g["W32"].n - MEND["context"] - 4) * 8 > 2 ** 32 and g["W32"].bytes < 9 * 10 ** 9
    assert all(x.n <= MAX_REC and 1 <= x.ch <= 8 and x.bytes <= 9 * 10 ** 9 for x in g.values())
    return True


# ------------------------------------------------------------------------------------------------------------ short files and shifts
def lead_of(n, unit=1):
    """The short file's lead for a far file of n sample times: Z, and as many more as make the shift a whole number of `unit`."""
    lead = Z + (n - Z - K) % unit
    assert (n - lead - K) % unit == 0 and lead >= Z
    return lead


def shift_of(n, unit=1):
    return n - lead_of(n, unit) - K


def short_file(tail, fill, lead=Z):
    """lead sample times of fill in front of the tail: (lead + K,) or (lead + K, ch), the tail's dtype."""
    body = np.full((lead,) + tail.shape[1:], fill, dtype=tail.dtype)
    return np.ascontiguousarray(np.concatenate([body, tail]))


def lift(rows, shift, fill_is_dead):
    """The short file's run table -> the far file's.  A row that starts at 0 is the body's run when the fill is dead: it stays at 0 and
    gains the shift in length; every other row moves by the shift.  A dead fill makes exactly such a first row; a live one makes none."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2).copy()
    body = len(rows) > 0 and rows[0, 0] == 0
    assert bool(body) == bool(fill_is_dead), (rows[:2].tolist(), fill_is_dead)
    assert np.all(rows[int(body):, 0] > 0)
    rows[int(body):, 0] += shift
    if body:
        assert rows[0, 1] >= Z
        rows[0, 1] += shift
    assert rows.size == 0 or (rows[:, 0] + rows[:, 1]).max() < 2 ** 31
    return rows.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ the tail
def grid(v, dtype):
    """Integers in grid steps -> samples of `dtype` (fp32: times 2^-16, exact)."""
    v = np.asarray(v)
    return (v.astype(np.float64) * 2.0 ** -16).astype(f32) if dtype is np.float32 else v.astype(dtype)


def fills(dtype):
    """(the zero body, the constant body): the constant is 1 / 16 of full scale, an eighth of the tail's peak."""
    return grid(0, dtype)[()], grid(AMP[dtype] // 16, dtype)[()]


def peak_of(dtype):
    return grid(AMP[dtype] // 2, dtype)[()]


def last_seam(n):
    """The tail position of the first sample time of the far file's last chunk."""
    b = (n - 1) // CHUNK * CHUNK - (n - K)
    assert 0 < b < K
    return b


def tail(geom, kind, seed=0):
    """The K sample times behind the body of geometry `geom`, as (K,) or (K, ch) host samples.  kind: what the planted damage is --
    "dead" (zeros and held values: quiet, dead and level detection), "burst" (alternating half scale), "invalid" (NaN, inf and
    over-ceiling values; see `ceiling`), "mend" (none: the bare noise; mend_runs itself takes `smooth_tail`).

    Base: per channel independent noise of 1/8 .. 1/4 of full scale, never zero, no two neighbours equal; each channel's peak, half of
    full scale exactly, planted once.  Damage, c = the last channel (every channel of a mono file):
        [K - 100, K - 90) in c alone            [K - 50, K - 45) in every channel (joint)
        [K - 7, K - 4)    in every channel      [K - 2, K) in c and [K - 4, K) in every other channel: a run of c and a joint run end with the file
        "dead": zeros in every channel over LONG_RUN, longer than the largest window; tail[b - 1] == tail[b], b = the far file's
        last chunk seam (a held link across it in c and jointly: a loud pair, or at K - 5 the zeros above; at K - 3 a loud pair in c
        and the other channels' zeros); a held run of 20 in c.  "burst": [K - 700, K - 600) in every channel
    so the last five sample times (E31, E32) and the last three (S24, F32) each hold damage and intact samples in c, and a joint run."""
    dtype, ch, A = geom.dtype, geom.ch, AMP[geom.dtype]
    rng = np.random.default_rng(1000 * seed + 7 * ch + BYTES[dtype])
    v = rng.integers(A // 8, A // 4, (K, ch)) * rng.choice([-1, 1], (K, ch))
    for c in range(ch):                                               # no accidental links: equal neighbours get another magnitude
        same = np.flatnonzero(v[1:, c] == v[:-1, c]) + 1
        v[same, c] += 1
    for c in range(ch):
        v[K - 3000 - 16 * c, c] = A // 2 * (-1 if c % 2 else 1)       # the channel's peak
    c, b = ch - 1, last_seam(geom.n)
    spots = [(K - 100, K - 90, [c]), (K - 50, K - 45, range(ch)), (K - 7, K - 4, range(ch)), (K - 2, K, [c]), (K - 4, K, range(ch - 1))]
    if kind == "dead":
        if b < K - 8:
            v[b - 1:b + 1, :] = A // 5                                # a link across the last chunk seam, loud
        elif b == K - 3:                                              # S24, F32: the seam lies among the last three.  The other channels'
            v[K - 4, c] = v[K - 3, c]                                 # zeros link across it; c gets a loud pair, K - 3 staying intact
        else:                                                         # E31, E32: the zeros of [K - 7, K - 4) link across it in every channel
            assert b == K - 5
        v[K - 300:K - 280, c] = -(A // 5)                             # a held run
        for a, z, cols in spots + [LONG_RUN + (range(ch),)]:
            for k in cols:
                v[a:z, k] = 0
    elif kind == "burst":
        for a, z, cols in spots + [(K - 700, K - 600, range(ch))]:
            for k in cols:
                v[a:z, k] = np.where(np.arange(a, z) % 2 == 0, A // 2, -(A // 2))
    elif kind == "invalid":
        for a, z, cols in spots:
            for k in cols:
                v[a:z, k] = (A * 15) // 16                            # above `ceiling`, below full scale
    else:
        assert kind == "mend"
    x = grid(v, dtype)
    if kind == "invalid" and dtype is np.float32:                     # NaN and inf among the over-ceiling values
        x[K - 100, c], x[K - 49, :], x[K - 5, :], x[K - 2:, :] = np.nan, np.inf, np.nan, -np.inf
    return np.ascontiguousarray(x[:, 0] if ch == 1 else x)


def ceiling(dtype):
    """The ceiling of the "invalid" tails: 7 / 8 of full scale, in the file's own units -- above the peak and the fills."""
    return float(grid(AMP[dtype] * 7 // 8, dtype))


def image(x):
    """A packed 24-bit file's fp32 image F = V 2^-23 (tests/s24_ref.py): what the fp32 references of quiet, dead and level read."""
    return np.asarray(x).astype(f32) * f32(2.0 ** -23)


def smooth_tail(geom, seed=0):
    """A tail for mend_runs: per channel a voiced signal at 0.3 of full scale (tests/mend_ref.py's), in the geometry's type."""
    from tests import mend_ref as M
    cols = [M.as_type(M.voiced(K, 50 + seed + 3 * c), geom.dtype) for c in range(geom.ch)]
    return cols[0] if geom.ch == 1 else np.ascontiguousarray(np.stack(cols, axis=1))


# ------------------------------------------------------------------------------------------------------------ the wrapped offsets
def _wrap(e, wrap):
    e = np.asarray(e, dtype=np.int64)
    if wrap == "int32":
        return (e + 2 ** 31) % 2 ** 32 - 2 ** 31
    assert wrap == "uint32"
    return e % 2 ** 32


def seen(geom, tail_, fill, wrap, lead=Z):
    """The short file (lead + K sample times) as a reader finds it in the virtual far file when its element offset t ch + c wraps to
    int32 or uint32, or ("bytes24") when the byte offset 3 e of a packed 24-bit sample wraps to uint32 and the three bytes are taken from
    there.  The virtual file is the tail at its true offsets and fill everywhere else, in front of the file included."""
    n, ch = geom.n, geom.ch
    flat = np.asarray(tail_).reshape(-1)
    t = np.arange(n - lead - K, n, dtype=np.int64)
    e = (t[:, None] * ch + np.arange(ch)[None, :]).reshape(-1)
    first = (n - K) * ch
    if wrap == "bytes24":
        assert geom.dtype is S24
        fb = np.array([(int(fill) >> s) & 0xFF for s in (0, 8, 16)], dtype=np.int64)
        tb = np.stack([(flat.astype(np.int64) >> s) & 0xFF for s in (0, 8, 16)], axis=1).reshape(-1)
        b = ((3 * e) % 2 ** 32)[:, None] + np.arange(3)[None, :]       # the three bytes from the wrapped base
        inside = (b >= 3 * first) & (b < 3 * n * ch)
        byte = np.where(inside, tb[np.clip(b - 3 * first, 0, tb.size - 1)], fb[b % 3])
        u = byte[:, 0] | byte[:, 1] << 8 | byte[:, 2] << 16
        out = (u - np.where(u & 0x800000, 1 << 24, 0)).astype(S24)
    else:
        w = _wrap(e, wrap)
        inside = (w >= first) & (w < n * ch)
        out = np.where(inside, flat[np.clip(w - first, 0, flat.size - 1)], fill).astype(flat.dtype)
    out = out.reshape(lead + K, ch)
    return np.ascontiguousarray(out[:, 0] if np.asarray(tail_).ndim == 1 else out)


def footprint(geom, times, channel, wrap):
    """The element (or, "bytes24", first-byte) offsets a writer touches for the sample `times` of `channel` when its offset wraps."""
    e = np.asarray(times, dtype=np.int64) * geom.ch + channel
    return (3 * e) % 2 ** 32 if wrap == "bytes24" else _wrap(e, wrap)


def true_footprint(geom, times, channel, wrap):
    e = np.asarray(times, dtype=np.int64) * geom.ch + channel
    return 3 * e if wrap == "bytes24" else e


# ------------------------------------------------------------------------------------------------------------ detector cases
DETECTORS = ("quiet", "dead", "level", "burst", "invalid")
TAIL_KIND = {"quiet": "dead", "dead": "dead", "level": "dead", "burst": "burst", "invalid": "invalid"}


def unit(dtype):
    """One grid step in the file's own units: what thresholds are given in."""
    return 2.0 ** -16 if dtype is np.float32 else 1.0


def detector_tail(geom, det, seed=0):
    return tail(geom, TAIL_KIND[det], seed)


def detector_params(det, dtype):
    """The parameter sets each detector runs with, thresholds in the file's own units.  Absolute thresholds sit between the zeros and
    the constant fill (1 / 16 of full scale); at least one set per detector is relative, so that the peak pass runs; level and burst
    take half = 0, 1 and the largest."""
    A, u = AMP[dtype], unit(dtype)
    if det == "quiet":
        return [dict(thr=A // 256 * u)]
    if det == "dead":
        return [dict(kind="any", rel=1.0 / 64), dict(kind="quiet", thr=A // 256 * u), dict(kind="held")]
    if det == "level":
        return [dict(half=0, thr=A // 64 * u), dict(half=1, rel=1.0 / 64), dict(half=MAX_HALF, thr=A // 64 * u)]
    if det == "burst":
        return [dict(half=0, thr=float(f32(1.15 * A * u))), dict(half=1, rel=2.3), dict(half=MAX_HALF, thr=float(f32(0.55 * A * u)))]
    return [dict(ceiling=ceiling(dtype))] + ([dict(ceiling=float("inf"))] if dtype is np.float32 else [])


def fill_is_dead(det, p, fill):
    """Is a body of `fill` one dead run under detector `det` with parameters p?  Zero: quiet, dead (either kind) and low.  The
    constant: held only -- it is above every threshold, its second difference is zero, and it is valid."""
    if det in ("burst", "invalid"):
        return False
    if float(fill) == 0.0:
        return True
    return det == "dead" and p["kind"] in ("any", "held")


def reference_rows(det, p, x, channel):
    """The float64 / exact references of tests/*_ref.py on the host file x ((n,) with channel None, (n, ch) with channel = c or -1).
    A packed 24-bit file goes through its fp32 image with thresholds times 2^-23 (tests/s24_ref.py) where the reference has no 24-bit
    type of its own."""
    from tests import burst_ref as B
    from tests import channels_ref as CH
    from tests import dead_ref as R
    from tests import detect_ref as D
    from tests import invalid_ref as IV
    from tests import level_ref as L
    s24 = x.dtype.type is S24
    if det == "burst":
        return B.burst_runs_ref(x, p["half"], p.get("thr", 0.0), p.get("rel", 0.0), 1, channel)
    if det == "invalid":
        return IV.invalid_runs_ref(x, p["ceiling"], 1, channel)
    F, s = (image(x), 2.0 ** -23) if s24 else (x, 1.0)
    thr = float(f32(p.get("thr", 0.0)) * f32(s))
    if det == "quiet":
        if channel is None:
            return D.quiet_runs_ref(F, thr, 1)
        return CH.joint_runs_ref(F, thr, 1) if channel < 0 else D.quiet_runs_ref(F[:, channel], thr, 1)
    if det == "dead":
        return R.dead_runs_ref(F, {"quiet": R.QUIET, "held": R.HELD, "any": R.ANY}[p["kind"]], thr, p.get("rel", 0.0), 0.0, 1, channel)
    return L.level_runs_ref(F, p["half"], thr, p.get("rel", 0.0), 1, channel)


def undecided(det, p, x, channel):
    """level and burst: the samples whose verdict could depend on the order of the device's additions (Case.undecided of the references)."""
    from tests import burst_ref as B
    from tests import level_ref as L
    if det == "burst":
        return B.Case("far", x, p["half"], p.get("thr", 0.0), p.get("rel", 0.0), 1, channel).undecided()
    assert det == "level"
    F, s = (image(x), 2.0 ** -23) if x.dtype.type is S24 else (x, 1.0)
    return L.Case("far", F, p["half"], float(f32(p.get("thr", 0.0)) * f32(s)), p.get("rel", 0.0), 1, channel).undecided()


def channels_of(geom):
    """The channel arguments a detector runs with: mono, or the last channel and joint."""
    return [None] if geom.ch == 1 else [geom.ch - 1, -1]


DETECTOR_GEOMETRIES = ("CAP", "E31", "E32", "S24", "F32")
REACH = {"detect": 2 * MAX_HALF + 1, "mend": 1024, "cut": 400}     # sample times a call reaches; every one is checked against Z


# ------------------------------------------------------------------------------------------------------------ mend cases
MEND = dict(order=8, context=32, max_len=64)
MEND_GEOMETRIES = ("CAP", "M24", "M32", "E31", "E32", "W32", "S24", "F32")


def mend_case(geom, edge, seed=0):
    """(tail, rows in TAIL positions) for si_mend_runs: a smooth tail whose damaged samples hold full scale (PCM) or NaN (fp32).  Rows: one
    whose context reaches 16 sample times into the body, lengths 5, 16 and 64 inside, and the last one, of 4 samples, whose e + context
    is n exactly (edge = False: it is mended) or n + 1 (edge = True: SI_MEND_EDGE, and the file keeps its bits there)."""
    from tests import mend_ref as M
    x = smooth_tail(geom, seed)
    Kc = MEND["context"]
    rows = [(16, 4), (K - 8000, 5), (K - 4000, 16), (K - 1000, 64), (K - Kc - 4 + int(edge), 4)]
    col = x if x.ndim == 1 else x[:, geom.ch - 1]
    for s, m in rows:
        col[s:s + m] = np.nan if geom.dtype is np.float32 else M.RANGE[geom.dtype][1]
    assert rows[-1][0] + rows[-1][1] + Kc == K + int(edge)
    return x, rows


def mend_channel(geom):
    return None if geom.ch == 1 else geom.ch - 1


# ------------------------------------------------------------------------------------------------------------ cutter cases
CUT_GEOMETRIES = ("CAP", "LOW", "E31", "S24")
TILE = 512                                         # CUT_RATE_TILE


def cut_rates(geom):
    """48 kHz and one more rate the geometry allows; LOW is a 16 kHz file by definition (at 48 kHz its 22.05 kHz axis is far from the
    cap), with 11.025 kHz beside it only where n allows -- it does not, so LOW runs at its own rate alone."""
    return [16000] if geom.name == "LOW" else [48000, 44100]


def cut_plan(geom, sr, L=TILE + 1):
    """Clip starts on the far file's 22.05 kHz axis, the same on the short file's, and both files' geometry.  One clip ends with the
    axis' last sample (it reads the zero extension past n_file), one straddles that clip's last tile seam, one lies a tile further in."""
    P, Q = G.rate_ratio(sr)
    n = geom.n
    lead = lead_of(n, Q)
    k = lead + K
    shift, shift22 = n - k, (n - k) // Q * P
    N22, N22s = -(-n * P // Q), -(-k * P // Q)
    assert (n - k) % Q == 0 and N22 == N22s + shift22
    starts = [N22 - L, N22 - L - (TILE // 2), N22 - L - 2 * TILE - 77]
    short = [s - shift22 for s in starts]
    assert min(short) * Q // P - REACH["cut"] >= 0, "a clip's taps reach in front of the short file"
    return dict(P=P, Q=Q, lead=lead, k=k, shift=shift, shift22=shift22, N22=N22, N22s=N22s, starts=starts, short=short, L=L)


def pair_plan(geom, sr):
    """cut_plan for si_cut_pair: frames of 20 ms.  The first clip ends with both axes (L22 and L16 reach N22 and ceil(N22 320 / 441)),
    the second a frame earlier, the third seven; the shift is a whole number of frames."""
    P, Q = G.rate_ratio(sr)
    per = sr // 50
    assert sr % 50 == 0 and per % Q == 0
    n = geom.n
    lead = lead_of(n, per)
    k = lead + K
    shift = n - k
    shift_f = shift // per
    N22, N22s = -(-n * P // Q), -(-k * P // Q)
    lim, lims = -(-N22 * 320 // 441), -(-N22s * 320 // 441)
    assert shift % per == 0 and N22 == N22s + 441 * shift_f and lim == lims + 320 * shift_f
    f0 = N22 // 441 - 3
    L22, L16 = N22 - 441 * f0, lim - 320 * f0
    frames = [f0, f0 - 1, f0 - 7]
    short = [f - shift_f for f in frames]
    assert min(short) * per - REACH["cut"] >= 0 and 3 * 441 <= L22 < 4 * 441
    return dict(P=P, Q=Q, lead=lead, k=k, shift=shift, shift_f=shift_f, N22=N22, N22s=N22s, lim=lim, lims=lims, frames=frames, short=short, L22=L22, L16=L16)


def column(x, channel):
    """The channel a call with `channel` reads, as the mono file the references take; a packed 24-bit file as its fp32 image (the cutters'
    contract in tests/s24_ref.py)."""
    col = x if x.ndim == 1 else x[:, channel]
    return image(col) if col.dtype.type is S24 else np.ascontiguousarray(col)


def patch_plan(geom, sr, fade_f, reach):
    """One span of 700 sample times that ends with the file, cross-faded in front, its window on the 22.05 kHz axis reaching the axis'
    end (tests/test_gpu_channels.py's): the far table's rows and the short table's."""
    P, Q = G.rate_ratio(sr)
    n = geom.n
    lead = lead_of(n, Q)
    k = lead + K
    shift, shift22 = n - k, (n - k) // Q * P
    N22, N22s = -(-n * P // Q), -(-k * P // Q)
    s, l = n - 700, 700
    ws = (s - fade_f) * P // Q - reach - 2
    wl = N22 - ws
    region = lambda a, lim: G.region_chunks(G.file_regions([(a, l)], [lim], fade_f))
    far_rows = dict(spans=[(s, l, 0, n)], windows=[(0, ws, wl, N22)], chunks=region(s, n))
    short_rows = dict(spans=[(s - shift, l, 0, k)], windows=[(0, ws - shift22, wl, N22s)], chunks=region(s - shift, k))
    assert N22 == N22s + shift22 and ws - shift22 > 0
    return dict(P=P, Q=Q, lead=lead, k=k, shift=shift, shift22=shift22, far=far_rows, short=short_rows, wl=wl, written=(s - fade_f, n))
