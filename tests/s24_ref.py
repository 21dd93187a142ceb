"""Packed 24-bit PCM: pack / unpack in numpy, the store rule, the case builders of tests/test_s24_host.py and
tests/test_gpu_s24.py, and test_gpu_rate.py's patch case restated.  A plain module, imported by name; importing it needs no GPU.

The contract needs no tolerance of its own.  A file V (int32 values in [-2^23, 2^23 - 1]) has the fp32 image F = V 2^-23, exact, and
multiplying by a power of two commutes with every rounding of the kernels, so
    detection   runs(V, thr, tol, rel, ...) are the existing references' rows on (F, thr 2^-23, tol 2^-23, rel, ...), and T_s24 = T_F 2^23
    cutters     the call on V gives the bytes the fp32 call gives on F
    patch       a written sample is store(the fp32 the fp32 call writes for F), store(w) = trunc(w 2^23) clamped, NaN -> 0
`expected` below is that statement.  The LIFTED cases are the int16 tables of detect_ref / dead_ref / level_ref with values, thresholds
and tolerances times 256: their rows are the int16 cases' own, which ties the two integer types together without passing through F.

unpack takes bug=<name>, one of MISTAKES, which seeds that mistake into the decoding: tests/test_s24_host.py shows that each one changes
the expected rows of at least one case, i.e. that the cases can tell."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from speech_inpainting_amd import gaps as G
from tests import dead_ref as R
from tests import detect_ref as D
from tests import level_ref as L
from tests import rate_ref as RR

f32 = np.float32
LO, HI = -(1 << 23), (1 << 23) - 1
SCALE = f32(2.0 ** -23)
MISTAKES = ("big_endian", "zero_extension", "sign_from_byte_0", "one_byte_shift")


# ------------------------------------------------------------------------------------------------------------ the sample type
def pack(v):
    """int values in [LO, HI], any shape -> uint8 (..., 3), little-endian."""
    v = np.asarray(v).astype(np.int64)
    assert v.size == 0 or (v.min() >= LO and v.max() <= HI)
    u = v & 0xFFFFFF
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def unpack(b, bug=None):
    """uint8 (..., 3) -> int32 (...).  bug: one of MISTAKES."""
    b = np.asarray(b)
    assert b.dtype == np.uint8 and b.shape[-1] == 3
    if bug == "one_byte_shift":                                        # bytes [3 i + 1, 3 i + 4) of the stream; the last one reads 0 behind it
        flat = np.concatenate([b.reshape(-1)[1:], np.zeros(1, np.uint8)])
        b = flat.reshape(b.shape)
    b0, b1, b2 = (b[..., k].astype(np.int64) for k in range(3))
    if bug == "big_endian":
        b0, b2 = b2, b0
    u = b0 | b1 << 8 | b2 << 16
    if bug == "zero_extension":
        return u.astype(np.int32)
    neg = (b0 if bug == "sign_from_byte_0" else b2) & 0x80
    return (u - np.where(neg != 0, 1 << 24, 0)).astype(np.int32)


def image(v):
    """F = V 2^-23 as fp32, exact."""
    return np.asarray(v).astype(f32) * SCALE


def store(w):
    """The store rule on fp32 values w: trunc(w * 8388608) in fp32 arithmetic, clamped to [LO, HI], NaN -> 0 -> int32."""
    w = np.asarray(w, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (w * f32(8388608.0)).astype(f32)
        p = np.where(np.isnan(p), f32(0), p)
        return np.clip(np.trunc(p.astype(np.float64)), LO, HI).astype(np.int32)


def store_f64(v):
    """The same on float64 values (a reference +- its bound): trunc(v 2^23), clamped."""
    return np.clip(np.trunc(np.asarray(v, dtype=np.float64) * 8388608.0), LO, HI).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ detection cases
@dataclass
class Case:
    """One detection call on a 24-bit file v (int32, (n,) or (n, ch)).  family: "quiet" (si_quiet_runs[_ch]), "dead" (si_dead_runs) or
    "level" (si_level_runs).  thr and tol in 24-bit steps.  rows: what a lifted case expects (the int16 case's rows), else None and
    `expected` is the only statement.  before / after: int32 sample times planted around the input, (k,) or (k, ch)."""
    family: str
    name: str
    v: np.ndarray
    thr: float = 0.0
    min_len: int = 1
    channel: Optional[int] = None
    kind: int = R.QUIET
    rel: float = 0.0
    tol: float = 0.0
    half: int = 0
    rows: Optional[np.ndarray] = None
    T: Optional[np.float32] = None
    before: Optional[np.ndarray] = None
    after: Optional[np.ndarray] = None


def expected(c, values=None):
    """(rows, T in 24-bit steps or None) of case c by the EXISTING fp32 references on the image F.  values: other int32 values in place
    of c.v (what a mistaken unpack decodes)."""
    F = image(c.v if values is None else values)
    thr, tol = f32(c.thr) * SCALE, f32(c.tol) * SCALE
    if c.family == "quiet":
        rows = D.quiet_runs_ref(F, thr, c.min_len) if F.ndim == 1 else R.dead_runs_ref(F, R.QUIET, thr, 0.0, 0.0, c.min_len, c.channel)
        return rows, None
    if c.family == "dead":
        T = R.threshold_ref(F, thr, c.rel, c.channel)
        return R.dead_runs_ref(F, c.kind, thr, c.rel, tol, c.min_len, c.channel), f32(T * f32(2.0 ** 23))
    case = L.Case(c.name, F, c.half, float(thr), c.rel, c.min_len, c.channel)
    if values is None:
        L.decided(case)
    return case.rows(), f32(case.threshold() * f32(2.0 ** 23))


def _lift(a):
    return None if a is None else np.asarray(a).astype(np.int32) * 256


def lifted_quiet_cases(sizes=D.SEAM_N):
    out = []
    for n in sizes:
        for name, q, min_len in D.seam_cases(n):
            x = D.materialize(q, np.int16, n)
            out.append(Case("quiet", f"lifted: {name}, n {n}", _lift(x), 256.0 * D.THR[np.int16], min_len,
                            rows=D.quiet_runs_ref(x, D.THR[np.int16], min_len)))
    return out


def _int16_dead_cases():
    out = [c for c in R.value_cases() if c.x.dtype == np.int16]
    for n in (1, 2, 9, 513, 2049, 4101):
        out += R.seam_cases(n, np.int16)
    out += R.peak_position_cases(np.int16)
    for ch in (2, 3):
        out += R.channel_cases(ch, np.int16)
    return out


def lifted_dead_cases():
    """dead_ref's int16 tables (all_cpu_cases' int16 half: value, seam, peak-position and channel cases), times 256."""
    return [Case("dead", "lifted: " + c.name, _lift(c.x), 256.0 * c.thr, c.min_len, c.channel, c.kind, c.rel, 256.0 * c.tol, rows=c.rows(),
                 T=f32(c.threshold() * f32(256)), before=_lift(c.before), after=_lift(c.after)) for c in _int16_dead_cases()]


def _int16_level_cases():
    out = []
    for h in (0, 1, 7, 48):
        out += L.value_cases(h, np.int16)
        for n in (1, 2, 2 * h + 1, 2049):
            out += L.size_cases(n, h, np.int16)
    out += L.half0_cases(np.int16)
    for ch in (2, 3):
        out += L.channel_cases(ch, np.int16)
    return out


def lifted_level_cases():
    """level_ref's int16 tables (all_cpu_cases' int16 half), times 256: squares up to 2^46, window sums multiples of 2^16 below 2^57."""
    return [Case("level", "lifted: " + c.name, _lift(c.x), 256.0 * c.thr, c.min_len, c.channel, rel=c.rel, half=c.half, rows=c.rows(),
                 T=f32(c.threshold() * f32(256)), before=_lift(c.before), after=_lift(c.after)) for c in _int16_level_cases()]


SPECIAL = np.array([LO, HI, -1, 0x0000FF, 0x00FF00, -0x010000], dtype=np.int32)      # bytes 0x800000, 0x7FFFFF, 0xFFFFFF, 0x0000FF, 0x00FF00, 0xFF0000


def value_cases():
    """What only 24 bits can hold, each with its rows written out by hand and checked against `expected`."""
    E = []

    def add(family, name, v, want, **kw):
        c = Case(family, name, np.asarray(v, dtype=np.int32), **kw)
        got = expected(c)[0].tolist()
        assert want is None or got == [list(w) for w in want], (name, got, want)
        E.append(c)
        return c

    assert pack(SPECIAL).tolist() == [[0, 0, 0x80], [0xFF, 0xFF, 0x7F], [0xFF, 0xFF, 0xFF], [0xFF, 0, 0], [0, 0xFF, 0], [0, 0, 0xFF]]
    x = np.concatenate([SPECIAL, SPECIAL[::-1], [0]])
    add("quiet", "the special bytes at thr 0", x, [(12, 1)], thr=0.0)
    add("quiet", "the special bytes at thr 1", x, [(2, 1), (9, 1), (12, 1)], thr=1.0)
    add("quiet", "the special bytes at thr 255", x, [(2, 2), (8, 2), (12, 1)], thr=255.0)
    add("quiet", "the special bytes at thr 65280", x, [(2, 3), (7, 3), (12, 1)], thr=65280.0)
    add("quiet", "the special bytes at thr 65536", x, [(2, 8), (12, 1)], thr=65536.0)
    add("quiet", "the special bytes at thr 2^23 - 1", x, [(1, 10), (12, 1)], thr=float(HI))
    add("quiet", "the special bytes at thr 2^23", x, [(0, 13)], thr=8388608.0)
    t = 0x012345                                                      # thr and thr + 1 differ in the low byte alone
    y = [t, t + 1, -t, -(t + 1), t + 256, t, t - 1, t + 1, -(t + 1) + 0x10000, -t]
    add("quiet", "thr and thr + 1 in the low byte", y, [(0, 1), (2, 1), (5, 2), (8, 2)], thr=float(t))
    add("quiet", "thr + 1 admits both", y, [(0, 4), (5, 5)], thr=float(t + 1))
    # held: the widest difference is 2^24 - 1, exact in fp32, and so is 2^24 - 2
    add("dead", "-2^23 | 2^23 - 1 at tol 2^24 - 2", [LO, HI, LO, HI, LO], [], kind=R.HELD, tol=float((1 << 24) - 2))
    add("dead", "-2^23 | 2^23 - 1 at tol 2^24 - 1", [LO, HI, LO, HI, LO], [(0, 5)], kind=R.HELD, tol=float((1 << 24) - 1))
    add("dead", "-2^23 | 2^23 - 2 at tol 2^24 - 2", [LO, HI - 1, HI, LO], [(0, 3)], kind=R.HELD, tol=float((1 << 24) - 2), min_len=2)
    add("dead", "steps of tol and tol + 1 in the low byte", [0x100, 0x1FF, 0x2FF, 0x3FE, 0x4FE, 0x5FF], [(0, 4)], kind=R.HELD, tol=255.0)
    add("dead", "the peak -2^23: T = 2^13", [LO, 8192, 8193, -8192, 0], [(1, 1), (3, 2)], kind=R.QUIET, rel=2.0 ** -10)
    add("dead", "the peak 2^23 - 1: T = 8191.999", [HI, 8192, 8191, -8192, 0], [(2, 1), (4, 1)], kind=R.QUIET, rel=2.0 ** -10)
    c = E[-1]
    assert expected(c)[1] == f32(HI) * f32(2.0 ** -10) and expected(E[-2])[1] == f32(8192)
    for h in (0, 7, 48):                                              # windows of full-scale samples: 2 h + 1 squares of 2^46 stay below 2^53
        n = 6 * (2 * h + 1) + 40
        add("level", f"all -2^23 at T = 2^23, h {h}", np.full(n, LO), [(0, n)], thr=8388608.0, half=h)
        add("level", f"all -2^23 at T = 2^23 - 1, h {h}", np.full(n, LO), [], thr=float(HI), half=h)
        add("level", f"all 2^23 - 1 at T = 2^23 - 1, h {h}", np.full(n, HI), [(0, n)], thr=float(HI), half=h)
        add("level", f"all 2^23 - 1 at T = 2^23 - 2, h {h}", np.full(n, HI), [], thr=float(HI - 1), half=h)
        w = np.where(np.arange(2 * D.CHUNK + 77) % 2 == 0, HI, LO).astype(np.int32)
        s = D.CHUNK - h - 3
        w[s:s + 2 * h + 1] = 255                                      # one low window across the chunk seam, in the low byte
        add("level", f"one window of 255 in full scale across the seam, h {h}", w, [(s, 2 * h + 1)], thr=255.0, half=h)
        add("level", f"one window of 255 at thr 254, h {h}", w, [], thr=254.0, half=h)
    return E


def channel_value_cases():
    """The special bytes interleaved: ch in {2, 3, 8}, one channel and joint; channel k holds SPECIAL rolled by k over 2 chunks + 77 times."""
    out = []
    n = 2 * D.CHUNK + 77
    for ch in (2, 3, 8):
        rng = np.random.default_rng(ch)
        v = (rng.integers(70000, HI, size=(n, ch)) * rng.choice([-1, 1], size=(n, ch))).astype(np.int32)
        for k in range(ch):
            v[100 + k:160, k] = np.resize(np.roll(SPECIAL[2:], k), 60 - k)          # quiet at thr 65536 from 100 + k on
            v[D.CHUNK - 9:D.CHUNK + 5 + k, k] = (k + 1) * 0x101 * (-1) ** k         # held, across the chunk seam
        v[n - 4:, :] = -1
        for c in (0, ch - 1, -1):
            out.append(Case("quiet", f"{ch} channels, channel {c}", v, 65536.0, 2, c))
            out.append(Case("dead", f"{ch} channels, channel {c}, any", v, 65536.0, 2, c, R.ANY, 2.0 ** -9, 0.0))
            out.append(Case("level", f"{ch} channels, channel {c}, h 7", v, 65536.0, 2, c, half=7))
        joint = expected(out[-3])[0].tolist()
        assert [100 + ch - 1, 60 - ch + 1] in joint and [n - 4, 4] in joint, joint
    return out


def all_cases():
    return lifted_quiet_cases((1, 7, 2049, 4101)) + lifted_dead_cases() + lifted_level_cases() + value_cases() + channel_value_cases()


# ------------------------------------------------------------------------------------------------------------ the patch case
N_FILE = 3 * 2048 + 77
AMP = 0.3


def patch_case(sr, fade_f):
    """tests/test_gpu_rate.py's case, restated: five spans over two windows of two contexts on a file of 3 * 2048 + 77 samples -- A
    reaches in front of sample 0, B and E cross chunk seams, C and D overlap their ramps and belong to two windows, E is cut by lim_f,
    and row 1 runs 10 samples past its context's end.  -> spans, windows, chunks, gen (2, lrow) fp32, v (N_FILE) int32 at amplitude 0.3."""
    import torch
    P, Q = G.rate_ratio(sr)
    H = RR.reach(sr)
    n22 = -(-N_FILE * P // Q)
    gap = 3 + fade_f // 2
    raw = [(30, 100, 0), (2048 - 60, 150, 0), (2700, 80, 0), (2780 + gap, 90, 1), (3 * 2048 - 100, 150, 1)]
    reg = lambda s, l: (max(s - fade_f, 0), s + l + fade_f)
    len0 = (reg(*raw[2][:2])[1] - 1) * P // Q + 1 + H + 5
    ws1 = reg(*raw[3][:2])[0] * P // Q - H - 3
    lim1 = (3 * 2048 + 6) * P // Q
    windows = [(0, 0, len0, len0), (1, ws1, lim1 + 10 - ws1, lim1)]
    assert ws1 > 0 and lim1 + 10 <= n22
    lims = [min(G.file_lim(w[3], sr), N_FILE) for w in windows]
    spans = [(s, l, w, lims[w]) for s, l, w in raw]
    assert raw[4][0] < lims[1] < raw[4][0] + raw[4][1] and lims[0] > reg(*raw[2][:2])[1]
    chunks = G.region_chunks(G.file_regions([(s, l) for s, l, _, _ in spans], [sp[3] for sp in spans], fade_f))
    assert [c for c, _, _ in chunks] == [0, 1, 2, 3]
    g = torch.Generator().manual_seed(sr + fade_f)
    lrow = max(w[2] for w in windows) + 3
    gen = ((torch.rand(2, lrow, generator=g) * 2 - 1) * AMP).contiguous()
    v = np.trunc((torch.rand(N_FILE, generator=g).numpy().astype(np.float64) * 2 - 1) * AMP * HI).astype(np.int32)
    return dict(spans=spans, windows=windows, chunks=chunks, gen=gen, v=v, lrow=lrow)
