"""Float64 references of the log-mel front-end's kernels (frontend_kernels.hip, mel_run in api.hip), stage by stage, each with an
explicit per-element bound, and the shapes both test files run (tests/test_frontend_ref.py on the CPU, tests/test_gpu_frontend_ops.py
on the device).

Every reference takes the stage's OWN input -- the fp32 clip, then the taps "mel_peak", "mel_frames", "mel_spec" exactly as the kernels
stored them -- and computes in float64.  The bounds are derived in the docstrings from the kernels' arithmetic; none is fitted to a
measurement.  u = U = 2^-24 is the unit roundoff of one fp32 VALU operation (round to nearest; division and square root are the
correctly rounded ones, the build has no fast-math flag); gamma, FTZ, ulp_f32 and the tap-GEMM's coefficient are those of encoder_ref.py
and vocoder_ref.py.

The stages (constants of I_ea/dataset/mel_dump.py:11-20: n_fft = win = 1024, hop 441, reflect pad 312, 80 bands):
    peak    max |x| over the clip's own samples with its spans zeroed                                      -> (B)
    frames  w[k] = (x[j] / div) * 0.95 * hann[k], j = m hop + k - pad reflected into [0, N) without repeating the edge, x[j] = 0
            inside a span; stored folded as [s_0 .. s_512 | 15 zeros | 0, d_1 .. d_511]                     -> (B, Tm, 1040)
    spec    Re X[n] = sum_k s_k cos(2 pi n k / 1024), Im X[n] = -sum_k d_k sin(2 pi n k / 1024), two fp32 tap-GEMMs
            -> rows [re(0..512) | 3 pad | im(0..512) | 3 pad]                                                -> (B, Tm, 1032)
    log-mel log(max(sum_f basis[i, f] sqrt(re^2 + im^2 + 1e-9), 1e-5))                                       -> (B, 80, Tm)
"""
import collections
import functools

import numpy as np
import torch

from tests.encoder_ref import U, gamma, ulp_f32
from tests.vocoder_ref import FTZ, tapgemm_ref

NFFT, HOP, PAD, NMEL, NBIN, HALF = 1024, 441, 312, 80, 513, 512
KC, KS, FRAME, IMOFF, LDSPEC = 528, 512, 1040, 516, 1032              # the folded frame and the spec row of api.hip (FE_*)
TINY = float(np.finfo(np.float32).tiny)                                 # 1.17549435e-38: a peak below it leaves the clip unscaled
C095 = float(np.float32(0.95))                                          # the kernels' 0.95f, 1e-9f and 1e-5f as the values they are
EPS_MAG = float(np.float32(1e-9))
CLAMP = float(np.float32(1e-5))
SECOND = 1.0 + 2.0 ** -10                                               # covers the products of two or more roundings (u^2 terms)

# frames: roundings of one windowed sample -- the division, the product with 0.95 and the product with hann[k] (3 u) -- a last-bit
# difference between the host's cos and numpy's in the fp32 Hann table (one fp32 ulp of hann[k] = at most 2 u relative: libm's cos is
# within an ulp of FLOAT64, which moves the fp32 rounding of 0.5 - 0.5 cos by at most one fp32 step, also where hann is 1e-5), and
# the fp32 add or subtract of the fold (u on |w[k] + w[n-k]| <= |w[k]| + |w[n-k]|): c = 3 + 2 + 1.  A product contracted into the add
# drops a rounding, and normalize = 0 drops two.
C_FRAMES = 6
# log-mel: the error allowance of logf in ulps of |log|.  The device library's log follows the OpenCL C accuracy table (OpenCL C 3.0
# specification, section 7.4 "Relative Error as ULPs": log <= 3 ulp in single precision), which is the requirement ROCm's ocml is built to.
LOGF_ULPS = 3


def mel_frames(N):
    return 0 if N + 2 * PAD < NFFT else (N + 2 * PAD - NFFT) // HOP + 1


def hann32(symmetric=False):
    """The kernels' Hann table restated: float32(0.5 - 0.5 cos(2 pi k / 1024)) computed in float64 (torch.hann_window's periodic form)."""
    k = np.arange(NFFT, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / (NFFT - 1 if symmetric else NFFT))).astype(np.float32)


def source_index(N, Tm, edge_repeat=False):
    """(Tm, 1024) clip positions frame m reads at k: m hop + k - pad, reflected at 0 and at N - 1 (the clip's OWN end) without
    repeating the edge sample (F.pad(mode="reflect")).  edge_repeat: the self-tests' mistake."""
    j = np.arange(Tm)[:, None] * HOP + np.arange(NFFT)[None, :] - PAD
    r = 1 if edge_repeat else 0
    j = np.where(j < 0, -j - r, j)
    return np.where(j >= N, 2 * (N - 1) - j + r, j)


def span_mask(N, spans):
    """bool (N): the samples inside some span [start, start + len) of the clip; a span may run past N."""
    m = np.zeros(N, dtype=bool)
    for s, l in spans or ():
        m[min(s, N):min(s + l, N)] = True
    return m


# --------------------------------------------------------------------------------------------------------------------- peak
def peak_ref(x, N, spans):
    """max |x| over the clip's own N samples with the spans zeroed, as the fp32 value it is: |x| and max round nothing, so the
    kernel's result is compared bit for bit."""
    v = np.abs(np.asarray(x[:N], dtype=np.float32))
    v[span_mask(N, spans)] = 0
    return np.float32(v.max())


# --------------------------------------------------------------------------------------------------------------------- frames
FramesRef = collections.namedtuple("FramesRef", "ref E zero")


def frames_ref(x, N, spans, peak, normalize):
    """The folded frame matrix of one clip in float64 from the fp32 clip x (its first N samples), its spans and the CAPTURED peak.
    -> FramesRef(ref (Tm, 1040), E, zero).

    w[k] = (v / div) * 0.95f * hann[k] with v = 0 inside a span, div = peak unless peak < the smallest normal float (then 1), hann the
    fp32 table (hann32) -- every factor the fp32 value the kernel holds, the arithmetic in float64.  Folded: s_k = w[k] + w[1024 - k],
    d_k = w[k] - w[1024 - k], s_0 = w[0], s_512 = w[512].
    Bound: the kernel rounds each windowed sample three times and the fold once, and its Hann table may differ from this one in the
    last bit (C_FRAMES): |got - ref| <= C_FRAMES u (1 + 2^-10) (|w[k]| + |w[1024 - k]|) + 4 * 2^-149, the last term for results of
    the four operations that are subnormal (each then rounds to a multiple of 2^-149 instead of relatively).  The compiler may
    contract a product into the fold's add (-O3, no fast-math: contraction is allowed), which removes a rounding, so bit identity with
    an fp32 restatement cannot be demanded but the bound holds either way.
    zero: the elements whose two source samples are both exactly zero in the reference -- d_0, the columns 513 .. 527, every column of
    a frame that lies wholly inside a span, s_0 (hann[0] = 0) -- must be exactly zero: products and sums of zeros round nothing."""
    Tm = mel_frames(N)
    xm = np.asarray(x[:N], dtype=np.float32).astype(np.float64)
    xm[span_mask(N, spans)] = 0.0
    v = xm[source_index(N, Tm)]
    if normalize:
        pk = float(peak)
        v = v / (1.0 if pk < TINY else pk) * C095
    w = v * hann32().astype(np.float64)[None, :]
    a = np.abs(w)
    ref = np.zeros((Tm, FRAME))
    mag = np.zeros((Tm, FRAME))
    back = slice(NFFT - 1, HALF, -1)                                    # w[1024 - k] for k = 1 .. 511
    ref[:, 0], ref[:, HALF] = w[:, 0], w[:, HALF]
    mag[:, 0], mag[:, HALF] = a[:, 0], a[:, HALF]
    ref[:, 1:HALF] = w[:, 1:HALF] + w[:, back]
    ref[:, KC + 1:KC + HALF] = w[:, 1:HALF] - w[:, back]
    mag[:, 1:HALF] = mag[:, KC + 1:KC + HALF] = a[:, 1:HALF] + a[:, back]
    zero = mag == 0
    E = np.where(zero, 0.0, C_FRAMES * U * SECOND * mag + 4 * 2.0 ** -149)
    return FramesRef(ref, E, zero)


def check_frames(got, fr):
    """-> dict(bad, ratio (Tm, 1040): err / E, inf where a required zero is not one)."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - fr.ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(fr.zero, np.where(got == 0, 0.0, np.inf), err / np.where(fr.zero, 1.0, fr.E))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    return dict(bad=int((ratio > 1).sum()), ratio=ratio)


# --------------------------------------------------------------------------------------------------------------------- spec
@functools.lru_cache(maxsize=None)
def _twiddles():
    """cos and sin of 2 pi (n k mod 1024) / 1024 in float64, (513, 1024): the argument reduced exactly."""
    r = (np.arange(NBIN)[:, None] * np.arange(NFFT)[None, :]) % NFFT
    a = 2.0 * np.pi * r / NFFT
    return np.cos(a), np.sin(a)


@functools.lru_cache(maxsize=None)
def dft_tables32(sin_sign=-1.0):
    """The two fp32 tables of ensure_frontend restated: cosines (513, 528) with the columns 513 .. 527 zero, and MINUS sines (513, 512)
    with column 0 zero (d_0 = 0).  sin_sign = +1: the self-tests' mistake."""
    c, s = _twiddles()
    tc = np.zeros((NBIN, KC), dtype=np.float32)
    ts = np.zeros((NBIN, KS), dtype=np.float32)
    tc[:, :HALF + 1] = c[:, :HALF + 1].astype(np.float32)
    ts[:, 1:HALF] = (sin_sign * s[:, 1:HALF]).astype(np.float32)
    return tc, ts


def unfold(frames):
    """(R, 1040) folded frames -> (R, 1024) windowed frames in float64: w[k] = (s_k + d_k) / 2, w[1024 - k] = (s_k - d_k) / 2 (the sum
    of two fp32 values in float64 is off by at most 2^-53 of the larger: nine orders below the bounds)."""
    f = np.asarray(frames, dtype=np.float64)
    s, d = f[:, :HALF + 1], f[:, KC:KC + HALF]
    w = np.zeros((f.shape[0], NFFT))
    w[:, 0], w[:, HALF] = s[:, 0], s[:, HALF]
    w[:, 1:HALF] = 0.5 * (s[:, 1:HALF] + d[:, 1:HALF])
    w[:, NFFT - 1:HALF:-1] = 0.5 * (s[:, 1:HALF] - d[:, 1:HALF])
    return w


def spec_ref(frames):
    """The exact DFT X[n] = sum_{k < 1024} w[k] exp(-2 pi i n k / 1024), n = 0 .. 512, of the CAPTURED folded frames, unfolded here, with
    float64 twiddles.  -> (re, im, E_re, E_im), each (R, 513).

    Bound.  The kernel multiplies the folded operands with fp32 tables in the exact-fp32 tap-GEMM: tapgemm_ref(..., "f32", ...)'s
    coefficient gamma(K + 1) + u (1 + gamma(K + 1)) on S = sum |operand||table| (+ (K + 1) FTZ), K = 528 for the cosine half and
    512 for the sine half (the launches' Cin), plus u (1 + 2^-20) S for the table: float32(cos) is within u of the float64 cosine
    relatively.  Where the true twiddle is zero (sin pi, cos pi/2: n k = 256, 512, 768 mod 1024) that relative statement says nothing:
    the float64 argument 2 pi r / 1024 carries the rounding of pi and of one product, at most 2^-52 of an argument <= 2 pi, and cos and
    sin pass that on one to one, so both the library's table and the twiddles used here hold about 1.2e-16 there instead of 0.  Both are
    covered by an absolute 2^-48 sum |operand| (2 x (2 pi 2^-52 + 2^-53)), eight orders below u S everywhere else.
    The zero columns of table and frame add exact zeros."""
    f32 = np.ascontiguousarray(np.asarray(frames, dtype=np.float32))
    c, s = _twiddles()
    w = unfold(f32)
    re, im = w @ c.T, -(w @ s.T)
    tc, ts = dft_tables32()
    out = []
    for op, tab, K in ((f32[:, :KC], tc, KC), (f32[:, KC:], ts, KS)):
        t = tapgemm_ref(torch.from_numpy(op.copy()), torch.from_numpy(tab), None, "f32", lambda a, ww: a @ ww.t(), K)
        S = np.abs(op.astype(np.float64)) @ np.abs(tab.astype(np.float64)).T
        out.append(t.E.numpy() + U * (1 + 2.0 ** -20) * S + 2.0 ** -48 * np.abs(op.astype(np.float64)).sum(axis=1, keepdims=True))
    return re, im, out[0], out[1]


def check_spec(got, frames):
    """got (R, 1032) captured spec rows, frames (R, 1040) captured folded frames.  The pad columns 513 .. 515 and 1029 .. 1031 hold
    whatever the workspace held and are sliced away.  -> dict(bad, ratio (R, 2, 513))."""
    got = np.asarray(got, dtype=np.float64)
    re, im, Ere, Eim = spec_ref(frames)
    g = np.stack([got[:, :NBIN], got[:, IMOFF:IMOFF + NBIN]], axis=1)
    ref, E = np.stack([re, im], axis=1), np.stack([Ere, Eim], axis=1)
    ratio = np.where(np.isfinite(g), np.abs(g - ref) / E, np.inf)
    return dict(bad=int((ratio > 1).sum()), ratio=ratio)


# --------------------------------------------------------------------------------------------------------------------- log-mel
@functools.lru_cache(maxsize=None)
def oracle_basis():
    from oracle import ref_cpu as R
    return R.mel_filterbank()


def logmel_interval(spec):
    """The interval every log-mel value must lie in, from the CAPTURED spec rows (R, 1032) and the oracle's mel_filterbank().
    -> (lo, hi), each (R, 80).

    mag = sqrt(re^2 + im^2 + 1e-9f): the two squares and the two adds are sums of non-negative terms, each term passing through at
    most three roundings, the root halves that and adds its own: |dmag| <= (3 / 2 + 1) u (1 + 2^-10) mag =: E_mag.
    acc = sum over ALL 513 bins of basis[i, f] mag[f] in float64 (a band limit that drops a non-zero bin shows).  The kernel's fma
    chain over a band of `width` bins, from the rounded magnitudes: |dacc| <= sum basis E_mag + gamma(W + 1, u) sum basis (mag + E_mag)
    with W the widest band (a chain of W fmas is gamma(W); + 1 keeps the bound valid for a product rounded apart from its add),
    + u sum basis mag for the filterbank: the library builds its table in C++ and the oracle in numpy, the two can differ in the last
    bit of an entry (at most 2 u of that entry's term) where the float64 values straddle a rounding point, which happens for a few
    entries of a band at the most, never for half its mass.
    got must lie in [log(max(acc - E, 1e-5f)) - d, log(max(acc + E, 1e-5f)) + d], d = LOGF_ULPS fp32 ulps of the larger |log| of the
    two ends: log and max are monotone, so the interval needs no list of excluded near-clamp elements, and none is skipped."""
    g = np.asarray(spec, dtype=np.float64)
    re, im = g[:, :NBIN], g[:, IMOFF:IMOFF + NBIN]
    mag = np.sqrt(re * re + im * im + EPS_MAG)
    Emag = 2.5 * U * SECOND * mag
    b = oracle_basis().astype(np.float64)
    W = int((b != 0).sum(axis=1).max())
    acc = mag @ b.T
    E = Emag @ b.T + gamma(W + 1, U) * ((mag + Emag) @ b.T) + U * acc
    lo, hi = np.log(np.maximum(acc - E, CLAMP)), np.log(np.maximum(acc + E, CLAMP))
    d = LOGF_ULPS * ulp_f32(torch.from_numpy(np.maximum(np.abs(lo), np.abs(hi)))).numpy()
    return lo - d, hi + d


def check_logmel(got, spec):
    """got (R, 80): the log-mel rows of the frames whose spec rows are given.  -> dict(bad, ratio (R, 80): distance from the middle
    of the interval in half-widths)."""
    got = np.asarray(got, dtype=np.float64)
    lo, hi = logmel_interval(spec)
    ok = (got >= lo) & (got <= hi)
    ratio = np.where(np.isfinite(got), np.abs(got - 0.5 * (lo + hi)) / (0.5 * (hi - lo)), np.inf)
    return dict(bad=int((~ok).sum()), ratio=ratio)


def float64_chain(x, spans, normalize=True):
    """The whole front-end of one clip in float64 (its own peak; no bound): (80, Tm).  For pinning the references to the oracle."""
    N = len(x)
    fr = frames_ref(x, N, spans, peak_ref(x, N, spans), normalize)
    c, s = _twiddles()
    w = unfold(fr.ref)
    mag = np.sqrt((w @ c.T) ** 2 + (w @ s.T) ** 2 + EPS_MAG)
    return np.log(np.maximum(mag @ oracle_basis().astype(np.float64).T, CLAMP)).T


# --------------------------------------------------------------------------------------------------------------------- one batch
def frame_kinds(N, spans):
    """Per frame of a clip: (spans in reach, head reflection, tail reflection).  In reach = non-empty spans that hold a sample the
    frame reads (directly or reflected) -- what FeFrameSpans keeps between k0 and k1, zero-length spans aside."""
    Tm = mel_frames(N)
    j = source_index(N, Tm)
    out = []
    for m in range(Tm):
        lo, hi = int(j[m].min()), int(j[m].max())
        n = sum(1 for s, l in spans or () if l > 0 and s <= hi and min(s + l, N) > lo)
        a = m * HOP - PAD
        out.append((n, a < 0, a + NFFT - 1 >= N))
    return out


def check_batch(case, peak, frames, spec, mel):
    """Every stage of one batch against its reference.  peak (B) or None (normalize off), frames (B, Tm, 1040), spec (B, Tm, 1032),
    mel (B, 80, Tm): numpy, as captured.  Frames past a ragged clip's own are skipped in the taps (not written) and must be exactly zero
    in the log-mel.  -> {stage: dict(bad, edge, interior)}: failures and the largest ratio over the edge frames (reflecting, or with
    a span in reach) and over the interior ones."""
    B, Ns = case.wave.shape
    res = {k: dict(bad=0, edge=0.0, interior=0.0) for k in ("peak", "frames", "spec", "logmel", "tail")}

    def fold_in(stage, r, edge):
        res[stage]["bad"] += r["bad"]
        rows = r["ratio"].reshape(len(edge), -1).max(axis=1)
        for sel, key in ((edge, "edge"), (~edge, "interior")):
            if sel.any():
                res[stage][key] = max(res[stage][key], float(rows[sel].max()))

    for b in range(B):
        N = Ns if case.lens is None else int(case.lens[b])
        sp = case.spans[b] if case.spans is not None else []
        tm = mel_frames(N)
        edge = np.array([n > 0 or h or t for n, h, t in frame_kinds(N, sp)])
        if case.normalize:
            ok = np.float32(peak[b]).tobytes() == peak_ref(case.wave[b], N, sp).tobytes()
            res["peak"]["bad"] += 0 if ok else 1
        fold_in("frames", check_frames(frames[b, :tm], frames_ref(case.wave[b], N, sp, peak[b] if case.normalize else None, case.normalize)), edge)
        fold_in("spec", check_spec(spec[b, :tm], frames[b, :tm]), edge)
        fold_in("logmel", check_logmel(mel[b, :, :tm].T, spec[b, :tm]), edge)
        res["tail"]["bad"] += int((mel[b, :, tm:] != 0).sum())
    return res


# --------------------------------------------------------------------------------------------------------------------- the shapes
Case = collections.namedtuple("Case", "name entry wave lens spans normalize")
Case.__doc__ = """entry: "single" (si_mel_frontend), "varlen" (si_mel_frontend_varlen) or "spans" (si_mel_frontend_spans, with lens: ragged);
wave (B, Ns) fp32; lens (B) or None; spans: per clip a list of (start, len), at most one for single / varlen, None: no mask at all."""

LENGTHS = (400, 841, 1281, 1282, 4099, 4100)          # Tm = 1 (reflects at both ends), 2, 2 | 3 (frame-count boundary), odd row | 16-byte loads
GAINS = (0.3, 1.7, 0.05)
FIVE = [(130, 3), (400, 1), (640, 2), (900, 50), (1152, 1)]             # five spans inside one frame's reach
SIXTEEN = [(130 + 60 * i, 7) for i in range(16)]                        # SI_MAX_SPANS spans inside one frame (130 .. 1037 of frame 1's 129 .. 1152)


def clips(N, seed=11):
    """Three clips of N samples (synth_wave scaled by 0.3, 1.7 and 0.05) with planted extremes: clip 0 a NEGATIVE peak at the index just
    before N & ~3 (the last sample of the peak kernel's 16-byte loop), clip 1 its peak at N & ~3 (the first sample of the scalar tail;
    the last vector's first sample when N is a multiple of 4), clip 2 its peak at the last sample."""
    from speech_inpainting_amd import synth
    w = synth.synth_wave(3, N, seed, sr=22050).numpy() * np.array(GAINS, dtype=np.float32)[:, None]
    i4 = (N & ~3) if N & 3 else N - 4
    w[0, i4 - 1] = -1.5 * np.abs(w[0]).max()
    w[1, i4] = 1.25 * np.abs(w[1]).max()
    w[2, N - 1] = 2.0 * np.abs(w[2]).max()
    return w.astype(np.float32)


def _plant(w, spans, factor=8.0):
    """A sample larger than the clip's peak inside the first non-empty span of each clip: the peak must ignore it."""
    for b, sp in enumerate(spans):
        for s, l in sp:
            if l > 0 and s < w.shape[1]:
                w[b, min(s + (l - 1) // 2, w.shape[1] - 1)] = factor * np.abs(w[b]).max()
                break
    return w


def _rows(w, lens, Ns):
    """Clips of lens[b] samples in rows of Ns, every row filled past its length with 1e30."""
    out = np.full((len(lens), Ns), 1e30, dtype=np.float32)
    for b, n in enumerate(lens):
        out[b, :n] = w[b % len(w), :n]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every batch of section "shapes" as a tuple of Case.  Frame m of a clip reads m 441 - 312 .. + 1023: at N = 1282 the frames read
    [0, 711] (head reflection: 1 .. 312 twice), [129, 1152] and [570, 1281] (tail reflection: 969 .. 1280 twice)."""
    out = []
    for N in LENGTHS:
        one = [[(N // 3, 50)], [(0, 20)], [(N - 30, 30)]]               # interior, at the head, at the tail
        out.append(Case(f"single-{N}-norm", "single", _plant(clips(N), one), None, one, True))
        out.append(Case(f"single-{N}-raw-nomask", "single", clips(N, 13), None, None, False))
        out.append(Case(f"single-{N}-norm-nomask", "single", clips(N, 17), None, None, True))   # the planted extremes ARE the peak
    N = 1282
    four = np.concatenate([clips(N, 19), clips(N, 23)[:1]])
    # five and sixteen spans in one frame's reach, an empty table next to full ones, spans at sample 0 and on [1, 2) (touching; the
    # first frame reads sample 1 twice)
    tab_a = [FIVE, SIXTEEN, [], [(0, 1), (1, 1)]]
    # a span over the last sample; a span inside 969 .. 1280, which the last frame reads twice through the tail reflection (no sample is
    # reached ONLY reflected: the pad of 312 is shorter than half a frame); touching and zero-length spans; a span running past the end
    tab_b = [[(1281, 1)], [(1000, 100)], [(300, 40), (340, 60), (500, 0), (700, 0), (700, 5)], [(1200, 500)]]
    for nm, tab in (("a", tab_a), ("b", tab_b)):
        for norm in (True, False):
            out.append(Case(f"spans-{nm}-{'norm' if norm else 'raw'}", "spans", _plant(four.copy(), tab), None, tab, norm))
    # ragged: rows of 1282 and of 4100, filled past each clip with 1e30; one span crosses n_len[b]
    lens = (1282, 1281, 841, 400)
    w4 = np.concatenate([clips(N, 29), clips(N, 31)[:1]])
    one = [[(600, 30)], [(0, 20)], [(800, 100)], [(390, 10)]]           # clip 2: [800, 900) crosses its 841 samples
    out.append(Case("varlen-1282-norm", "varlen", _rows(_plant(w4.copy(), one), lens, N), lens, one, True))
    out.append(Case("varlen-1282-raw-nomask", "varlen", _rows(w4, lens, N), lens, None, False))
    tab_r = [FIVE, [(1270, 50)], [], [(0, 1), (1, 1), (200, 3), (398, 7)]]   # clip 1: [1270, 1320) crosses its 1281 samples
    out.append(Case("spans-ragged-1282-norm", "spans", _rows(_plant(w4.copy(), tab_r), lens, N), lens, tab_r, True))
    lens = (4100, 4099, 1282, 400)
    w5 = np.concatenate([clips(4100, 37), clips(4100, 41)[:1]])
    one = [[(2000, 64)], [(4090, 20)], [(0, 9)], [(100, 1)]]            # clip 1: [4090, 4110) crosses its 4099 samples
    out.append(Case("varlen-4100-norm", "varlen", _rows(_plant(w5.copy(), one), lens, 4100), lens, one, True))
    # a fully masked clip, a silent clip, and a clip whose peak is the subnormal 1e-39: unscaled, as R.peak_normalize_095 leaves it
    w = clips(N, 43)
    w[1] = 0.0
    w[2] = (w[2].astype(np.float64) * (1e-39 / np.abs(w[2]).max())).astype(np.float32)
    out.append(Case("special-1282-norm", "single", w, None, [[(0, N)], [(0, 0)], [(0, 0)]], True))
    return tuple(out)


def coverage():
    """The frame x span situations the cases reach: {"spans": set of spans-in-reach counts, "reflect": set of {"none", "head", "tail",
    "both"}} over the cases that run the table kernels ("spans") and over all."""
    counts, refl = set(), set()
    for c in cases():
        for b in range(c.wave.shape[0]):
            N = c.wave.shape[1] if c.lens is None else c.lens[b]
            for n, h, t in frame_kinds(N, c.spans[b] if c.spans is not None else []):
                if c.entry == "spans":
                    counts.add(n)
                refl.add("both" if h and t else "head" if h else "tail" if t else "none")
    return dict(spans=counts, reflect=refl)
