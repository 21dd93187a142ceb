"""CPU self-tests of tests/frontend_ref.py: the float64 chain agrees with the oracle, an fp32 emulation of the front-end's kernels (numpy
float32 in the kernels' operation order, their reflect / mask / fold logic restated) passes every bound on every shape of
frontend_ref.cases(), and each seeded mistake fails at least one bound on those shapes."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import frontend_ref as FR

f32 = np.float32

MISTAKES = ("reflect_edge_repeat", "reflect_row_end", "span_end_inclusive", "span_start_late", "third_span_ignored", "peak_sees_masked",
            "peak_sees_row", "hann_symmetric", "d_sign", "s_half_doubled", "col513_nonzero", "sin_plus", "hi_short", "no_eps",
            "subnormal_divisor")


FIRST = {"subnormal_divisor": "special-1282-norm", "reflect_row_end": "varlen-1282-norm", "peak_sees_row": "varlen-1282-norm",
         "third_span_ignored": "spans-a-norm"}

# ----------------------------------------------------------------------------------------------------------- the emulation
def emu_peak(x, N, spans, bug=None):
    """wave_peak[_spans]_kernel: max |x| over [0, N) with the spans' samples as zero."""
    n = len(x) if bug == "peak_sees_row" else N
    v = np.abs(x[:n].astype(f32))
    if bug != "peak_sees_masked":
        v[FR.span_mask(n, spans)] = 0
    return f32(v.max())


def emu_reach(spans, a, N, bug=None):
    """FeFrameSpans: the spans that frame [a, a + 1024) can touch -- [jlo, jhi] as the kernel computes it, the first two kept, the rest
    walked."""
    z = a + FR.NFFT - 1
    jlo, jhi = max(a, 0), min(z, N - 1)
    if a < 0:
        jlo, jhi = 0, min(max(jhi, -a), N - 1)
    if z >= N:
        jlo, jhi = max(min(jlo, 2 * (N - 1) - z), 0), N - 1
    k0, k1 = 0, len(spans)
    while k0 < k1 and spans[k0][0] + spans[k0][1] <= jlo:
        k0 += 1
    while k1 > k0 and spans[k1 - 1][0] > jhi:
        k1 -= 1
    return spans[k0:min(k1, k0 + 2) if bug == "third_span_ignored" else k1]


def emu_frames(x, N, spans, peak, normalize, table, bug=None):
    """mel_frames[_spans]_kernel in float32: ((v / div) * 0.95f) * hann[k], folded.  table: the spans kernel's per-frame reach."""
    Tm = FR.mel_frames(N)
    Nr = len(x) if bug == "reflect_row_end" else N
    j = FR.source_index(Nr, Tm, edge_repeat=bug == "reflect_edge_repeat")
    sp = list(spans or ())
    if bug == "span_end_inclusive":
        sp = [(s, l + 1) for s, l in sp]
    if bug == "span_start_late":
        sp = [(s + 1, max(l - 1, 0)) for s, l in sp]
    hann = FR.hann32(symmetric=bug == "hann_symmetric")
    div = f32(1)
    if normalize:
        pk = f32(peak)
        div = pk if (pk > 0 if bug == "subnormal_divisor" else pk >= f32(FR.TINY)) else f32(1)
    out = np.zeros((Tm, FR.FRAME), dtype=f32)
    for m in range(Tm):
        reach = emu_reach(sp, m * FR.HOP - FR.PAD, N, bug) if table else sp
        hit = FR.span_mask(len(x), reach)
        v = np.where(hit[j[m]], f32(0), x.astype(f32)[j[m]])
        if normalize:
            with np.errstate(over="ignore", invalid="ignore"):
                v = (v / div) * f32(0.95)
        w = (v * hann).astype(f32)
        back = w[FR.NFFT - 1:FR.HALF:-1]
        out[m, 0] = w[0]
        out[m, FR.HALF] = w[FR.HALF] + w[FR.HALF] if bug == "s_half_doubled" else w[FR.HALF]
        out[m, 1:FR.HALF] = w[1:FR.HALF] + back
        d = w[1:FR.HALF] - back
        out[m, FR.KC + 1:FR.KC + FR.HALF] = -d if bug == "d_sign" else d
        if bug == "col513_nonzero":
            out[m, FR.HALF + 1] = w[FR.HALF - 1]
    return out


def emu_spec(frames, bug=None):
    """The two fp32 GEMMs against the fp32 tables; the pad columns of a row hold garbage."""
    tc, ts = FR.dft_tables32(1.0 if bug == "sin_plus" else -1.0)
    out = np.full((frames.shape[0], FR.LDSPEC), 1e30, dtype=f32)
    out[:, :FR.NBIN] = frames[:, :FR.KC] @ tc.T
    out[:, FR.IMOFF:FR.IMOFF + FR.NBIN] = frames[:, FR.KC:] @ ts.T
    return out


def emu_project(spec, bug=None):
    """mel_project_kernel: sqrtf(re re + im im + 1e-9f), one multiply-add per bin of the band [lo, hi) in bin order, logf(fmaxf(., 1e-5f))."""
    re, im = spec[:, :FR.NBIN], spec[:, FR.IMOFF:FR.IMOFF + FR.NBIN]
    with np.errstate(over="ignore", invalid="ignore"):                 # (a seeded mistake may read the 1e30 past a clip)
        t = re * re + im * im
        mag = np.sqrt(t if bug == "no_eps" else t + f32(1e-9)).astype(f32)
    basis = FR.oracle_basis()
    nz = basis != 0
    lo = nz.argmax(axis=1)
    hi = FR.NBIN - nz[:, ::-1].argmax(axis=1) - (1 if bug == "hi_short" else 0)
    acc = np.zeros((spec.shape[0], FR.NMEL), dtype=f32)
    for f in range(FR.NBIN):
        band = (lo <= f) & (f < hi)
        if band.any():
            acc[:, band] = acc[:, band] + basis[band, f][None, :] * mag[:, f][:, None]
    return np.log(np.maximum(acc, f32(1e-5))).astype(f32)


def emulate(case, bug=None):
    """One batch through the emulated kernels -> (peak, frames, spec, mel) shaped as the taps and the output.  Frames past a ragged
    clip's own: taps stale (1e30), log-mel zero."""
    B, Ns = case.wave.shape
    Tm = FR.mel_frames(Ns)
    peak = np.zeros(B, dtype=f32)
    frames = np.full((B, Tm, FR.FRAME), 1e30, dtype=f32)
    spec = np.full((B, Tm, FR.LDSPEC), 1e30, dtype=f32)
    mel = np.zeros((B, FR.NMEL, Tm), dtype=f32)
    for b in range(B):
        N = Ns if case.lens is None else case.lens[b]
        sp = case.spans[b] if case.spans is not None else []
        tm = FR.mel_frames(N)
        if case.normalize:
            peak[b] = emu_peak(case.wave[b], N, sp, bug)
        frames[b, :tm] = emu_frames(case.wave[b], N, sp, peak[b], case.normalize, case.entry == "spans", bug)
        spec[b, :tm] = emu_spec(frames[b, :tm], bug)
        mel[b, :, :tm] = emu_project(spec[b, :tm], bug).T
    return (peak if case.normalize else None), frames, spec, mel


def _bad(case, bug=None):
    return {k: v["bad"] for k, v in FR.check_batch(case, *emulate(case, bug)).items()}


# ----------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("N", [400, 1281, 1282, 22063])
def test_float64_chain_agrees_with_the_oracle(N):
    """Composed end to end from the clip, the float64 references agree with R.masked_mel on pre-zeroed clips within the 2e-4 of
    tests/test_gpu_frontend.py."""
    w = FR.clips(N)
    spans = [[(N // 3, 60)], [(0, 25)], [(N - 40, 40)]]
    ref = R.masked_mel(w, [s[0][0] for s in spans], [s[0][0] + s[0][1] for s in spans]).numpy()
    for b in range(3):
        got = FR.float64_chain(w[b], spans[b])
        assert got.shape == ref[b].shape == (80, FR.mel_frames(N))
        assert np.abs(got - ref[b]).max() <= 2e-4, (N, b, np.abs(got - ref[b]).max())
    raw = R.masked_mel(w, None, None, normalize=False).numpy()
    assert np.abs(FR.float64_chain(w[1], [], normalize=False) - raw[1]).max() <= 2e-4


@pytest.mark.parametrize("case", FR.cases(), ids=lambda c: c.name)
def test_fp32_emulation_passes_every_bound(case):
    res = FR.check_batch(case, *emulate(case))
    assert all(v["bad"] == 0 for v in res.values()), res
    worst = max(max(v["edge"], v["interior"]) for v in res.values())
    assert 0 < worst <= 1


@pytest.mark.parametrize("bug", MISTAKES)
def test_seeded_mistake_fails_a_bound(bug):
    """Each mistake, seeded into the emulation, fails at least one stage's bound on at least one of the shapes (and the first such shape
    is reported)."""
    for case in sorted(FR.cases(), key=lambda c: c.name != FIRST.get(bug)):     # (the shape made for it first; then all the others)
        bad = _bad(case, bug)
        if any(bad.values()):
            print(f"{bug}: caught on {case.name}: {bad}")
            return
    pytest.fail(f"{bug}: no bound fails on any shape")


def test_the_emulation_of_the_span_reach_equals_the_mask():
    """FeFrameSpans' [jlo, jhi] restated above keeps every span a frame reads: the emulated table kernel equals the plain mask."""
    for case in FR.cases():
        if case.entry != "spans":
            continue
        for b in range(case.wave.shape[0]):
            N = case.wave.shape[1] if case.lens is None else case.lens[b]
            a = emu_frames(case.wave[b], N, case.spans[b], f32(1), False, True)
            c = emu_frames(case.wave[b], N, case.spans[b], f32(1), False, False)
            assert np.array_equal(a, c), (case.name, b)


def test_coverage_of_frame_and_span_situations():
    """0, 1, 2, 3+ and 16 spans in one frame's reach through the table kernels; no, head, tail and double reflection."""
    cov = FR.coverage()
    assert {0, 1, 2, 16} <= cov["spans"] and any(3 <= n < 16 for n in cov["spans"]), cov
    assert cov["reflect"] == {"none", "head", "tail", "both"}, cov


def test_subnormal_peak_clip_is_left_unscaled_like_the_oracle():
    """The 1e-39 clip of the special batch: the reference frames are those of the unscaled clip times 0.95, as R.peak_normalize_095 leaves it."""
    case = [c for c in FR.cases() if c.name == "special-1282-norm"][0]
    x = case.wave[2]
    pk = FR.peak_ref(x, len(x), [])
    assert 0 < float(pk) < FR.TINY
    assert np.array_equal(R.peak_normalize_095(x), x * f32(0.95))
    fr = FR.frames_ref(x, len(x), [], pk, True)
    w = x.astype(np.float64)[FR.source_index(len(x), 3)] * FR.C095 * FR.hann32().astype(np.float64)
    assert np.array_equal(fr.ref[:, FR.HALF], w[:, FR.HALF]) and np.abs(fr.ref).max() > 0
