"""CPU: the definition behind si_cut_pair (tests/pair_ref.py) -- against the existing definition of the 22.05 kHz row,
against the oracle's whole-file resampler, against analytic sines beside the two-step clips it replaces, on a 16 kHz file, past the file's
end, and with six seeded mistakes that each have to be caught."""
import os

import numpy as np
import pytest

from oracle import ref_cpu as O
from speech_inpainting_amd import gaps as G
from tests import feed_ref as F
from tests import pair_ref as PR

RATES = [48000, 44100, 32000, 16000, 11025, 8000, 4000, 192000]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lj001_resample.npz")
_ORACLE = {}


def _noise(n, seed, pcm=False):
    v = np.random.default_rng(seed).integers(-20000, 20001, size=n).astype(np.int16)
    return v if pcm else (v.astype(np.float32) / np.float32(32768.0))


# ------------------------------------------------------------------------------------------------------------ the 22.05 kHz row
@pytest.mark.parametrize("sr", RATES)
def test_the_22050_hz_row_is_feed_ref_bit_for_bit(sr):
    """pair_ref.samples at target 22050 against feed_ref.samples on every sample of a short file's axis, and the clips' rows against
    feed_ref.clips on starts 441 f."""
    x = _noise(3 * F.reach(sr) + 1500 * sr // 22050 + 77, sr, pcm=True)
    N22 = F.n22(x.size, sr)
    a = PR.samples(x, np.arange(N22), sr, 22050)
    b = F.samples(x, np.arange(N22), sr)
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and N22 > 1400
    frames = [N22 // 441 - 1, 0, 1]
    got = PR.clips(x, sr, frames, 441, 320)
    want = F.clips(x, sr, [441 * f for f in frames], 441)
    assert np.array_equal(got["y22"], want[0]) and np.array_equal(got["A22"], want[1])


# ------------------------------------------------------------------------------------------------------------ the oracle
def _oracle16(x, sr):
    key = (sr, x.size, float(x[:64].sum()))
    if key not in _ORACLE:
        _ORACLE[key] = O.resample_kaiser_best(F.as_f64(x), sr, 16000)
    return _ORACLE[key]


def _oracle_violations(sr, mistake=None, frames=None):
    """0.25 s of noise as clips of one frame: the 16 kHz outputs outside 2^-23 max(|a|, |b|) + S tau_j of the oracle's whole-file
    resample, tau_j = (j + 2) 2^-53 (j Q / P) the accumulated time's own error bound (4.17 (a)); the integer-time outputs (j a multiple
    of P16) and those at or past int(n ratio) are left out and reported.
    -> (violations, compared, integer-time outputs that differ, their largest difference, |last sample| of ours, of the oracle's)."""
    P, Q = G.rate_ratio16(sr)
    x = _noise(sr // 4 + 1, sr + 1)
    ref = _oracle16(x, sr)
    n_live = int(x.size * (16000.0 / sr))
    N16 = PR.n_axis(x.size, sr, 16000)
    assert ref.size == N16 and N16 - n_live in (0, 1)
    n_fr = N16 // 320
    frames = list(range(n_fr)) if frames is None else frames
    c = PR.clips(x, sr, frames, 441, 320, mistake)
    j = 320 * np.asarray(frames, dtype=np.int64)[:, None] + np.arange(320)[None, :]
    a, b = c["y16"].astype(np.float32).astype(np.float64), ref[j].astype(np.float32).astype(np.float64)
    tau = (j + 2) * 2.0 ** -53 * (j * Q / P)
    tol = 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b)) + c["S16"] * tau
    keep = (j % P != 0) & (j < n_live)
    whole = (j % P == 0) & (j < n_live)
    d = np.abs(a - b)
    last = PR.samples16(x, [N16 - 1], sr, mistake)[0][0]
    return (int((d[keep] > tol[keep]).sum()), int(keep.sum()), int((d[whole] != 0).sum()), float(d[whole].max()) if whole.any() else 0.0,
            abs(float(last)), abs(float(ref[N16 - 1])))


@pytest.mark.parametrize("sr", [48000, 44100, 24000, 11025, 8000])
def test_the_16_khz_row_against_the_oracle(sr):
    """At 48 kHz every 16 kHz sample sits at an integer time (P16 = 1): nothing falls under the bound, everything is reported."""
    bad, total, whole_moved, whole_max, last, last_ref = _oracle_violations(sr)
    print(f"   {sr} Hz -> 16 kHz: {total} outputs at non-integer times inside the bound; {whole_moved} integer-time outputs differ, by up to "
          f"{whole_max:.3e}; last sample |ours| {last:.3e}, |oracle| {last_ref:.3e}")
    assert bad == 0 and (total > 1500 if G.rate_ratio16(sr)[0] > 1 else total == 0)


# ------------------------------------------------------------------------------------------------------------ analytic sines
def _sine_errors(sr, fq):
    """One clip of 10 frames out of 0.4 s of a sine of amplitude 0.5, cut mid-file: max |y - sine| of the direct 16 kHz cut, of the
    two-step clip (the 22.05 kHz clip, fp32, resampled to 16 kHz as a file of its own) and of the reference's own load of the whole file
    (the oracle's resample_kaiser_best(file, sr, 16000), sliced) -- over the whole clip, and over its interior alone (200 samples in from
    either edge, more than the 22.05 -> 16 kHz filter's 89 taps per wing).  -> {"clip": (direct, two), "interior": (direct, two, own)}."""
    n_file = 2 * sr // 5
    x = (0.5 * np.sin(2 * np.pi * fq * np.arange(n_file) / sr)).astype(np.float32)
    f0, nf = 5, 10
    c = PR.clips(x, sr, [f0], 441 * nf, 320 * nf)
    two = O.resample_kaiser_best(c["y22"][0].astype(np.float32).astype(np.float64), 22050, 16000)
    assert two.size == 320 * nf
    j = 320 * f0 + np.arange(320 * nf)
    own = O.resample_kaiser_best(x.astype(np.float64), sr, 16000)[j]
    want = 0.5 * np.sin(2 * np.pi * fq * j / 16000.0)
    mid = slice(200, 320 * nf - 200)
    err = lambda y, where: float(np.abs(y - want)[where].max())
    return {"clip": (err(c["y16"][0], slice(None)), err(two, slice(None))), "interior": (err(c["y16"][0], mid), err(two, mid), err(own, mid))}


@pytest.mark.parametrize("sr", [48000, 44100, 32000, 11025, 8000])
def test_analytic_sines_direct_against_two_step(sr):
    """On the same clip -- every sample of it, which is what the encoder is fed -- the direct cut's error is at most the two-step clip's.
    MEASURED, float64, max |y - sine| direct / two-step at 1 kHz and at 3 kHz (DESIGN.md 4.26 holds the numbers):
        48 kHz     1.37e-3 / 1.22e-2    1.50e-3 / 3.94e-2
        44.1 kHz   1.38e-3 / 1.22e-2    1.52e-3 / 3.95e-2
        32 kHz     2.01e-8 / 1.21e-2    1.53e-8 / 3.93e-2
        11.025 kHz 9.93e-8 / 1.22e-2    6.73e-7 / 3.95e-2
        8 kHz      1.73e-8 / 1.22e-2    2.75e-8 / 3.95e-2
    The two-step clip's error sits at its edges, where it has nothing before or after it.  The clip's INTERIOR alone is printed beside
    it and NOT asserted: there the direct cut equals the reference's own load of the file to three digits at every rate, and at 48 and
    44.1 kHz that is FARTHER from the sine than the two-step clip (1.37e-3 against 5.41e-4 and 1.38e-3 against 3.03e-4 at 1 kHz) --
    resampy truncates the table step to an integer, 170 for 170.67 at 48 -> 16 kHz and 185 for 185.76 at 44.1 -> 16 kHz (0.4 %), where
    the two steps truncate 235 for 235.2 and 371 for 371.52 (0.09 % and 0.14 %): DESIGN.md 4.16's pattern.  The option is fidelity to the
    reference's second load, not to the band-limited truth."""
    got = {fq: _sine_errors(sr, fq) for fq in (1000, 3000)}
    for fq, e in got.items():
        print(f"   {sr} Hz, {fq} Hz sine: whole clip direct {e['clip'][0]:.3e}, two-step {e['clip'][1]:.3e}; interior direct {e['interior'][0]:.3e}, "
              f"two-step {e['interior'][1]:.3e}, the reference's own load of the file {e['interior'][2]:.3e}")
    for fq, e in got.items():
        assert e["clip"][0] <= e["clip"][1], (sr, fq, e)


# ------------------------------------------------------------------------------------------------------------ a 16 kHz file
def test_a_16_khz_file_reaches_the_encoder_as_it_is():
    """seg16 of the golden utterance as a 16 kHz int16 file: the direct rows are its samples, exactly; the two-step rows (cut at
    22.05 kHz, each clip resampled to 16 kHz) differ from them by an RMS above 1e-3 in the clips' interior."""
    v = np.load(GOLDEN)["seg16"]
    file = v.astype(np.float32) / np.float32(32768.0)
    nf = 30
    frames = [0, 25, v.size // 320 - nf]
    c = PR.clips(v, 16000, frames, 441 * nf, 320 * nf)
    diff = []
    for b, f in enumerate(frames):
        assert np.array_equal(c["y16"][b], file[320 * f:320 * (f + nf)].astype(np.float64))
        two = O.resample_kaiser_best(c["y22"][b].astype(np.float32).astype(np.float64), 22050, 16000)
        diff.append((two - file[320 * f:320 * (f + nf)])[200:-200])
    assert not c["A16"].any() and float(np.abs(c["y16"]).max()) > 0.1
    rms = float(np.sqrt(np.mean(np.concatenate(diff) ** 2)))
    print(f"   seg16 as a 16 kHz file: two-step clips differ from the file by RMS {rms:.3e}, max {float(np.abs(np.concatenate(diff)).max()):.3e} "
          f"(signal RMS {float(np.sqrt(np.mean(file.astype(np.float64) ** 2))):.3f}); direct clips: 0")
    assert rms > 1e-3


# ------------------------------------------------------------------------------------------------------------ past the file's end
def test_the_l16_rule_exceeds_n16_by_at_most_one():
    seen = set()
    for sr in list(range(4000, 192001, 250)) + [4001, 11025, 44100, 191999, 16000]:
        if sr == 22050:
            continue
        for n in (1, 2, 7, 320, 441, 4410, 12345, 48000, 100003, 2 ** 31 - 1 - 2048):
            d = PR.lim16(n, sr) - PR.n_axis(n, sr, 16000)
            assert d in (0, 1), (sr, n, d)
            seen.add(d)
    assert seen == {0, 1}


def _end_case():
    """A 48 kHz file whose L16 rule allows one 16 kHz sample past N16, and the whole-recording clip that reaches it."""
    for n in range(12001, 12400):
        if PR.lim16(n, 48000) == PR.n_axis(n, 48000, 16000) + 1:
            return _noise(n, 5, pcm=True), PR.n_axis(n, 48000, 22050), PR.lim16(n, 48000)
    raise AssertionError("no such length")


def test_outputs_past_the_end_are_zero():
    x, N22, L16 = _end_case()
    c = PR.clips(x, 48000, [0], N22, L16)
    N16 = PR.n_axis(x.size, 48000, 16000)
    assert L16 == N16 + 1 and c["y16"][0, -1] == 0.0 and not np.signbit(c["y16"][0, -1]) and c["y16"][0, -2] != 0.0
    y, A, _ = PR.samples16(x, [N16 - 1, N16, N16 + 5], 48000)
    assert y[0] != 0 and not y[1:].any() and not A[1:].any()
    v = _noise(100, 1, pcm=True)
    y, _, _ = PR.samples16(v, [99, 100, 101], 16000)
    assert y[0] == v[99] / 32768.0 and not y[1:].any()


# ------------------------------------------------------------------------------------------------------------ seeded mistakes
def _caught(mistake):
    """Which checks object to the reference read with `mistake`."""
    found = []
    if _oracle_violations(44100, mistake, frames=[0, 7, 11])[0] > 0:
        found.append("oracle 44.1 kHz")
    n = 3 * 16000 // 10 + 1
    x = _noise(n, 16001)
    if _oracle_violations(8000, mistake, frames=[0, 5, PR.n_axis(8000 // 4 + 1, 8000, 16000) // 320 - 1])[0] > 0:
        found.append("oracle 8 kHz")
    c = PR.clips(x, 16000, [0, 3], 441 * 4, 320 * 4, mistake)
    if not np.array_equal(c["y16"], np.stack([x[:1280], x[960:2240]]).astype(np.float64)):
        found.append("16 kHz file")
    xe, N22, L16 = _end_case()
    if PR.clips(xe, 48000, [0], N22, L16, mistake)["y16"][0, -1] != 0.0:
        found.append("past the end")
    v = _noise(3000, 9, pcm=True)
    if not np.array_equal(PR.clips(v, 48000, [0, 1], 441, 320, mistake)["y22"], F.clips(v, 48000, [0, 441], 441)[0]):
        found.append("feed_ref")
    # the recording's last sample, where the right wing is cut by the file's end: against a plain loop over the few taps left
    xs = _noise(4801, 21)
    N16 = PR.n_axis(xs.size, 48000, 16000)
    j = np.array([N16 - 3, N16 - 2])
    y = PR.samples16(xs, j, 48000, mistake)[0]
    if not np.array_equal(y, np.array([_plain16(xs, int(k), 48000) for k in j])):
        found.append("plain loop at the end")
    return found


def _plain16(x, j, sr):
    """The 16 kHz definition, one tap at a time in Python floats."""
    f = PR.tables(sr, 16000)
    win, dwin, nwin, ntab, step, scale = f["win"], f["dwin"], f["win"].size, f["num_table"], f["step"], f["scale"]
    P, Q = G.rate_ratio16(sr)
    x = F.as_f64(x)
    n, r = divmod(int(j) * Q, P)
    frac = scale * (r / P)
    acc = 0.0
    idx = frac * ntab
    off = int(idx)
    eta = idx - off
    for k in range(min(n + 1, (nwin - off) // step)):
        acc += (float(win[off + k * step]) + eta * float(dwin[off + k * step])) * float(x[n - k])
    idx = (scale - frac) * ntab
    off = int(idx)
    eta = idx - off
    for k in range(min(len(x) - n - 1, (nwin - off) // step)):
        acc += (float(win[off + k * step]) + eta * float(dwin[off + k * step])) * float(x[n + 1 + k])
    return acc


def test_no_check_objects_to_the_definition():
    assert _caught(None) == []


@pytest.mark.parametrize("mistake", PR.MISTAKES)
def test_each_seeded_mistake_is_caught(mistake):
    found = _caught(mistake)
    print(f"   {mistake}: caught by {found}")
    assert found, mistake
    want = {"filters_swapped": "oracle 44.1 kHz", "start_441": "oracle 44.1 kHz", "filter_at_16k": "16 kHz file", "past_end_not_zeroed": "past the end",
            "ratio_scaling_missing": "oracle 44.1 kHz", "right_limit_off_by_one": "plain loop at the end"}[mistake]
    assert want in found, (mistake, found)
