"""CPU: the float64 definition of the file-rate repair (tests/rate_ref.py) against an analytic sine, five seeded
mistakes that each must be caught, and the hand-checked host arithmetic of speech_inpainting_amd/gaps.py's file-axis helpers.

The reference against 0.5 sin(2 pi f t), f = 1 kHz and 3 kHz, fp32 input at 22.05 kHz, every output sample at least 400 input samples
away from the ends; the worst |y - analytic| of the float64 sum, measured with the repository's own kaiser_best tables:
    24 000, 32 000, 44 100, 48 000 Hz   1.9e-7   (the fp32 rounding of the INPUT samples through a 130-tap sum)
    11 025 Hz                           1.7e-8
    16 000 Hz                           4.7e-4   } resampy's table step truncated to an integer when down-sampling (371 for 371.5,
     8 000 Hz                           2.0e-3   } 185 for 185.8): the filter's zero crossings drift off the samples.  Inherited on purpose.
Each rate is gated at twice its figure.
"""
import numpy as np
import pytest

from speech_inpainting_amd import gaps as G
from tests import rate_ref as R

FIGURE = {24000: 1.9e-7, 32000: 1.9e-7, 44100: 1.9e-7, 48000: 1.9e-7, 11025: 1.7e-8, 16000: 4.7e-4, 8000: 2.0e-3}
N22 = 6000


def _worst(sr, mistake=None, stride=1):
    """max |reference - analytic| over both tones and every `stride`-th file sample at least 400 input samples from the ends."""
    P, Q = G.rate_ratio(sr)
    n = np.arange(N22)
    worst = 0.0
    for f in (1000.0, 3000.0):
        x = (0.5 * np.sin(2.0 * np.pi * f * n / 22050.0)).astype(np.float32)
        for i in range(-(-400 * Q // P), (N22 - 400) * Q // P, stride):
            try:
                y, _ = R.sample(x, 0, i, sr, N22, mistake=mistake)
            except IndexError:
                return float("inf")
            worst = max(worst, abs(y - 0.5 * np.sin(2.0 * np.pi * f * i / sr)))
    return worst


@pytest.mark.parametrize("sr", sorted(FIGURE))
def test_reference_reproduces_a_sine(sr):
    worst = _worst(sr)
    print(f"sr {sr}: worst |y - analytic| = {worst:.3g}, figure {FIGURE[sr]:.3g}")
    assert worst <= 2.0 * FIGURE[sr]


# eta is identically zero where every phase falls on a table entry (44 100 Hz: phases 0 and 1/2; 11 025 Hz: phase 0), and at 8 kHz the
# inherited 2.0e-3 hides it: dropping eta is shown at the rates where it exists and the gate can see it
@pytest.mark.parametrize("mistake,rates", [("pq_swapped", sorted(FIGURE)), ("time_off_by_one", sorted(FIGURE)), ("wings_swapped", sorted(FIGURE)),
                                           ("eta_dropped", [16000, 24000, 32000, 48000])])
def test_seeded_mistakes_fail_the_gate(mistake, rates):
    for sr in rates:
        worst = _worst(sr, mistake=mistake, stride=37)
        assert worst > 2.0 * FIGURE[sr], f"{mistake} at {sr} Hz passes the gate: worst {worst:.3g}"


def test_rate_ratio_and_fade_by_hand():
    assert [G.rate_ratio(sr) for sr in (8000, 11025, 16000, 44100, 48000)] == [(441, 160), (2, 1), (441, 320), (1, 2), (147, 320)]
    assert [G.file_fade(5.0, sr) for sr in (8000, 11025, 16000, 44100, 48000)] == [40, 55, 80, 220, 240]      # 55.125 -> 55, 220.5 -> 220 (round half to even)
    for sr in (3999, 192001, 0, -1):
        with pytest.raises(ValueError):
            G.rate_ratio(sr)
    assert G.rate_ratio(4000) == (441, 80) and G.rate_ratio(192000) == (147, 1280)
    assert [R.reach(sr) for sr in (8000, 16000, 22050 * 2, 48000)] == [178, 89, 65, 65]


def test_file_spans_by_hand():
    # frames [3, 5): 60 ms .. 100 ms
    want = {8000: (480, 320), 11025: (662, 441), 16000: (960, 640), 44100: (2646, 1764), 48000: (2880, 1920)}
    for sr, span in want.items():
        assert G.file_spans([(3, 2)], sr) == [span]
    # 11 025 Hz has 220.5 samples per frame: frame 1 is samples [221, 441), frame 2 [441, 662)
    assert G.file_spans([(1, 1), (2, 1)], 11025) == [(221, 220), (441, 221)]
    # a file sample belongs to the span iff its 22.05 kHz position lies in [441 p, 441 (p + l))
    for sr in want:
        P, Q = G.rate_ratio(sr)
        for p, l in ((0, 1), (1, 1), (7, 3), (101, 2)):
            (s, n), = G.file_spans([(p, l)], sr)
            inside = [i for i in range(max(s - 3, 0), s + n + 3) if 441 * p * Q <= i * P < 441 * (p + l) * Q]
            assert inside == list(range(s, s + n))


def test_file_lim_is_a_ceiling():
    want = {8000: 364, 11025: 501, 16000: 727, 44100: 2002, 48000: 2180}          # ceil(1001 Q / P)
    floored = {8000: 363, 11025: 500, 16000: 726, 44100: 2002, 48000: 2179}
    for sr, lim in want.items():
        assert G.file_lim(1001, sr) == lim
        assert G.file_lim(1001, sr, n_file=300) == 300
        P, Q = G.rate_ratio(sr)
        # the property a floored limit breaks: file sample lim - 1 still sits in front of 22.05 kHz sample 1001, sample lim does not
        ok = lambda v: (v - 1) * P < 1001 * Q <= v * P
        assert ok(lim)
        assert floored[sr] == 1001 * Q // P and (ok(floored[sr]) == (floored[sr] == lim))
    assert sum(floored[sr] != want[sr] for sr in want) == 4


def test_regions_and_reach_by_hand():
    assert G.file_regions([(2880, 1920), (9000, 100), (20, 50)], [10000, 9000, 60], 240) == [(2640, 5040), None, (0, 60)]
    # 48 kHz: floor(2640 * 147 / 320) = 1212, floor(5039 * 147 / 320) = 2314; H = 65
    assert G.reach_regions22([(2640, 5040), None], 48000, 65, 0, 10 ** 6) == [(1147, 2380), None]
    assert G.reach_regions22([(2640, 5040)], 48000, 65, 1200, 2300) == [(1200, 2300)]
    # 8 kHz: floor(440 * 441 / 160) = 1212, floor(839 * 441 / 160) = 2312; H = 178
    assert G.reach_regions22([(440, 840)], 8000, 178, 0, 10 ** 6) == [(1034, 2491)]
    # every tap of every sample of the region lies inside the mapped range, and its two ends are reached
    for sr in (8000, 11025, 16000, 44100, 48000):
        P, Q = G.rate_ratio(sr)
        H = R.reach(sr)
        a, b = 1000, 1300
        (lo, hi), = G.reach_regions22([(a, b)], sr, H, 0, 10 ** 9)
        ns = [i * P // Q for i in range(a, b)]
        assert lo <= min(ns) - (H - 1) and max(ns) + H < hi and lo == min(ns) - H and hi == max(ns) + 1 + H


def test_reference_refuses_a_tap_outside_the_row():
    x = np.zeros(1000, dtype=np.float32)
    R.sample(x, 500, 48000 * 1000 // 22050, 48000, 10 ** 6)                      # n = 1000 - ... well inside [500, 1500)
    with pytest.raises(IndexError):
        R.sample(x, 500, 48000 * 530 // 22050, 48000, 10 ** 6)                   # the left wing reaches below sample 500
    # ... unless those taps lie before recording sample 0 or at / past lim22, where they read as zero
    y0, _ = R.sample(np.ones(200, dtype=np.float32), 0, 10, 48000, 200)
    y1, _ = R.sample(np.ones(200, dtype=np.float32), 0, 10, 48000, 30)               # n = 4: the right wing reaches sample 69
    assert np.isfinite(y0) and np.isfinite(y1) and y0 != y1


def test_weights_follow_the_region_rule():
    ramp = G.fade_ramp(7)
    w, owner = R.weights([(100, 10, 0, 10 ** 6), (120, 5, 0, 123)], 7, 200)
    assert np.array_equal(w[93:100], ramp) and np.all(w[100:110] == 1) and np.array_equal(w[110:113], ramp[::-1][:3])
    # the ramps of the two spans overlap in [113, 117): the maximum wins, and its span owns the sample
    assert np.array_equal(w[113:117], np.maximum(ramp[::-1][3:7], ramp[0:4])) and np.all(w[120:123] == 1)
    assert np.all(w[123:] == 0) and np.all(owner[123:] == -1) and np.all(w[:93] == 0)
    assert list(owner[113:117]) == [0 if ramp[::-1][3 + j] >= ramp[j] else 1 for j in range(4)]
