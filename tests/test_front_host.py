"""The request front's host rules, no GPU: audio.resampled_len is librosa 0.9.1's length rule and the resampler's,
and the time-register table of a shorter clip is a bitwise prefix of a longer clip's (what lets the engine keep one per rate pair)."""
import math

import numpy as np
import pytest

from speech_inpainting_amd import audio
from speech_inpainting_amd.arch import mel_frames

RATES_IN = (7350, 8000, 11025, 16000, 22050, 24000, 32000, 32075, 37800, 44100, 47999, 48000, 75600, 96000)
RATES_OUT = (22050, 16000)
N_MAX = 200000
PAIRS = ((44100, 16000), (48000, 22050), (8000, 22050), (37800, 22050), (22050, 16000))


def _librosa_len(n, orig_sr, target_sr):
    """librosa/core/audio.py (0.9.1), resample: `ratio = float(target_sr) / orig_sr`, `n_samples = int(np.ceil(y.shape[axis] * ratio))`;
    at equal rates it returns y itself."""
    if orig_sr == target_sr:
        return n
    ratio = float(target_sr) / orig_sr
    return int(np.ceil(n * ratio))


@pytest.mark.parametrize("sr_out", RATES_OUT)
def test_resampled_len_is_librosas_rule(sr_out):
    n = np.arange(1, N_MAX + 1, dtype=np.int64)
    for sr_in in RATES_IN:
        got = np.fromiter((audio.resampled_len(int(v), sr_in, sr_out) for v in n), dtype=np.int64, count=n.size)
        want = n if sr_in == sr_out else np.ceil(n * (float(sr_out) / sr_in)).astype(np.int64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (sr_in, sr_out, bad.size, n[bad[:5]].tolist())
        for v in (1, 2, 107, 108, 147, 27900, 49164, N_MAX):                         # the scalar spelling of the same expression
            assert audio.resampled_len(v, sr_in, sr_out) == _librosa_len(v, sr_in, sr_out), (sr_in, sr_out, v)
        assert isinstance(audio.resampled_len(5, sr_in, sr_out), int)


@pytest.mark.parametrize("sr_out", RATES_OUT)
def test_resampled_len_is_the_resamplers_n_out(sr_out):
    rng = np.random.default_rng(11)
    for sr_in in RATES_IN:
        if sr_in == sr_out:
            continue
        for n in [1, 2, 108, 147, 27900, 25632, 49164] + [int(v) for v in rng.integers(1, 2000000, 6)]:
            f = audio.design_kaiser_best(sr_in, sr_out, n)
            assert f["n_out"] == audio.resampled_len(n, sr_in, sr_out) == f["time_reg"].size, (sr_in, sr_out, n)


def test_the_product_first_rule_disagrees_so_this_file_is_not_blind():
    """`ceil(n * float(sr) / sr_in)` -- the front's former spelling -- is another function: it rounds n * sr before the division."""
    first = {}
    for sr_in, sr_out in ((37800, 22050), (7350, 16000)):
        differ = [n for n in range(1, N_MAX + 1) if int(math.ceil(n * float(sr_out) / sr_in)) != audio.resampled_len(n, sr_in, sr_out)]
        print(f"   {sr_in} -> {sr_out}: {len(differ)} of {N_MAX} lengths differ, first {differ[:3]}")
        assert len(differ) > 0
        first[sr_in] = differ[:3]
        for n in differ[:50]:                                                       # the old rule is the shorter one: the exact quotient is an integer
            assert int(math.ceil(n * float(sr_out) / sr_in)) == audio.resampled_len(n, sr_in, sr_out) - 1 and (n * sr_out) % sr_in == 0
    assert first == {37800: [108, 204, 216], 7350: [147, 294, 441]}
    # the clips the GPU tests send at 37800 Hz: one sample fewer is one mel frame fewer (27900, 25632) or only a shorter patch (4916x)
    old = lambda n: int(math.ceil(n * 22050.0 / 37800))
    for n in (27900, 25632, 24876, 26388, 27144):
        assert mel_frames(old(n)) + 1 == mel_frames(audio.resampled_len(n, 37800, 22050)), n
    for n in (49164, 49176, 49188):
        assert old(n) + 1 == audio.resampled_len(n, 37800, 22050), n


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_time_registers_of_a_shorter_clip_are_a_bitwise_prefix(sr_in, sr_out):
    long = audio.design_kaiser_best(sr_in, sr_out, 400000)
    assert long["time_reg"].dtype == np.float64 and long["time_reg"].size == long["n_out"]
    for n in (1, 2, 147, 1000, 26460, 99999):
        f = audio.design_kaiser_best(sr_in, sr_out, n)
        assert f["time_reg"].dtype == np.float64 and f["time_reg"].size == f["n_out"] <= long["n_out"]
        assert f["time_reg"].tobytes() == long["time_reg"][:f["n_out"]].tobytes(), (sr_in, sr_out, n)
        assert audio.time_registers(sr_in, sr_out, f["n_out"]).tobytes() == f["time_reg"].tobytes()
        for k in ("win", "dwin"):                                                   # and the filter itself does not depend on the length
            assert f[k].tobytes() == long[k].tobytes(), k
        assert all(f[k] == long[k] for k in ("num_table", "step", "scale", "ratio"))
