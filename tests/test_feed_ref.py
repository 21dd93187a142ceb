"""CPU: the definition behind si_cut_rate (tests/feed_ref.py) -- against analytic sines, against a plain loop, against a
numpy copy of the accumulated-time resampler it stands in for, and with five seeded mistakes that each have to be caught; then the host
side of the route: the `long: {feed: ...}` key of predict.yaml, the declaration of si_cut_rate against the Python mirror and the LDS a
launch asks for at every permitted rate."""
import ctypes
import os
import re

import numpy as np
import pytest

from speech_inpainting_amd import audio
from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from speech_inpainting_amd.config import load_predict_config
from tests import feed_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [48000, 44100, 32000, 16000, 11025, 8000, 4000, 192000]

# max |y - sine| over the interior outputs of `_sine_case`, float64 y, measured on the CPU with this file's construction (DESIGN.md
# 4.17): ~1e-7 and below when up-sampling (the table's linear interpolation); when down-sampling the table step int(scale 512) is
# truncated -- 235 for 235.2 at 48 kHz, 58 for 58.8 at 192 kHz -- which scales the pass band by step / (scale 512): 4.16's pattern.
SINE_ERR = {(48000, 1000): 2.53e-4, (48000, 3000): 2.77e-4, (44100, 1000): 1.57e-8, (44100, 3000): 1.52e-8, (32000, 1000): 4.90e-4,
            (32000, 3000): 6.34e-4, (16000, 1000): 5.95e-8, (16000, 3000): 3.55e-7, (11025, 1000): 2.00e-8, (11025, 3000): 3.07e-8,
            (8000, 1000): 1.57e-7, (8000, 3000): 1.35e-6, (4000, 1000): 6.09e-7, (192000, 1000): 6.16e-3, (192000, 3000): 6.22e-3}


def _sine_case(sr, fq):
    """0.05 s + 2 (H + 8) samples of a sine of amplitude 0.5 at fq Hz and the outputs whose taps all lie inside the file."""
    H = F.reach(sr)
    P, Q = G.rate_ratio(sr)
    n_file = 2 * (H + 8) + sr // 20
    x = (0.5 * np.sin(2 * np.pi * fq * np.arange(n_file) / sr)).astype(np.float32)
    j = np.arange(F.n22(n_file, sr))
    n = j * Q // P
    return x, j[(n >= H) & (n <= n_file - H - 2)]


def _sine_error(sr, fq, mistake=None):
    x, mid = _sine_case(sr, fq)
    y, _, _ = F.samples(x, mid, sr, mistake)
    return float(np.abs(y - 0.5 * np.sin(2 * np.pi * fq * mid / 22050.0)).max())


@pytest.mark.parametrize("sr", RATES)
def test_analytic_sines(sr):
    for fq in (1000, 3000):
        if (sr, fq) not in SINE_ERR:                                   # 3 kHz is above a 4 kHz file's Nyquist
            assert sr == 4000 and fq == 3000
            continue
        err = _sine_error(sr, fq)
        print(f"   {sr} Hz, {fq} Hz sine: max error {err:.3e} (measured {SINE_ERR[sr, fq]:.3e})")
        assert err <= 2 * SINE_ERR[sr, fq], (sr, fq, err)
    assert sr < 22050 or max(SINE_ERR[sr, f] for f in (1000, 3000)) > 1e-4 or sr == 44100      # the truncated step shows when down-sampling
    assert sr > 22050 or SINE_ERR[sr, 1000] < 1e-6


# ------------------------------------------------------------------------------------------------------------ a plain loop
def _plain(x, j, sr):
    """The definition, one tap at a time in Python floats (float64, separate multiply and add)."""
    f = F.tables(sr)
    win, dwin, nwin, ntab, step, scale = f["win"], f["dwin"], f["win"].size, f["num_table"], f["step"], f["scale"]
    P, Q = G.rate_ratio(sr)
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


def _noise(n, seed, pcm=False):
    v = np.random.default_rng(seed).integers(-20000, 20001, size=n).astype(np.int16)
    return v if pcm else (v.astype(np.float32) / np.float32(32768.0))


def _plain_mismatches(sr, mistake=None):
    """How many of a few outputs -- the recording's first and last ones, integer times, the middle -- differ from the plain loop in
    float64 bits."""
    P, Q = G.rate_ratio(sr)
    n_file = 3 * F.reach(sr) + 77
    x = _noise(n_file, sr)
    N22 = F.n22(n_file, sr)
    j = sorted({0, 1, 2, P, 2 * P, N22 // 2, N22 // 2 + 1, (N22 // 2 // P) * P, N22 - 3, N22 - 2, N22 - 1} & set(range(N22)))
    y, _, _ = F.samples(x, j, sr, mistake)
    return sum(float(y[k]) != _plain(F.as_f64(x), jj, sr) for k, jj in enumerate(j))


@pytest.mark.parametrize("sr", RATES)
def test_the_vectorised_reference_is_the_plain_loop_bit_for_bit(sr):
    assert _plain_mismatches(sr) == 0


def test_int16_and_fp32_files_give_the_same_reference():
    v = _noise(700, 3, pcm=True)
    a = F.clips(v, 48000, [0, 100], 150)
    b = F.clips(v.astype(np.float32) / np.float32(32768.0), 48000, [0, 100], 150)
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and a[0].shape == (2, 150)
    assert np.array_equal(a[0][0, 100:], a[0][1, :50])                # a sample is the same in whichever clip it is cut


# ------------------------------------------------------------------------------------------------------------ the accumulated time
def _accumulated(x, sr):
    """A numpy copy of resample_sinc_kernel over the whole file: time_reg = 1 / ratio accumulated by repeated addition, n = int(time),
    frac = scale (time - n); zero at and past int(n_in ratio).  -> float64 (ceil(n_in ratio))."""
    f = audio.design_kaiser_best(sr, 22050, len(x))
    time = f["time_reg"]
    n_live = int(len(x) * f["ratio"])
    n = time.astype(np.int64)
    frac = f["scale"] * (time - n)
    y = np.zeros(f["n_out"])
    y[:n_live] = F.at_times(F.as_f64(x), n[:n_live], frac[:n_live], sr)[0]
    return y, n_live


def _accumulated_violations(sr, mistake=None):
    """0.25 s of noise: the outputs outside 2^-23 max(|a|, |b|) + S tau_j of the accumulated-time resampler's, tau_j = (j + 2) 2^-53
    (j Q / P) the accumulation's own error bound; the integer-time outputs (one in P) and those at or past int(n ratio) left out.
    -> (violations, outputs compared, outputs whose fp32 bits differ, integer-time outputs that differ, their largest difference)."""
    P, Q = G.rate_ratio(sr)
    x = _noise(sr // 4 + 1, sr + 1)
    acc, n_live = _accumulated(x, sr)
    N22 = F.n22(len(x), sr)
    assert acc.size == N22 and N22 - n_live in (0, 1)
    j = np.arange(N22)
    y, A, S = F.samples(x, j, sr, mistake)
    a, b = y.astype(np.float32).astype(np.float64), acc.astype(np.float32).astype(np.float64)
    tau = (j + 2) * 2.0 ** -53 * (j * Q / P)
    tol = 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b)) + S * tau
    keep = (j % P != 0) & (j < n_live)
    assert int((~keep[:n_live]).sum()) == -(-n_live // P)             # exactly one in P
    whole = (j % P == 0) & (j < n_live)
    d = np.abs(a - b)
    return int((d[keep] > tol[keep]).sum()), int(keep.sum()), int((d[keep] != 0).sum()), int((d[whole] != 0).sum()), float(d[whole].max())


@pytest.mark.parametrize("sr", [48000, 16000])
def test_against_the_accumulated_time_resampler(sr):
    bad, total, moved, whole_moved, whole_max = _accumulated_violations(sr)
    print(f"   {sr} Hz: {moved} of {total} outputs change fp32 bits; {whole_moved} integer-time outputs differ, by up to {whole_max:.3e}")
    assert bad == 0 and total > 3000
    assert moved <= 0.05 * total                                      # difference (a): a rounding here and there, not another signal


@pytest.mark.parametrize("sr", [44100, 11025])
def test_where_the_increment_is_exact_the_two_agree_bit_for_bit(sr):
    x = _noise((sr // 4) | 1, sr + 2)                                 # an odd count: at 44.1 kHz n P / Q is no integer
    acc, n_live = _accumulated(x, sr)
    N22 = F.n22(len(x), sr)
    y, _, _ = F.samples(x, np.arange(N22), sr)
    assert np.array_equal(y[:n_live], acc[:n_live])
    if sr == 44100:                                                   # difference (b): the last sample is interpolated, not zero
        assert N22 == n_live + 1 and acc[-1] == 0.0 and y[-1] != 0.0


def test_the_last_sample_is_interpolated_at_48k():
    x = _noise(48000 // 4 + 1, 9)
    acc, n_live = _accumulated(x, 48000)
    N22 = F.n22(len(x), 48000)
    y, A, _ = F.samples(x, [N22 - 1], 48000)
    assert N22 == n_live + 1 and acc[-1] == 0.0 and abs(y[0]) > 1e-3 and (N22 - 1) * 320 // 147 < len(x)


# ------------------------------------------------------------------------------------------------------------ seeded mistakes
def _caught(mistake):
    """Which of the three checks above object to the reference read with `mistake`."""
    found = []
    if _sine_error(48000, 3000, mistake) > 2 * SINE_ERR[48000, 3000]:
        found.append("sines")
    if _plain_mismatches(48000, mistake) > 0:
        found.append("plain loop")
    if _accumulated_violations(48000, mistake)[0] > 0:
        found.append("accumulated time")
    return found


def test_no_check_objects_to_the_definition():
    assert _caught(None) == []


@pytest.mark.parametrize("mistake", F.MISTAKES)
def test_each_seeded_mistake_is_caught(mistake):
    found = _caught(mistake)
    print(f"   {mistake}: caught by {found}")
    assert found, mistake
    if mistake in ("pq_swapped", "ratio_scaling_missing"):
        assert "sines" in found
    if mistake in ("time_fp32", "right_limit_off_by_one"):
        assert "accumulated time" in found


# ------------------------------------------------------------------------------------------------------------ the host side
def _yaml(tmp_path, extra):
    import yaml
    data = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "golden", "iea_predict.yaml")))
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_long_feed_key(tmp_path):
    assert load_predict_config(_yaml(tmp_path, "")).long_feed == "recording"
    assert load_predict_config(_yaml(tmp_path, "long: {}\n")).long_feed == "recording"
    assert load_predict_config(_yaml(tmp_path, "long: {rate: file}\n")).long_feed == "recording"                # the default is today's route
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file, feed: contexts}\n"))
    assert cfg.long_feed == "contexts" and cfg.long_rate == "file" and cfg.long == {"clip_s": 4.0, "context_s": 1.0, "batch": 32}
    cfg = load_predict_config(_yaml(tmp_path, "long: {feed: contexts, batch: 2, rate: file}\n"))              # in any order
    assert cfg.long_feed == "contexts" and cfg.long["batch"] == 2
    assert load_predict_config(_yaml(tmp_path, "long: {rate: file, feed: recording}\n")).long_feed == "recording"
    assert load_predict_config(_yaml(tmp_path, "long: {feed: recording}\n")).long_rate == 22050
    for bad in ("clips", "true", "22050", "[contexts]"):
        with pytest.raises(ValueError, match="long.feed = "):
            load_predict_config(_yaml(tmp_path, f"long: {{rate: file, feed: {bad}}}\n"))
    with pytest.raises(ValueError, match="long.feed = 'clips'"):
        load_predict_config(_yaml(tmp_path, "long: {rate: file, feed: clips}\n"))
    for text in ("long: {feed: contexts}\n", "long: {rate: 22050, feed: contexts}\n"):
        with pytest.raises(ValueError, match="needs `rate: file`"):
            load_predict_config(_yaml(tmp_path, text))
    with pytest.raises(ValueError, match=r"unknown key `feeds` in `long:` \(it takes clip_s, context_s, batch, rate, feed\)"):
        load_predict_config(_yaml(tmp_path, "long: {feeds: contexts}\n"))


def test_header_declares_the_entry_the_mirror_calls():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr)
    assert int(re.search(r"#define SI_CUT_RATE_TILE (\d+)\b", hdr).group(1)) == native.CUT_RATE_TILE
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.search(r"int si_cut_rate\((.*?)\);", code, flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "x", "is_pcm16", "n_file", "sr", "host_start", "start", "C", "L", "filt", "out", "stream"]
    assert [("*" in a) for a in args] == [True, True, False, False, False, True, True, False, False, True, True, False]
    assert "si_cut_rate" in native.EXPORTS
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert len(lib.si_cut_rate.argtypes) == len(args) and lib.si_version() == 3
        assert [t is ctypes.c_int32 for t in lib.si_cut_rate.argtypes] == [not p for p in [("*" in a) or a.startswith("si_stream_t") for a in args]]
    # the header says what the entry replaces, as its neighbours do; the Makefile builds its file
    assert re.search(r"si_cut_rate\s+<-", hdr) and "DESIGN.md 4.17" in hdr
    assert "rate_feed_kernels.hip" in open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "Makefile")).read()


def test_a_tile_s_staged_samples_fit_the_lds_at_every_permitted_rate():
    """floor((tile - 1) Q / P) + 2 + 2 H floats per workgroup: 65 taps per wing when up-sampling, 140 at 48 kHz, 565 at 192 kHz; the
    largest launch stays under the 64 KB a launch gets without asking for more, far inside the CU's 160 KB."""
    assert (F.reach(16000), F.reach(48000), F.reach(192000)) == (65, 140, 565)
    worst = 0
    for sr in list(range(4000, 192001, 25)) + [4001, 11025, 44100, 191999]:
        if sr == 22050:
            continue
        P, Q = G.rate_ratio(sr)
        scale = min(1.0, 22050.0 / sr)
        H = -(-32769 // int(scale * 512))
        worst = max(worst, (native.CUT_RATE_TILE - 1) * Q // P + 2 + 2 * H)
    assert worst == (native.CUT_RATE_TILE - 1) * 192000 // 22050 + 2 + 2 * 565 and 4 * worst <= 65536 < 160 * 1024
