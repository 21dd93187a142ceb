"""The route of DESIGN.md 4.28: engine.conceal_file / conceal_recording / find_gaps with kind="burst" and win_ms, and `detect: {kind:
burst, threshold: ..., win_ms: ...}` in predict.yaml, with the tiny random model and the recordings of tests/test_gpu_level_route.py.

The damage here is LOUDER than the recording: one gap's samples replaced by seeded uniformly random values over the whole range, the
other's byte-swapped (24-bit: shifted by one byte).  Each builder first asserts with the CPU references that the second-difference
level at 1.15 of full scale over 4 ms finds two runs, each containing its block, that the clean file has none, and that the quiet and
level detectors at their documented settings find neither block.  The route adds no arithmetic of its own: what it repairs is compared
bit for bit with patch_file / patch_recording on the gaps it reports."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from tests import burst_ref as B
from tests import dead_ref as R
from tests import level_ref as L
from tests import s24_ref as S
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 300, 75, 15
GAPS = [(100, 10), (200, 10)]                                         # two blocks of 200 ms
KW = dict(clip_frames=CLIP, min_context=CTX, merge_frames=1)
WIN_MS = 4.0
T16, T24, TF = 1.15 * 32768, 1.15 * 8388608, 1.15                     # as the caller gives them; the C ABI takes their fp32
_FILES = {}


def _engine(voc="fp32"):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", voc, key=("patch", voc))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.int16 else torch.int32)


def _covers(gaps, blocks, sr):
    """Every block [s, s + l) of file samples lies inside one gap's frames."""
    return all(any(p * sr <= s * 50 and (p + k) * sr >= (s + l) * 50 for p, k in gaps) for s, l in blocks)


def _touching(gaps, blocks, sr):
    return [g for g in gaps for s, l in blocks if g[0] * sr < (s + l) * 50 and (g[0] + g[1]) * sr > s * 50]


def _file(sr, seed, gaps, frames=N_REC, extra=77, s24=False):
    """A recording at `sr` Hz as int16 (tests/test_gpu_level_route.py's), or as 24-bit values, with the gaps' file samples corrupted:
    even gaps by seeded random values, odd ones by a byte swap (24-bit: the stretch's bytes shifted by one).  -> (x, clean, blocks)."""
    from speech_inpainting_amd import synth
    key = (sr, seed, tuple(gaps), frames, s24)
    if key not in _FILES:
        n = -(-frames * sr // 50) + extra
        clean = (synth.synth_wave(1, n, seed, sr=sr)[0] * 32767.0).to(torch.int16).numpy()
        rng = np.random.default_rng(seed)
        blocks = G.file_spans(gaps, sr)
        if s24:
            clean = clean.astype(np.int32) * 256 + rng.integers(0, 256, n).astype(np.int32)
            x = clean.copy()
            for k, (s, l) in enumerate(blocks):
                if k % 2 == 0:
                    x[s:s + l] = rng.integers(S.LO, S.HI + 1, l)
                else:
                    raw = S.pack(x[s:s + l + 1]).reshape(-1)
                    x[s:s + l] = S.unpack(raw[1:3 * l + 1].reshape(l, 3))
            T, dt = np.float32(T24), B.S24
        else:
            x = clean.copy()
            for k, (s, l) in enumerate(blocks):
                x[s:s + l] = rng.integers(-32768, 32768, l).astype(np.int16) if k % 2 == 0 else x[s:s + l].byteswap()
            T, dt = np.float32(T16), np.int16
        h, min_len = G.level_half(WIN_MS, sr), int(round(5.0 * sr / 1000.0))
        rows = B.burst_runs_ref(x.astype(dt), h, float(T), 0.0, min_len).tolist()
        assert len(rows) == len(blocks) and all(a <= s and a + k >= s + l for (a, k), (s, l) in zip(rows, blocks)), (rows, blocks)
        assert B.burst_runs_ref(clean.astype(dt), h, float(T), 0.0, min_len).tolist() == []
        x16 = x if not s24 else (x >> 8).astype(np.int16)              # the quiet and level references on the int16 image
        touch = lambda rr: [r for r in rr.tolist() for s, l in blocks if r[0] < s + l and r[0] + r[1] > s]
        assert touch(R.dead_runs_ref(x16, R.QUIET, 0.0, 0.0, 0.0, min_len)) == []
        assert touch(L.level_runs_ref(x16, G.level_half(2.0, sr), 16.0, 0.0, min_len)) == []
        _FILES[key] = (x, clean, blocks, rows)
    return _FILES[key]


def test_corrupted_blocks_in_a_48_khz_int16_file():
    """conceal_file(kind="burst", threshold=1.15 * 32768, win_ms=4), feed="contexts": the reference's runs, gaps that cover both blocks,
    patch_file's bytes on them; kind quiet and kind level at their documented settings find neither block."""
    eng = _engine()
    sr = 48000
    x, clean, blocks, rows = _file(sr, 47, GAPS)
    x = torch.from_numpy(x)
    found = eng.find_gaps(x, sr, T16, kind="burst", win_ms=WIN_MS, merge_frames=1)
    assert found["runs"].tolist() == rows and found["skipped"] == [] and len(found["gaps"]) == 2 and _covers(found["gaps"], blocks, sr)
    assert found["threshold"] == float(np.float32(T16))
    eng.ctx.profile_start(4000)
    got = eng.conceal_file(x, sr, T16, kind="burst", win_ms=WIN_MS, feed="contexts", **KW)
    names = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    want = eng.patch_file(x, sr, got["gaps"], feed="contexts", clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"] == found["gaps"] and got["skipped"] == [] and got["threshold"] == float(np.float32(T16))
    assert "detect_dead" in names and not names & {"detect_bits", "detect_bits_ch", "detect_peak"}    # the burst kernel's family is detect_dead
    assert got["patched"].dtype == torch.int16 and torch.equal(_bits(got["patched"]), _bits(want["patched"])) and torch.equal(got["labels"], want["labels"])
    for s, l in blocks:                                                 # the garbage was replaced
        assert int((got["patched"][s:s + l].cpu() != x[s:s + l]).sum()) > l // 2
    for kind, thr, kw in (("quiet", 0.0, {}), ("level", 16.0, {"win_ms": 2.0})):
        none = eng.conceal_file(x, sr, thr, kind=kind, feed="contexts", **kw, **KW)
        torch.cuda.synchronize()
        assert _touching(none["gaps"], blocks, sr) == [], (kind, none["gaps"])
        for s, l in blocks:
            assert torch.equal(none["patched"][s:s + l].cpu(), x[s:s + l])
    with pytest.raises(ValueError, match="held_tol = 1.0 with kind = 'burst'"):
        eng.conceal_file(x, sr, T16, kind="burst", held_tol=1.0, **KW)
    with pytest.raises(ValueError, match="at most win_ms = 42.666 at this rate"):
        eng.conceal_file(x, sr, T16, kind="burst", win_ms=50.0, **KW)
    with pytest.raises(ValueError, match=r"is T = 0: every window would be hot.*1\.15 of full scale.*win_ms = 4\.0"):
        eng.conceal_file(x, sr, kind="burst", **KW)


def test_corrupted_blocks_in_a_22_khz_fp32_recording():
    """conceal_recording on such a file as fp32 (multiples of 2^-15: every window's energy is a float64), threshold in full scale;
    relative to the peak as well."""
    eng = _engine()
    sr = 22050
    x16, clean, blocks, rows = _file(sr, 43, GAPS)
    x = torch.from_numpy(x16).to(torch.float32) / 32768.0
    assert B.burst_runs_ref(x.numpy(), 44, TF, 0.0, 110).tolist() == rows
    got = eng.conceal_recording(x, threshold=TF, kind="burst", win_ms=WIN_MS, **KW)
    want = eng.patch_recording(x, got["gaps"], clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert len(got["gaps"]) == 2 and _covers(got["gaps"], blocks, sr) and got["skipped"] == [] and got["threshold"] == float(np.float32(TF))
    assert torch.equal(_bits(got["patched"]), _bits(want["patched"]))
    for kind, thr, kw in (("quiet", 0.0, {}), ("level", 16.0 / 32768, {"win_ms": 2.0})):
        none = eng.conceal_recording(x, threshold=thr, kind=kind, **kw, **KW)
        assert _touching(none["gaps"], blocks, sr) == [], (kind, none["gaps"])
    rel = 1.15                                                          # of the file's own peak, which the garbage sets: 32768 / 32768
    found = eng.find_gaps(x, sr, kind="burst", rel_threshold=rel, win_ms=WIN_MS, merge_frames=1)
    assert np.float32(found["threshold"]).tobytes() == R.threshold_ref(x.numpy(), 0.0, rel).tobytes()
    assert found["runs"].tolist() == B.burst_runs_ref(x.numpy(), 44, 0.0, rel, 110).tolist() and _covers(found["gaps"], blocks, sr)


def test_a_corrupted_block_in_one_channel_of_a_stereo_file():
    """detect="each": the block is repaired in the channel it is in, the other channel keeps its bytes; "joint" finds nothing."""
    eng = _engine()
    sr = 48000
    left = torch.from_numpy(_file(sr, 53, [])[0])
    right, _, blocks, rows = _file(sr, 47, GAPS[:1])
    x = torch.stack([left, torch.from_numpy(right)], dim=1).contiguous()
    got = eng.conceal_file(x, sr, T16, kind="burst", win_ms=WIN_MS, feed="contexts", detect="each", **KW)
    want = eng.patch_file(x, sr, channel_gaps=got["gaps"], feed="contexts", clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"][0] == [] and len(got["gaps"][1]) == 1 and _covers(got["gaps"][1], blocks, sr) and got["skipped"] == [[], []]
    assert got["threshold"] == [float(np.float32(T16))] * 2
    assert torch.equal(got["patched"], want["patched"]) and torch.equal(got["patched"][:, 0].cpu(), x[:, 0])
    (s, l), = blocks
    assert not torch.equal(got["patched"][s:s + l, 1].cpu(), x[s:s + l, 1])
    joint = eng.conceal_file(x, sr, T16, kind="burst", win_ms=WIN_MS, feed="contexts", detect="joint", **KW)
    assert joint["gaps"] == [] and joint["threshold"] == float(np.float32(T16)) and torch.equal(joint["patched"].cpu(), x)


def test_corrupted_blocks_in_a_packed_24_bit_file():
    """A 24-bit file as its packed bytes: one block of random 24-bit values, one whose bytes are shifted by one; the threshold counts
    24-bit steps; the repaired file comes back packed."""
    eng = _engine()
    sr = 48000
    v, clean, blocks, rows = _file(sr, 47, GAPS, s24=True)
    x = torch.from_numpy(S.pack(v))
    found = eng.find_gaps(x, sr, T24, kind="burst", win_ms=WIN_MS, merge_frames=1)
    assert found["runs"].tolist() == rows and found["threshold"] == float(np.float32(T24)) and _covers(found["gaps"], blocks, sr)
    got = eng.conceal_file(x, sr, T24, kind="burst", win_ms=WIN_MS, feed="contexts", **KW)
    want = eng.patch_file(x, sr, got["gaps"], feed="contexts", clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"] == found["gaps"] and got["skipped"] == [] and got["patched"].dtype == torch.uint8 and got["patched"].shape == x.shape
    assert torch.equal(got["patched"], want["patched"])
    for s, l in blocks:
        assert not torch.equal(got["patched"][s:s + l].cpu(), x[s:s + l])
    for kind, thr, kw in (("quiet", 0.0, {}), ("level", 16.0 * 256, {"win_ms": 2.0})):
        none = eng.conceal_file(x, sr, thr, kind=kind, feed="contexts", **kw, **KW)
        assert _touching(none["gaps"], blocks, sr) == [], (kind, none["gaps"])


def test_predict_entry_point_with_kind_burst(tmp_path, monkeypatch, capsys):
    """predict.py with `detect: {kind: burst, threshold: 1.15, win_ms: 4}` on a 48 kHz int16 file with two corrupted blocks: the expected
    gaps come from the reference on the file itself, the threshold scaled to int16 steps and win_ms not; gaps.json names kind, T and
    win_ms.  With the threshold left at 0 the run ends with the engine's refusal."""
    import joblib
    from scipy.io import wavfile
    from sklearn.cluster import MiniBatchKMeans
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.predict import main

    harch, varch = HubertArch.base(), VocoderArch.v1()
    hsd, gsd, cb = synth.synth_hubert_state(harch, pos_conv_style="legacy"), synth.synth_generator_state(varch), synth.synth_codebook(100)
    (tmp_path / "trained_models").mkdir()
    torch.save(dict(hsd), tmp_path / "trained_models" / "save_checkpoint.pt")
    (tmp_path / "hifi_gan" / "LJ_V1").mkdir(parents=True)
    torch.save({"generator": dict(gsd)}, tmp_path / "hifi_gan" / "LJ_V1" / "generator_v1")
    (tmp_path / "hifi_gan" / "LJ_V1" / "config.json").write_text(json.dumps(dict(
        resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
        resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=80, sampling_rate=22050, seed=1234)))
    kdir = tmp_path / "kmeans" / "km_model_100"
    kdir.mkdir(parents=True)
    km = MiniBatchKMeans(n_clusters=100)
    km.cluster_centers_ = cb.numpy()
    joblib.dump(km, kdir / "model.km")
    sr = 48000
    n = 3 * sr + 77
    planted = [(25, 6), (100, 6)]
    pcm_in, _, blocks, rows = _file(sr, 47, planted, frames=150)
    assert len(pcm_in) == n
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, pcm_in)
    text = f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts}}
detect: {{kind: burst, win_ms: 4, threshold: THRESHOLD, min_ms: 5}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
"""
    (tmp_path / "predict.yaml").write_text(text.replace("THRESHOLD", "1.15"))
    n_rec = -(-n * 147 // 320) // 441
    gaps, skipped = G.runs_to_gaps(rows, n, sr, n_rec, merge_frames=2)
    assert len(gaps) == 2 and skipped == [] and _covers(gaps, blocks, sr)
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    T = float(np.float32(T16))
    assert json.loads((out / "gaps.json").read_text()) == {"gaps": [list(g) for g in gaps], "skipped": [], "kind": "burst", "T": T, "win_ms": 4.0}
    printed = capsys.readouterr().out
    assert f"Detection kind = burst, effective threshold T = {T} (int16 steps), window win_ms = 4.0" in printed
    assert f"Detected gap 1 = frames [{gaps[1][0]}, {gaps[1][0] + gaps[1][1]})" in printed
    rate, wav = wavfile.read(out / "patched.wav")
    assert rate == sr and wav.dtype == np.int16 and len(wav) == n
    keep = np.ones(n, dtype=bool)
    for p, l in gaps:
        keep[960 * p - 240:960 * (p + l) + 240] = False
    assert np.array_equal(wav[keep], pcm_in[keep])
    for s, l in blocks:
        assert int((wav[s:s + l] != pcm_in[s:s + l]).sum()) > l // 2    # the garbage was replaced
    (tmp_path / "predict.yaml").write_text(text.replace("THRESHOLD", "0"))
    with pytest.raises(ValueError, match=r"is T = 0: every window would be hot.*1\.15 of full scale.*win_ms = 4\.0"):
        main([])
