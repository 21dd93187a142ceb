"""The route of DESIGN.md 4.25: engine.conceal_file / conceal_recording / find_gaps with kind="level" and win_ms, and `detect: {kind:
level, win_ms: ...}` in predict.yaml, with the tiny random model and the recordings of tests/test_gpu_dead_route.py.

A dropout here is a NOISE FLOOR: the gap's samples replaced by seeded rint(N(0, 12)) int16 steps.  Each builder first asserts with the
CPU references that the windowed level at T = 16 finds exactly the planted samples and that the sample-wise detector at the same
threshold finds nothing.  The route adds no arithmetic of its own: what it repairs is compared bit for bit with patch_file /
patch_recording on the known gaps."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from tests import dead_ref as R
from tests import level_ref as L
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 300, 75, 15
GAPS = [(100, 10), (200, 10)]                                         # two dropouts of 200 ms
KW = dict(clip_frames=CLIP, min_context=CTX, merge_frames=1)
SIGMA, T16 = 12.0, 16.0                                               # int16 steps
_FILES = {}


def _engine(voc="fp32"):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", voc, key=("patch", voc))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.int16 else torch.int32)


def _file(sr, seed, gaps, frames=N_REC, extra=77):
    """A recording at `sr` Hz as int16 (tests/test_gpu_dead_route.py's), the gaps' file samples filled with the noise floor.  Asserted
    on the CPU: the level detector at T16 finds exactly those samples, the sample-wise one nothing, and the clean file holds neither."""
    from speech_inpainting_amd import synth
    key = (sr, seed, tuple(gaps))
    if key not in _FILES:
        n = -(-frames * sr // 50) + extra
        clean = (synth.synth_wave(1, n, seed, sr=sr)[0] * 32767.0).to(torch.int16).numpy()
        x = clean.copy()
        rng = np.random.default_rng(seed)
        spans = G.file_spans(gaps, sr)
        for s, l in spans:
            x[s:s + l] = np.rint(rng.normal(0.0, SIGMA, l))
        h, min_len = G.level_half(2.0, sr), int(round(5.0 * sr / 1000.0))
        assert L.level_runs_ref(x, h, T16, 0.0, min_len).tolist() == [list(g) for g in spans]
        assert L.level_runs_ref(clean, h, T16, 0.0, min_len).tolist() == []
        assert R.dead_runs_ref(x, R.QUIET, T16, 0.0, 0.0, min_len).tolist() == []
        _FILES[key] = torch.from_numpy(x)
    return _FILES[key]


def test_noise_floor_dropouts_in_a_48_khz_int16_file():
    """conceal_file(kind="level", threshold=16, win_ms=2), feed="contexts": exactly the planted gaps, patch_file's bytes on them; the
    sample-wise kind at the same threshold finds none and returns an exact copy."""
    eng = _engine()
    sr = 48000
    x = _file(sr, 47, GAPS)
    found = eng.find_gaps(x, sr, T16, kind="level", win_ms=2.0, merge_frames=1)
    assert found["gaps"] == GAPS and found["skipped"] == [] and found["runs"].tolist() == [list(g) for g in G.file_spans(GAPS, sr)]
    assert found["threshold"] == T16
    eng.ctx.profile_start(4000)
    got = eng.conceal_file(x, sr, T16, kind="level", win_ms=2.0, feed="contexts", **KW)
    names = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    want = eng.patch_file(x, sr, GAPS, feed="contexts", clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"] == GAPS and got["skipped"] == [] and got["threshold"] == T16
    assert "detect_dead" in names and not names & {"detect_bits", "detect_bits_ch", "detect_peak"}    # the level kernel's family is detect_dead
    assert got["patched"].dtype == torch.int16 and torch.equal(_bits(got["patched"]), _bits(want["patched"])) and torch.equal(got["labels"], want["labels"])
    for s, l in G.file_spans(GAPS, sr):
        assert int((got["patched"][s:s + l].cpu().to(torch.int32).abs() > 4 * SIGMA).sum()) > l // 4      # the noise floor was replaced
    eng.ctx.profile_start(200)
    none = eng.conceal_file(x, sr, T16, kind="quiet", feed="contexts", **KW)
    prof = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    torch.cuda.synchronize()
    assert prof == {"detect_bits", "detect_carry", "detect_count", "detect_offsets", "detect_emit"}, prof      # the launches of before
    assert none["gaps"] == [] and "threshold" not in none and torch.equal(_bits(none["patched"].cpu()), _bits(x))
    with pytest.raises(ValueError, match="held_tol = 1.0 with kind = 'level'"):
        eng.conceal_file(x, sr, T16, kind="level", held_tol=1.0, **KW)
    with pytest.raises(ValueError, match="at most win_ms = 42.666 at this rate"):
        eng.conceal_file(x, sr, T16, kind="level", win_ms=50.0, **KW)


def test_noise_floor_dropouts_in_a_22_khz_fp32_recording():
    """conceal_recording on the same values as fp32 (multiples of 2^-15: every window's energy is a float64), threshold in full scale;
    relative to the peak as well."""
    eng = _engine()
    sr = 22050
    x16 = _file(sr, 43, GAPS)
    x = x16.to(torch.float32) / 32768.0
    got = eng.conceal_recording(x, threshold=T16 / 32768.0, kind="level", win_ms=2.0, **KW)
    want = eng.patch_recording(x, GAPS, clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"] == GAPS and got["skipped"] == [] and got["threshold"] == T16 / 32768.0
    assert torch.equal(_bits(got["patched"]), _bits(want["patched"]))
    none = eng.conceal_recording(x, threshold=T16 / 32768.0, **KW)
    assert none["gaps"] == [] and torch.equal(_bits(none["patched"].cpu()), _bits(x))
    peak = int(x16.to(torch.int32).abs().max())
    rel = T16 / peak
    T = R.threshold_ref(x.numpy(), 0.0, rel)
    assert L.level_runs_ref(x16.numpy(), 22, float(R.threshold_ref(x16.numpy(), 0.0, rel)), 0.0, 110).tolist() == [list(g) for g in G.file_spans(GAPS, sr)]
    found = eng.find_gaps(x16, sr, kind="level", rel_threshold=rel, merge_frames=1)
    assert found["gaps"] == GAPS and np.float32(found["threshold"]).tobytes() == R.threshold_ref(x16.numpy(), 0.0, rel).tobytes()
    assert 15.0 < found["threshold"] < 17.0 and 15.0 / 32768 < float(T) < 17.0 / 32768


def test_a_noise_floor_dropout_in_one_channel_of_a_stereo_file():
    """detect="each": the dropout is repaired in the channel it is in, the other channel keeps its bytes; "joint" finds nothing."""
    eng = _engine()
    sr = 48000
    x = torch.stack([_file(sr, 53, []), _file(sr, 47, GAPS[:1])], dim=1).contiguous()
    got = eng.conceal_file(x, sr, T16, kind="level", feed="contexts", detect="each", **KW)
    want = eng.patch_file(x, sr, channel_gaps=[[], GAPS[:1]], feed="contexts", clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"] == [[], GAPS[:1]] and got["skipped"] == [[], []] and got["threshold"] == [T16, T16]
    assert torch.equal(got["patched"], want["patched"]) and torch.equal(got["patched"][:, 0].cpu(), x[:, 0])
    (s, l), = G.file_spans(GAPS[:1], sr)
    assert int((got["patched"][s:s + l, 1].cpu().to(torch.int32).abs() > 4 * SIGMA).sum()) > l // 4
    joint = eng.conceal_file(x, sr, T16, kind="level", feed="contexts", detect="joint", **KW)
    assert joint["gaps"] == [] and joint["threshold"] == T16 and torch.equal(joint["patched"].cpu(), x)


def test_predict_entry_point_with_kind_level(tmp_path, monkeypatch, capsys):
    """predict.py with `detect: {kind: level, win_ms: 2}` on a 48 kHz int16 file with two noise-floor dropouts: the expected gaps come
    from the reference on the file itself, the threshold scaled to int16 steps and win_ms not; gaps.json names kind, T and win_ms."""
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
    pcm_in = _file(sr, 47, planted, frames=150).numpy()
    assert len(pcm_in) == n
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts}}
detect: {{kind: level, win_ms: 2, threshold: {T16 / 32768.0!r}, min_ms: 5}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    n_rec = -(-n * 147 // 320) // 441
    gaps, skipped = G.runs_to_gaps(L.level_runs_ref(pcm_in, 48, T16, 0.0, 240).tolist(), n, sr, n_rec, merge_frames=2)
    assert gaps == planted and skipped == []
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    assert json.loads((out / "gaps.json").read_text()) == {"gaps": [list(g) for g in gaps], "skipped": [], "kind": "level", "T": T16, "win_ms": 2.0}
    printed = capsys.readouterr().out
    assert f"Detection kind = level, effective threshold T = {T16} (int16 steps), window win_ms = 2.0" in printed
    assert "Detected gap 1 = frames [100, 106)" in printed and "Predicted codewords, gap 0 = frames [25, 31)" in printed
    rate, wav = wavfile.read(out / "patched.wav")
    assert rate == sr and wav.dtype == np.int16 and len(wav) == n
    keep = np.ones(n, dtype=bool)
    for p, l in gaps:
        keep[960 * p - 240:960 * (p + l) + 240] = False
        assert int((np.abs(wav[960 * p:960 * (p + l)].astype(np.int32)) > 4 * SIGMA).sum()) > 240 * l
    assert np.array_equal(wav[keep], pcm_in[keep])
