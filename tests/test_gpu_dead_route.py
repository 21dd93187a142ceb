"""The route of DESIGN.md 4.20: engine.conceal_file / find_gaps with kind, rel_threshold and held_tol, and the three new keys of
`detect:` in predict.yaml, with the tiny random model and the route shapes of tests/test_gpu_feed_route.py.

The route adds no arithmetic of its own: what conceal_file repairs is compared bit for bit with patch_file on the known gaps.  A held
dropout here keeps the frame's FIRST sample through the rest of the gap's frames, so the held run is exactly the gap's samples
(gaps.runs_to_gaps covers every frame a run touches)."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from tests import dead_ref as R
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 300, 75, 15
HELD = [(100, 10), (200, 10)]                                         # two dropouts of 200 ms
KW = dict(clip_frames=CLIP, min_context=CTX, merge_frames=1)
_FILES = {}


def _engine(voc="fp32"):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", voc, key=("patch", voc))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.int16 else torch.int32)


def _file(sr, seed=41, frames=N_REC, extra=77):
    """A recording at `sr` Hz as an fp32 and an int16 file that hold the same values, no sample zero and no two neighbours equal."""
    from speech_inpainting_amd import synth
    if (sr, seed) not in _FILES:
        n = -(-frames * sr // 50) + extra
        x16 = (synth.synth_wave(1, n, seed, sr=sr)[0] * 32767.0).to(torch.int16)
        x16[x16 == 0] = 1
        for _ in range(3):
            same = torch.nonzero(x16[1:] == x16[:-1]).reshape(-1) + 1
            x16[same] += torch.where(x16[same] > 0, -1, 1).to(torch.int16) * 2
            x16[x16 == 0] = 3
        assert int((x16[1:] == x16[:-1]).sum()) == 0 and int((x16 == 0).sum()) == 0
        _FILES[sr, seed] = (x16.to(torch.float32) / 32768.0, x16)
    return _FILES[sr, seed]


def _hold(x, gaps, sr, channel=None):
    """The gaps' samples filled with the first of them: an underrun that repeats the last sample it had."""
    out = x.clone()
    col = out if channel is None else out[:, channel]
    for s, l in G.file_spans(gaps, sr):
        col[s + 1:s + l] = col[s]
    return out


@pytest.mark.parametrize("sr,pcm,feed", [(22050, False, "recording"), (48000, True, "contexts")], ids=["fp32 22.05k", "int16 48k contexts"])
def test_held_dropouts_are_found_and_repaired(sr, pcm, feed):
    """Two 200 ms dropouts that hold a sample: kind="held" finds exactly those gaps and the result is patch_file's on them, bit for
    bit; at the defaults the same file has no gaps and comes back an exact copy."""
    eng = _engine()
    x = _hold(_file(sr)[1 if pcm else 0], HELD, sr)
    found = eng.find_gaps(x, sr, kind="held", merge_frames=1)
    assert found["gaps"] == HELD and found["skipped"] == [] and found["runs"].tolist() == [list(g) for g in G.file_spans(HELD, sr)]
    assert found["threshold"] == 0.0
    eng.ctx.profile_start(4000)
    got = eng.conceal_file(x, sr, kind="held", feed=feed, **KW)
    names = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    want = eng.patch_file(x, sr, HELD, feed=feed, clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"] == HELD and got["skipped"] == [] and got["threshold"] == 0.0
    assert "detect_dead" in names and "detect_bits" not in names and "detect_peak" not in names
    assert got["patched"].dtype == x.dtype and torch.equal(_bits(got["patched"]), _bits(want["patched"])) and torch.equal(got["labels"], want["labels"])
    for s, l in G.file_spans(HELD, sr):
        assert int((got["patched"][s + 1:s + l].cpu() != x[s]).sum()) > l // 2      # the held stretch was replaced
    eng.ctx.profile_start(200)
    none = eng.conceal_file(x, sr, feed=feed, **KW)
    prof = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    torch.cuda.synchronize()
    assert prof == {"detect_bits", "detect_carry", "detect_count", "detect_offsets", "detect_emit"}, prof      # the launches of before
    assert none["gaps"] == [] and "threshold" not in none and torch.equal(_bits(none["patched"].cpu()), _bits(x))


def test_a_mute_that_is_not_exact_zeros_is_found_relative_to_the_peak():
    """One dropout filled with +-2 LSB of noise in an int16 file: found by kind="quiet" with rel_threshold = 2.5 / the file's own peak
    (T = 2.5 int16 steps), not at threshold 0."""
    eng = _engine()
    sr, gap = 22050, [(140, 8)]
    x = _file(sr, seed=43)[1].clone()
    (s, l), = G.file_spans(gap, sr)
    x[s:s + l] = torch.tensor([-2, 1, 2, -1, 0, 2, -2], dtype=torch.int16).repeat(l // 7 + 1)[:l]
    peak = int(x.to(torch.int32).abs().max())
    rel = 2.5 / peak
    want_runs = R.dead_runs_ref(x.numpy(), R.QUIET, 0.0, rel, 0.0, 110)
    assert want_runs.tolist() == [[s, l]] and 2.0 < float(R.threshold_ref(x.numpy(), 0.0, rel)) < 3.0
    found = eng.find_gaps(x, sr, rel_threshold=rel, merge_frames=1)
    assert found["gaps"] == gap and found["runs"].tolist() == [[s, l]]
    assert np.float32(found["threshold"]).tobytes() == R.threshold_ref(x.numpy(), 0.0, rel).tobytes()
    got = eng.conceal_file(x, sr, rel_threshold=rel, **KW)
    want = eng.patch_file(x, sr, gap, clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"] == gap and torch.equal(got["patched"], want["patched"]) and int((got["patched"][s:s + l].abs() > 2).sum()) > l // 2
    none = eng.conceal_file(x, sr, threshold=0.0, **KW)
    assert none["gaps"] == [] and torch.equal(none["patched"].cpu(), x)
    assert eng.find_gaps(x, sr, kind="any", merge_frames=1)["gaps"] == []         # nor held: the noise never repeats


def test_a_held_dropout_in_one_channel_of_a_stereo_file():
    """detect="each": the dropout is repaired in the channel it is in, the other channel keeps its bytes; "joint" finds nothing."""
    eng = _engine()
    sr = 48000
    x = torch.stack([_file(sr, seed=47)[1], _file(sr, seed=53)[1]], dim=1).contiguous()
    x = _hold(x, HELD[:1], sr, channel=1)
    x[G.file_spans(HELD[:1], sr)[0][0] + 5, 0] = x[G.file_spans(HELD[:1], sr)[0][0] + 5, 1]      # the neighbouring ELEMENT holds the same value
    got = eng.conceal_file(x, sr, kind="held", feed="contexts", detect="each", **KW)
    want = eng.patch_file(x, sr, channel_gaps=[[], HELD[:1]], feed="contexts", clip_frames=CLIP, min_context=CTX)
    torch.cuda.synchronize()
    assert got["gaps"] == [[], HELD[:1]] and got["skipped"] == [[], []] and got["threshold"] == [0.0, 0.0]
    assert torch.equal(got["patched"], want["patched"]) and torch.equal(got["patched"][:, 0].cpu(), x[:, 0])
    (s, l), = G.file_spans(HELD[:1], sr)
    assert int((got["patched"][s + 1:s + l, 1].cpu() != x[s, 1]).sum()) > l // 2
    joint = eng.conceal_file(x, sr, kind="held", feed="contexts", detect="joint", **KW)
    assert joint["gaps"] == [] and torch.equal(joint["patched"].cpu(), x)


def test_predict_entry_point_with_the_three_keys(tmp_path, monkeypatch, capsys):
    """predict.py with `detect: {kind, rel_threshold, held_tol}` on a 48 kHz int16 file with two held dropouts: the expected gaps and T
    come from the numpy reference on the file itself, held_tol scaled to int16 steps and rel_threshold not; gaps.json names kind and T."""
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
    pcm_in = (synth.synth_wave(1, n, 5, sr=sr)[0].numpy() * 32767).astype(np.int16)
    held = [(25, 6), (100, 6)]
    for s, l in G.file_spans(held, sr):
        pcm_in[s + 1:s + l] = pcm_in[s]
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts}}
detect: {{kind: any, rel_threshold: 3.0e-5, held_tol: 0.00001, min_ms: 5}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    tol = 0.00001 * 32768.0                                            # 0.33 int16 steps: equal samples only
    T = R.threshold_ref(pcm_in, 0.0, 3.0e-5)
    assert 0.0 < float(T) < 1.0                                        # below one step: quiet means zero
    n_rec = -(-n * 147 // 320) // 441
    gaps, skipped = G.runs_to_gaps(R.dead_runs_ref(pcm_in, R.ANY, 0.0, 3.0e-5, tol, 240).tolist(), n, sr, n_rec, merge_frames=2)
    assert gaps == held and skipped == []
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    assert json.loads((out / "gaps.json").read_text()) == {"gaps": [list(g) for g in gaps], "skipped": [], "kind": "any", "T": float(T)}
    printed = capsys.readouterr().out
    assert f"Detection kind = any, effective threshold T = {float(T)} (int16 steps)" in printed
    assert "Detected gap 1 = frames [100, 106)" in printed and "Predicted codewords, gap 0 = frames [25, 31)" in printed
    rate, wav = wavfile.read(out / "patched.wav")
    assert rate == sr and wav.dtype == np.int16 and len(wav) == n
    keep = np.ones(n, dtype=bool)
    for p, l in gaps:
        keep[960 * p - 240:960 * (p + l) + 240] = False
        assert int((wav[960 * p + 1:960 * (p + l)] != pcm_in[960 * p]).sum()) > 480 * l
    assert np.array_equal(wav[keep], pcm_in[keep])
