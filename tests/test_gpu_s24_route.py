"""The route of DESIGN.md 4.27: a packed 24-bit file through engine.conceal_file / patch_file(feed="contexts") and `long: {rate: file,
feed: contexts, pcm24: keep}` of predict.yaml, against the SAME calls on its fp32 image F = V 2^-23.  The cutters give the image's
bytes, so the model sees the same clips: labels, gaps and contexts are equal, `patched` is the input's bytes outside the regions and
the store rule applied to the fp32 run's `patched` inside them."""
import json
import wave

import numpy as np
import pytest
import torch

from speech_inpainting_amd import audio
from speech_inpainting_amd import gaps as G
from tests import s24_ref as S
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

SR, N_REC, CLIP, CTX = 48000, 300, 75, 15
N = N_REC * SR // 50 + 77
GAPS = [[(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)], [(30, 4), (140, 6), (200, 9)]]     # channel 0: test_gpu_long.py's; channel 1: its own
KW = dict(clip_frames=CLIP, min_context=CTX, feed="contexts")
_FILES = {}


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", "fp32", key=("patch", "fp32"))


def _file(ch):
    """(V int32 (N, ch), its packed bytes (N, ch, 3)): a synthetic recording per channel at 24 bits with no zero sample of its own and
    channel c's GAPS zeroed."""
    from speech_inpainting_amd import synth
    if ch not in _FILES:
        cols = []
        for c in range(ch):
            v = np.trunc(synth.synth_wave(1, N, 41 + c, sr=SR)[0].numpy().astype(np.float64) * S.HI).astype(np.int32)
            v[v == 0] = 1
            for s, l in G.file_spans(GAPS[c], SR):
                v[s:s + l] = 0
            cols.append(v)
        v = np.stack(cols, axis=1)
        _FILES[ch] = (v, S.pack(v))
    return _FILES[ch]


def _regions(ch):
    """Boolean (N, ch): the samples a repair of GAPS may write (the gaps and their 5 ms cross-fades)."""
    fade = G.file_fade(5.0, SR)
    m = np.zeros((N, ch), dtype=bool)
    for c in range(ch):
        for s, l in G.file_spans(GAPS[c], SR):
            m[max(s - fade, 0):s + l + fade, c] = True
    return m


def _compare(got, ref, v, b, ch, label):
    assert got["patched"].dtype == torch.uint8 and tuple(got["patched"].shape) == ((N, 3) if ch == 1 else (N, ch, 3)), label
    assert got["contexts"] == ref["contexts"] and got["label_off"] == ref["label_off"] and torch.equal(got["labels"], ref["labels"]), label
    assert got["labels"].numel() > 0
    out = got["patched"].cpu().numpy().reshape(N, ch, 3)
    want = S.store(ref["patched"].cpu().numpy().reshape(N, ch))
    m = _regions(ch)
    assert np.array_equal(out[~m], b.reshape(N, ch, 3)[~m]), label                               # the input's bytes outside the regions
    assert np.array_equal(S.unpack(out), want), (label, int((S.unpack(out) != want).sum()))      # the store rule of the fp32 run everywhere
    for c in range(ch):
        for s, l in G.file_spans(GAPS[c], SR)[:2]:
            assert np.any(S.unpack(out)[s:s + l, c] != 0), label                                 # the gaps were filled


@pytest.mark.parametrize("clips16", ["resampled", "file"])
@pytest.mark.parametrize("ch", [1, 2])
def test_conceal_file_and_patch_file_equal_the_fp32_image_s_runs(ch, clips16):
    eng = _engine()
    v, b = _file(ch)
    mono = ch == 1
    x24 = torch.from_numpy(b[:, 0] if mono else b)                     # (N, 3) | (N, 2, 3), a host tensor
    img = torch.from_numpy(S.image(v)[:, 0] if mono else S.image(v))
    kw = dict(KW, clips16=clips16)
    got = eng.conceal_file(x24, SR, threshold=0.0, merge_frames=1, **kw)
    ref = eng.conceal_file(img, SR, threshold=0.0, merge_frames=1, **kw)
    torch.cuda.synchronize()
    assert got["gaps"] == ref["gaps"] == (GAPS[0] if mono else GAPS) and got["skipped"] == ref["skipped"]
    _compare(got, ref, v, b, ch, ("conceal_file", ch, clips16))
    gaps_kw = dict(gaps=GAPS[0]) if mono else dict(channel_gaps=GAPS)
    got = eng.patch_file(b[:, 0] if mono else b, SR, **gaps_kw, **kw)                            # a numpy array of the WAV's bytes
    ref = eng.patch_file(img, SR, **gaps_kw, **kw)
    torch.cuda.synchronize()
    _compare(got, ref, v, b, ch, ("patch_file", ch, clips16))


def test_thresholds_count_24_bit_steps_and_one_channel_files_keep_their_shape():
    eng = _engine()
    v, b = _file(2)
    w = v.copy()
    for s, l in G.file_spans(GAPS[1], SR):
        w[s:s + l, 1] = np.where(np.arange(l) % 2 == 0, 300, -300)     # a noise floor of 300 steps in place of the zeros
    x = torch.from_numpy(S.pack(w))
    assert eng.find_gaps(x, SR, threshold=299.0, merge_frames=1, channel=1)["gaps"] == []
    assert eng.find_gaps(x, SR, threshold=300.0, merge_frames=1, channel=1)["gaps"] == GAPS[1]
    found = eng.find_gaps(x, SR, kind="level", win_ms=2.0, threshold=300.0, merge_frames=1, channel=1)
    assert found["gaps"] == GAPS[1] and found["threshold"] == 300.0
    held = eng.find_gaps(x, SR, kind="held", held_tol=600.0, merge_frames=1, channel=1)
    assert held["gaps"] == GAPS[1] and eng.find_gaps(x, SR, kind="held", held_tol=599.0, merge_frames=1, channel=1)["gaps"] == []
    runs, T = eng.find_dead_runs(x, "quiet", rel_threshold=2.0 ** -10, channel=-1, return_threshold=True)
    assert T == float(np.float32(np.abs(w).max()) * np.float32(2.0 ** -10))
    one = torch.from_numpy(S.pack(v[:, :1]))                           # (N, 1, 3): the mono route, reshaped at the end
    got = eng.conceal_file(one, SR, merge_frames=1, **KW)
    assert tuple(got["patched"].shape) == (N, 1, 3) and got["gaps"] == GAPS[0]


def test_no_gaps_is_an_exact_copy_and_launches_nothing():
    eng = _engine()
    _, b = _file(2)
    for x in (torch.from_numpy(b).to(eng.device), torch.from_numpy(b[:, 0]).to(eng.device)):
        eng.ctx.profile_start(100)
        kw = dict(gaps=[]) if x.dim() == 2 else dict(channel_gaps=[[], []])
        got = eng.patch_file(x, SR, **kw, **KW)
        launched = [e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0]
        assert launched == [] and got["patched"].data_ptr() != x.data_ptr() and torch.equal(got["patched"], x) and got["contexts"] == []


def test_refusals():
    eng = _engine()
    _, b = _file(2)
    with pytest.raises(ValueError, match=r"patch_file: packed 24-bit PCM needs feed = 'contexts'"):
        eng.patch_file(b, SR, channel_gaps=GAPS, clip_frames=CLIP, min_context=CTX)
    with pytest.raises(ValueError, match=r"conceal_file: packed 24-bit PCM needs feed = 'contexts'"):
        eng.conceal_file(b, SR, feed="recording")
    with pytest.raises(ValueError, match=r"patch_file: packed 24-bit PCM at 22050 Hz"):
        eng.patch_file(b, 22050, channel_gaps=GAPS, **KW)
    for bad in (b.reshape(-1), b.reshape(N, 6), b[:, :, :2], b.reshape(N, 2, 3, 1)):
        with pytest.raises(ValueError, match=r"patch_file: a uint8 input is packed 24-bit PCM"):
            eng.patch_file(bad, SR, gaps=GAPS[0], **KW)
    with pytest.raises(ValueError, match="at most 8"):
        eng.patch_file(np.zeros((N, 9, 3), np.uint8), SR, channel_gaps=[[]] * 9, **KW)


def test_predict_entry_point_keeps_a_24_bit_file(tmp_path, monkeypatch, capsys):
    """predict.py on a 6 s stereo 24-bit 48 kHz file with `detect:`: with `pcm24: keep` three 24-bit files of the input's n, rate and
    channels, masked.wav with the gaps' bytes zeroed, gaps.json's T in 24-bit steps; without the key, the float32 files of before."""
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
    n = 6 * SR + 123
    v = np.stack([np.trunc(synth.synth_wave(1, n, 5 + c, sr=SR)[0].numpy().astype(np.float64) * S.HI).astype(np.int32) for c in range(2)], axis=1)
    v[v == 0] = 1
    gaps = [[(25, 6), (250, 12)], [(100, 5)]]
    for c in range(2):
        for s, l in G.file_spans(gaps[c], SR):
            v[s:s + l, c] = 0
    b = S.pack(v)
    (tmp_path / "wavs").mkdir()
    audio.write_wav_s24(str(tmp_path / "wavs" / "call.wav"), b, SR)
    yaml = """
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{d}/wavs/call.wav', save_pred: '{d}/{out}'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts{key}}}
detect: {{min_ms: 5, kind: any, rel_threshold: 0.0000152587890625}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{d}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{d}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{d}/kmeans/', km_model_path: '{d}/kmeans/'}}}}
"""
    monkeypatch.chdir(tmp_path)
    (tmp_path / "predict.yaml").write_text(yaml.format(d=tmp_path, out="kept", key=", pcm24: keep"))
    assert main([]) == 0
    out = tmp_path / "kept" / "call"
    assert sorted(p.name for p in out.iterdir()) == ["gaps.json", "masked.wav", "orig.wav", "patched.wav"]
    report = json.loads((out / "gaps.json").read_text())
    peak = np.abs(v).max(axis=0).astype(np.float32) * np.float32(2.0 ** -16)
    assert report["gaps"] == [[list(g) for g in one] for one in gaps] and report["unit"] == "24-bit steps" and report["T"] == [float(t) for t in peak]
    assert "(24-bit steps)" in capsys.readouterr().out
    files = {}
    for f in ("orig.wav", "masked.wav", "patched.wav"):
        with wave.open(str(out / f)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 3, SR, n), f
        files[f], sr, ch = audio.read_wav_pcm(str(out / f))
        assert (sr, ch) == (SR, 2) and files[f].shape == (n, 2, 3)
    assert np.array_equal(files["orig.wav"], b)
    zeroed, keep = b.copy(), np.ones((n, 2), dtype=bool)
    fade = G.file_fade(5.0, SR)
    for c in range(2):
        for s, l in G.file_spans(gaps[c], SR):
            zeroed[s:s + l, c] = 0
            keep[s - fade:s + l + fade, c] = False
            assert np.any(files["patched.wav"][s:s + l, c] != 0)
    assert np.array_equal(files["masked.wav"], zeroed) and np.array_equal(files["patched.wav"][keep], b[keep])
    # without the key: what the same input produced before -- float32 files, T in full-scale units
    (tmp_path / "predict.yaml").write_text(yaml.format(d=tmp_path, out="plain", key=""))
    assert main([]) == 0
    plain = tmp_path / "plain" / "call"
    report = json.loads((plain / "gaps.json").read_text())
    assert report["gaps"] == [[list(g) for g in one] for one in gaps] and "unit" not in report
    for f in ("orig.wav", "masked.wav", "patched.wav"):
        sr, data = wavfile.read(plain / f)
        assert sr == SR and data.dtype == np.float32 and data.shape == (n, 2), f
    sr, data = wavfile.read(plain / "orig.wav")
    assert np.array_equal(data, (v.astype(np.float64) * 256).astype(np.float32) / np.float32(2147483648.0))
