"""The route of DESIGN.md 4.26: engine.patch_file / engine.conceal_file with feed="contexts", clips16="file" and `long: {rate: file, feed:
contexts, clips16: file}` of predict.yaml -- the encoder's 16 kHz clips cut straight from the file beside the 22.05 kHz ones (si_cut_pair),
on test_gpu_feed_route.py's tiny random model and 6 s route file.

The kernels are held to their definition in tests/test_gpu_pair.py; here the contract is the routing: the default is today's bytes and
launches, clips16="file" launches one cut_rate-family kernel per pass and no resample_sinc, its clips are si_cut_pair's, and everything
after the cut is the same code.  Labels and `patched` of the two modes are compared and REPORTED, not asserted: the two sets of 16 kHz
clips are different signals at the clip edges (DESIGN.md 4.17 says why neither feed is "the" answer), and a random tiny model's arg-max
flips on less."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 300, 75, 15
GAPS = [(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)]              # test_gpu_long.py's
KW = dict(clip_frames=CLIP, min_context=CTX)
FILE = dict(feed="contexts", clips16="file")
L22, L16 = CLIP * 441, CLIP * 320
_FILES = {}


def _engine(voc="fp32"):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", voc, key=("patch", voc))


def _i32(t):
    return t.contiguous().view(torch.int32)


def _file(sr, seed=41, frames=N_REC, extra=77):
    """A recording of `frames` frames and `extra` samples at `sr` Hz as an fp32 and an int16 file that hold the same values."""
    from speech_inpainting_amd import synth
    if (sr, seed, frames) not in _FILES:
        n = -(-frames * sr // 50) + extra
        x16 = (synth.synth_wave(1, n, seed, sr=sr)[0] * 32767.0).to(torch.int16)
        _FILES[sr, seed, frames] = (x16.to(torch.float32) / 32768.0, x16)
    return _FILES[sr, seed, frames]


def _profiled(eng, run):
    eng.ctx.profile_start(4000)
    out = run()
    prof = [(e["name"], e["launches"]) for e in eng.ctx.profile_stop() if e["launches"] > 0]
    torch.cuda.synchronize()
    return out, prof


def _outside_regions(got, n):
    keep = np.ones(n, dtype=bool)
    for p in got["passes"]:
        for a, b in p["plan"]["regions"]:
            keep[a:b] = False
    return keep


def test_the_default_is_unchanged():
    """clips16="resampled" is the call without the option: the same bytes, the same profiled launches in the same order."""
    eng = _engine()
    _, x16 = _file(48000)
    eng.patch_file(x16, 48000, GAPS, batch=3, feed="contexts", **KW)                        # warm: the filters are cached outside the profile
    a, pa = _profiled(eng, lambda: eng.patch_file(x16, 48000, GAPS, batch=3, feed="contexts", return_windows=True, **KW))
    b, pb = _profiled(eng, lambda: eng.patch_file(x16, 48000, GAPS, batch=3, feed="contexts", clips16="resampled", return_windows=True, **KW))
    assert pa == pb and dict(pa)["resample_sinc"] == 2 and dict(pa)["cut_rate"] == 2
    assert torch.equal(a["patched"], b["patched"]) and torch.equal(a["labels"], b["labels"]) and a["contexts"] == b["contexts"]
    assert all("clips16" not in p for p in a["passes"] + b["passes"])
    c, pc = _profiled(eng, lambda: eng.patch_file(x16, 48000, GAPS, batch=3, **KW))
    d, pd = _profiled(eng, lambda: eng.patch_file(x16, 48000, GAPS, batch=3, clips16="resampled", **KW))
    assert pc == pd and torch.equal(c["patched"], d["patched"]) and "cut_rate" not in dict(pc)


@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_clips16_file_on_the_mono_route(voc):
    """An int16 48 kHz file: no resample_sinc launch and one cut_rate-family launch per pass; clips22 are the default route's bytes;
    clips16 are si_cut_pair's called alone; `patched` is the file outside the blend regions, bit for bit; the labels and samples that
    differ from the default route are reported."""
    eng = _engine(voc)
    sr = 48000
    _, x16 = _file(sr)
    old = eng.patch_file(x16, sr, GAPS, batch=3, feed="contexts", return_windows=True, **KW)
    eng.patch_file(x16, sr, GAPS, batch=3, **FILE, **KW)                                    # warm
    got, prof = _profiled(eng, lambda: eng.patch_file(x16, sr, GAPS, batch=3, return_windows=True, **FILE, **KW))
    prof = dict(prof)
    assert len(got["contexts"]) == 4 and len(got["passes"]) == 2 and got["contexts"] == old["contexts"] and got["label_off"] == old["label_off"]
    assert "resample_sinc" not in prof and "cut_clips" not in prof and "cut_rate_ch" not in prof
    assert prof["cut_rate"] == 2 and prof["patch_rate"] == 2                                # passes of 3 + 1 clips
    xd = x16.to(eng.device)
    f22, f16 = eng._feed_filter(sr), eng._feed_filter16(sr)
    for p, q in zip(got["passes"], old["passes"]):
        frames = [c["start"] for c in p["contexts"]]
        assert p["clips22"].shape == (len(frames), L22) and p["clips16"].shape == (len(frames), L16)
        assert torch.equal(_i32(p["clips22"]), _i32(q["clips22"]))
        w22, w16 = eng.ctx.cut_pair(xd, sr, frames, L22, L16, f22, f16)
        assert torch.equal(_i32(p["clips22"]), _i32(w22)) and torch.equal(_i32(p["clips16"]), _i32(w16))
        two = eng.resample(q["clips22"], 22050, 16000)
        d = (two - p["clips16"]).abs()
        print(f"   {sr} Hz {voc}: 16 kHz clips of a pass, file against resampled: max |d| {float(d.max()):.3e} over the clips, "
              f"{float(d[:, 200:-200].max()):.3e} in their interior (signal max {float(p['clips16'].abs().max()):.3f})")
    keep = _outside_regions(got, x16.numel())
    out = got["patched"].cpu().numpy()
    assert got["patched"].dtype == torch.int16 and np.array_equal(out[keep], x16.numpy()[keep]) and int((~keep).sum()) > 0
    for s, l in G.file_spans(GAPS, sr):                                                      # every gap was filled, by something other than the recording
        assert not np.array_equal(out[s:s + l], x16.numpy()[s:s + l]) and not keep[s:s + l].any()
    labels = int((got["labels"] != old["labels"]).sum())
    dp = (got["patched"].to(torch.int32) - old["patched"].to(torch.int32)).abs()
    print(f"   {sr} Hz {voc}: clips16 file against resampled: {labels} of {got['labels'].numel()} labels differ; patched differs in "
          f"{int((dp != 0).sum())} samples by up to {int(dp.max())} int16 steps")


def test_batching_changes_no_byte_and_conceal_file_is_patch_file():
    eng = _engine()
    sr = 48000
    x16 = _file(sr, seed=47)[1].clone()
    for s, l in G.file_spans(GAPS, sr):
        x16[s:s + l] = 0
    full = eng.patch_file(x16, sr, GAPS, batch=32, **FILE, **KW)
    for batch in (1, 2):
        got = eng.patch_file(x16, sr, GAPS, batch=batch, **FILE, **KW)
        torch.cuda.synchronize()
        assert torch.equal(got["patched"], full["patched"]) and torch.equal(got["labels"], full["labels"]), batch
        assert got["label_off"] == full["label_off"] and got["contexts"] == full["contexts"]
    found = eng.conceal_file(x16, sr, threshold=0.0, merge_frames=1, **FILE, **KW)
    torch.cuda.synchronize()
    assert found["gaps"] == GAPS and found["skipped"] == []
    assert found["patched"].dtype == torch.int16 and torch.equal(found["patched"], full["patched"]) and torch.equal(found["labels"], full["labels"])


def test_a_16_khz_file_reaches_the_encoder_as_it_is():
    """An fp32 16 kHz file: the encoder's input rows are the file's samples, bit for bit; the default route's rows are not."""
    eng = _engine()
    sr = 16000
    x32, _ = _file(sr)
    got, prof = _profiled(eng, lambda: eng.patch_file(x32, sr, GAPS, return_windows=True, **FILE, **KW))
    old = eng.patch_file(x32, sr, GAPS, feed="contexts", return_windows=True, **KW)
    torch.cuda.synchronize()
    assert dict(prof)["cut_rate"] == 1 and "resample_sinc" not in dict(prof) and len(got["passes"]) == 1
    w16 = got["passes"][0]["clips16"].cpu()
    starts = [c["start"] for c in got["contexts"]]
    assert starts == [0, 68, 106, 225]
    for b, f in enumerate(starts):
        assert torch.equal(_i32(w16[b]), _i32(x32[320 * f:320 * f + L16]))
    assert torch.equal(_i32(got["passes"][0]["clips22"]), _i32(old["passes"][0]["clips22"]))
    two = eng.resample(old["passes"][0]["clips22"], 22050, 16000).cpu()
    d = (two - w16).double()
    print(f"   16 kHz file: the resampled clips differ from the file by RMS {float(d.pow(2).mean().sqrt()):.3e}, max {float(d.abs().max()):.3e} "
          f"(signal RMS {float(w16.double().pow(2).mean().sqrt()):.3f}); the cut clips by 0")
    assert float(d.abs().max()) > 1e-4
    keep = _outside_regions(got, x32.numel())
    assert torch.equal(_i32(got["patched"].cpu())[torch.from_numpy(keep)], _i32(x32)[torch.from_numpy(keep)])
    print(f"   16 kHz file: {int((got['labels'] != old['labels']).sum())} of {got['labels'].numel()} labels differ between the two modes")


def test_a_stereo_int16_file_channel_by_channel():
    """Each channel byte-equal to the mono route on its copy; one cut_rate_ch launch per channel present in a pass, nothing else cuts."""
    eng = _engine()
    sr = 48000
    x = torch.stack([_file(sr, seed=41)[1], _file(sr, seed=43)[1]], dim=1).contiguous()
    per = [GAPS[:3], GAPS[2:]]
    eng.patch_file(x, sr, channel_gaps=per, **FILE, **KW)                                   # warm
    got, prof = _profiled(eng, lambda: eng.patch_file(x, sr, channel_gaps=per, return_windows=True, **FILE, **KW))
    prof = dict(prof)
    assert got["patched"].shape == x.shape and got["patched"].dtype == torch.int16
    assert "resample_sinc" not in prof and "cut_rate" not in prof and "cut_clips" not in prof
    n_ch = sum(len(G.pass_channels(p["contexts"])) for p in got["passes"])
    assert prof["cut_rate_ch"] == n_ch == 2 and len(got["passes"]) == 1
    off = got["channel_off"]
    for c in (0, 1):
        mono = eng.patch_file(x[:, c].contiguous(), sr, per[c], return_windows=True, **FILE, **KW)
        torch.cuda.synchronize()
        assert torch.equal(got["patched"][:, c], mono["patched"]), c
        lo = got["label_off"]
        assert torch.equal(got["labels"][lo[off[c]]:lo[off[c + 1]]], mono["labels"]), c
        rows = [b for b, k in enumerate(got["passes"][0]["contexts"]) if k["channel"] == c]
        assert torch.equal(_i32(got["passes"][0]["clips16"][rows]), _i32(torch.cat([p["clips16"] for p in mono["passes"]])))
        assert torch.equal(_i32(got["passes"][0]["clips22"][rows]), _i32(torch.cat([p["clips22"] for p in mono["passes"]])))


def test_refusals():
    eng = _engine()
    _, x16 = _file(48000)
    eng.ctx.profile_start(100)
    with pytest.raises(ValueError, match="clips16 = 'file' needs feed = 'contexts'"):
        eng.patch_file(x16, 48000, GAPS, feed="recording", clips16="file", **KW)
    with pytest.raises(ValueError, match="clips16 = 'file' needs feed = 'contexts'"):
        eng.conceal_file(x16, 48000, clips16="file", **KW)
    with pytest.raises(ValueError, match="clips16 = 'direct': 'resampled' or 'file'"):
        eng.patch_file(x16, 48000, GAPS, feed="contexts", clips16="direct", **KW)
    with pytest.raises(ValueError, match="clips16 = 'file' needs feed = 'contexts'"):
        eng.patch_file(torch.stack([x16, x16], dim=1), 48000, GAPS, clips16="file", **KW)
    launched = [e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0 and not e["name"].startswith("detect")]
    assert launched == [], launched
    # at 22050 Hz the option is not read, as feed is not
    x22 = _file(22050, seed=45)[1]
    a = eng.patch_file(x22, 22050, GAPS, **KW)
    b = eng.patch_file(x22, 22050, GAPS, clips16="file", **KW)
    assert torch.equal(a["patched"], b["patched"]) and torch.equal(a["labels"], b["labels"])


def test_predict_entry_point_with_clips16_file(tmp_path, monkeypatch, capsys):
    """predict.py with `long: {rate: file, feed: contexts, clips16: file}` and `detect:` on a 48 kHz int16 file: the key reaches
    patch_file, is printed, and gaps.json records it."""
    import joblib
    from scipy.io import wavfile
    from sklearn.cluster import MiniBatchKMeans
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.engine import InpaintingEngine
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
    for p, l in ((25, 6), (100, 6)):
        pcm_in[960 * p:960 * (p + l)] = 0
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts, clips16: file}}
detect: {{min_ms: 5}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    calls = []
    inner = InpaintingEngine.patch_file

    def spy(self, x, sr_, gaps, **kw):
        self.ctx.profile_start(4000)
        out = inner(self, x, sr_, gaps, **kw)
        names = {e["name"] for e in self.ctx.profile_stop() if e["launches"] > 0}
        calls.append((kw, out["patched"].cpu().numpy().copy(), names, list(gaps)))
        return out

    monkeypatch.setattr(InpaintingEngine, "patch_file", spy)
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    assert len(calls) == 1
    kw, patched, names, gaps = calls[0]
    assert kw["feed"] == "contexts" and kw["clips16"] == "file" and len(gaps) == 2
    assert "cut_rate" in names and "resample_sinc" not in names and "cut_clips" not in names
    out = tmp_path / "prediction" / "call"
    assert json.loads((out / "gaps.json").read_text()) == {"gaps": [list(g) for g in gaps], "skipped": [], "clips16": "file"}
    assert "16 kHz clips: clips16 = file" in capsys.readouterr().out
    rate, wav = wavfile.read(out / "patched.wav")
    assert rate == sr and wav.dtype == np.int16 and np.array_equal(wav, patched)
    for p, l in gaps:
        assert int((wav[960 * p:960 * (p + l)] != 0).sum()) > 960 * l // 2
