"""The route of DESIGN.md 4.17: engine.patch_file / engine.conceal_file with feed="contexts" and `long: {rate: file, feed: contexts}` of
predict.yaml -- the model fed by context clips cut straight from the file (si_cut_rate), on test_gpu_rate.py's route shapes.

Each pass's clips22 is held to the kernel's bound against tests/feed_ref.py; `patched` to DESIGN.md 4.16's bound against
tests/rate_ref.py composed from the pass's own windows and gains; every sample outside the regions to the file's bits.  Against
feed="recording" the clips are held to the CPU test's bound (tests/test_feed_ref.py) with its two exclusions; the labels and `patched` of
the two feeds are compared and REPORTED, not asserted: a rounding can flip an arg-max of a random tiny model."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from tests import feed_ref as F
from tests import rate_ref as R
from tests.harness import RatioSummary, build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 300, 75, 15
GAPS = [(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)]              # test_gpu_long.py's
KW = dict(clip_frames=CLIP, min_context=CTX)
ROUTE_RATES = [48000, 16000]
SUMMARY = RatioSummary()
_FILES, _CLIPS = {}, {}


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


def _clip_ref(x16, sr, seed, starts, L):
    """feed_ref of the context clips, once per file (both sample types hold the same values)."""
    key = (sr, seed, tuple(starts), L)
    if key not in _CLIPS:
        _CLIPS[key] = F.clips(x16.numpy(), sr, starts, L)
    return _CLIPS[key]


def _check_clips(got, x16, sr, seed, label):
    """Every pass's clips22 within the kernel's bound of the definition.  -> the reference (y, A, S) of all contexts, in order."""
    starts = [441 * c["start"] for c in got["contexts"]]
    w22 = torch.cat([p["clips22"] for p in got["passes"]]).cpu().numpy()
    y, A, S = _clip_ref(x16, sr, seed, starts, w22.shape[1])
    assert w22.shape == y.shape
    ratio = np.abs(w22.astype(np.float64) - y) / F.kernel_bound(y, A, sr)
    edge = np.zeros(y.shape, dtype=bool)
    edge[:, :F.reach(sr)] = edge[:, -F.reach(sr):] = True
    SUMMARY.note(label, float(ratio[edge].max()), float(ratio[~edge].max()) if (~edge).any() else 0.0)
    assert float(ratio.max()) <= 1.0, (label, float(ratio.max()))
    return y, A, S


def _check_patched(got, x, sr, pcm, label, it=None):
    """`patched` against rate_ref.compose on the (one) pass's own windows and gains: 4.16's bound inside the regions, the file's bits
    outside.  -> the interpolation record, for the file's other sample type."""
    assert len(got["passes"]) == 1
    p = got["passes"][0]
    plan, gen, gain = p["plan"], p["gen"].cpu().numpy(), p["gain"].cpu().numpy()
    fade_f = G.file_fade(5.0, sr)
    if it is None:
        it = R.interpolate(sr, plan["spans"], plan["rows"], [gen[w][:row[2]] for w, row in enumerate(plan["rows"])], fade_f, x.numel())
    ref, E, written = R.blend(x.numpy(), it, gain)
    out = got["patched"].cpu().numpy()
    word = np.int16 if pcm else np.int32
    assert np.array_equal(out[~written].view(word), x.numpy()[~written].view(word)), label                # the file's, bit for bit
    assert int(written.sum()) >= sum(l for _, l in G.file_spans(GAPS[:4], sr))
    if not pcm:
        ratio = float((np.abs(out[written].astype(np.float64) - ref[written]) / E[written]).max())
        SUMMARY.note(label, ratio, ratio)
        assert ratio <= 1.0, (label, ratio)
    else:                                                             # test_gpu_rate.py's int16 rule
        v = ref[written] * 32768.0
        d = out[written].astype(np.float64) - np.trunc(v)
        near = np.abs(v - np.round(v)) <= E[written] * 32768.0
        assert np.all((d == 0) | ((np.abs(d) == 1) & near)), (label, int(np.sum((d != 0) & ~near)))
        assert np.mean(d != 0) <= 0.10 and np.mean(near) < 0.05, (label, float(np.mean(d != 0)), float(np.mean(near)))
    return it


@pytest.mark.parametrize("sr", ROUTE_RATES)
@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_patch_file_fed_by_contexts(voc, sr):
    """The acceptance test: fp32 and int16 files; a context at the recording's start, one clamped to its end, two that share a
    foreign gap."""
    eng = _engine(voc)
    x32, x16 = _file(sr)
    got = eng.patch_file(x32, sr, GAPS, return_windows=True, feed="contexts", **KW)
    got16 = eng.patch_file(x16.numpy(), sr, list(reversed(GAPS)), return_windows=True, feed="contexts", **KW)      # a host array, the gaps in any order
    torch.cuda.synchronize()
    assert got["patched"].dtype == torch.float32 and got16["patched"].dtype == torch.int16 and got16["patched"].shape == x16.shape
    ctxs = got["contexts"]
    assert [c["start"] for c in ctxs] == [0, 68, 106, 225] and got16["contexts"] == ctxs and ctxs[-1]["start"] == N_REC - CLIP
    # contexts 68 and 106 each hold, masked, a gap that the other one owns: (140, 6) cut by the clip's end and (106, 4) at the clip's start
    assert [[c["start"] + p for p, _ in c["foreign"]] for c in ctxs] == [[], [140], [106], []]
    assert got["label_off"] == [0, 3, 8, 12, 18, 23] and torch.equal(got["labels"], got16["labels"])
    for res in (got, got16):
        _check_clips(res, x16, sr, 41, f"clips22 {sr} Hz")
    assert torch.equal(_i32(got["passes"][0]["clips22"]), _i32(got16["passes"][0]["clips22"]))
    it = _check_patched(got, x32, sr, False, f"patched {sr} Hz {voc}")
    _check_patched(got16, x16, sr, True, f"patched {sr} Hz {voc}", it)
    for s, l in G.file_spans(GAPS, sr):                               # every gap was filled, by something other than the recording
        assert not np.array_equal(got16["patched"].cpu().numpy()[s:s + l], x16.numpy()[s:s + l])
    SUMMARY.report(keys=[f"clips22 {sr} Hz", f"patched {sr} Hz {voc}"])


def test_a_recording_shorter_than_a_clip():
    """One context, the whole recording with its true sample count (60 frames and 57 samples, int16) at 44.1 kHz: the clip is the
    whole 22.05 kHz axis, its last sample the interpolated one of 4.17 (b)."""
    eng = _engine()
    sr, gaps = 44100, [(2, 3), (30, 4), (35, 4), (50, 8)]
    _, x16 = _file(sr, seed=53, frames=60, extra=57)
    assert x16.numel() % 2 == 1
    got = eng.patch_file(x16, sr, gaps, return_windows=True, feed="contexts", **KW)
    torch.cuda.synchronize()
    assert len(got["contexts"]) == 1 and got["contexts"][0]["own"] == gaps and got["label_off"] == [0, 3, 7, 11, 19]
    w22 = got["passes"][0]["clips22"]
    assert w22.shape == (1, F.n22(x16.numel(), sr)) and float(w22[0, -1]) != 0.0
    _check_clips(got, x16, sr, 53, "clips22 short 44100 Hz")
    p = got["passes"][0]
    it = R.interpolate(sr, p["plan"]["spans"], p["plan"]["rows"], [p["gen"][w].cpu().numpy()[:row[2]] for w, row in enumerate(p["plan"]["rows"])],
                       G.file_fade(5.0, sr), x16.numel())
    ref, E, written = R.blend(x16.numpy(), it, p["gain"].cpu().numpy())
    out = got["patched"].cpu().numpy()
    assert np.array_equal(out[~written], x16.numpy()[~written]) and int(written.sum()) == sum(l for _, l in G.file_spans(gaps, sr)) + 2 * G.file_fade(5.0, sr) * 4
    v = ref[written] * 32768.0
    d = out[written].astype(np.float64) - np.trunc(v)
    near = np.abs(v - np.round(v)) <= E[written] * 32768.0
    assert np.all((d == 0) | ((np.abs(d) == 1) & near)) and np.mean(d != 0) <= 0.10
    SUMMARY.report(keys=["clips22 short 44100 Hz"])


@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_batching_changes_no_byte(voc):
    eng = _engine(voc)
    for sr in ROUTE_RATES:
        _, x16 = _file(sr, seed=43)
        full = eng.patch_file(x16, sr, GAPS, batch=32, feed="contexts", **KW)
        for batch in (1, 2):
            got = eng.patch_file(x16, sr, GAPS, batch=batch, feed="contexts", **KW)
            torch.cuda.synchronize()
            assert torch.equal(got["patched"], full["patched"]) and torch.equal(got["labels"], full["labels"]), (sr, batch)
            assert got["label_off"] == full["label_off"] and got["contexts"] == full["contexts"]


def test_conceal_file_is_patch_file_on_the_gaps_it_found():
    eng = _engine()
    sr = 48000
    x16 = _file(sr, seed=47)[1].clone()
    for s, l in G.file_spans(GAPS, sr):
        x16[s:s + l] = 0
    got = eng.conceal_file(x16, sr, threshold=0.0, merge_frames=1, feed="contexts", **KW)
    ref = eng.patch_file(x16, sr, GAPS, feed="contexts", **KW)
    torch.cuda.synchronize()
    assert got["gaps"] == GAPS and got["skipped"] == []
    assert got["patched"].dtype == torch.int16 and torch.equal(got["patched"], ref["patched"]) and torch.equal(got["labels"], ref["labels"])
    for s, l in G.file_spans(GAPS, sr):
        assert int((got["patched"][s:s + l] != 0).sum()) > l // 2
    with pytest.raises(ValueError, match="feed = 'clips'"):
        eng.patch_file(x16, sr, GAPS, feed="clips", **KW)


def test_a_22050_hz_file_is_patch_recording_bit_for_bit():
    eng = _engine()
    x32, x16 = _file(22050, seed=45)
    ref = eng.patch_recording(x16.to(torch.float32) / 32768.0, GAPS, fade=110, pcm=True, **KW)
    eng.ctx.profile_start(4000)
    got16 = eng.patch_file(x16, 22050, GAPS, feed="contexts", **KW)
    names = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    ref32 = eng.patch_recording(x32, GAPS, fade=110, **KW)
    got32 = eng.patch_file(x32, 22050, GAPS, feed="contexts", **KW)
    torch.cuda.synchronize()
    assert got16["patched"].dtype == torch.int16 and torch.equal(got16["patched"], ref["patched_pcm"]) and torch.equal(got16["labels"], ref["labels"])
    assert torch.equal(_i32(got32["patched"]), _i32(ref32["patched"])) and torch.equal(got32["labels"], ref32["labels"])
    assert "cut_rate" not in names and "cut_clips" in names


@pytest.mark.parametrize("pcm", [False, True], ids=["fp32", "int16"])
def test_no_gaps_is_an_exact_copy_and_launches_nothing(pcm):
    eng = _engine()
    x32, x16 = _file(48000, seed=51)
    x = (x16 if pcm else x32).to(eng.device)
    if not pcm:
        x.view(torch.int32)[5] = -2 ** 31
        x.view(torch.int32)[6] = 0x7fc12345
    eng.ctx.profile_start(100)
    got = eng.patch_file(x, 48000, [], return_windows=True, feed="contexts", **KW)
    launched = [e for e in eng.ctx.profile_stop() if e["launches"] > 0]
    torch.cuda.synchronize()
    assert launched == [], launched                                   # neither cut_rate nor a model kernel
    assert got["patched"].data_ptr() != x.data_ptr() and got["patched"].dtype == x.dtype
    assert torch.equal(got["patched"].view(torch.int16), x.view(torch.int16))
    assert got["contexts"] == [] and got["labels"].numel() == 0 and got["label_off"] == [0] and got["passes"] == []


@pytest.mark.parametrize("sr", ROUTE_RATES)
def test_only_the_16_khz_clips_go_through_the_whole_clip_resampler(sr):
    """With gaps: one cut_rate launch per pass, no cut_clips, and resample_sinc only with the shapes of the 22.05 -> 16 kHz clips."""
    eng = _engine()
    _, x16 = _file(sr)
    from speech_inpainting_amd import audio
    L22 = CLIP * 441
    L16 = audio.design_kaiser_best(22050, 16000, L22)["n_out"]
    eng.patch_file(x16, sr, GAPS, batch=3, feed="contexts", **KW)     # warm: the filters are built and cached outside the profile
    eng.ctx.profile_start(4000)
    got = eng.patch_file(x16, sr, GAPS, batch=3, feed="contexts", **KW)
    prof = {e["name"]: e for e in eng.ctx.profile_stop() if e["launches"] > 0}
    torch.cuda.synchronize()
    assert len(got["contexts"]) == 4
    assert prof["cut_rate"]["launches"] == 2 and "cut_clips" not in prof and prof["patch_rate"]["launches"] == 2
    rs = prof["resample_sinc"]
    assert rs["launches"] == 2 and rs["bytes"] == 4.0 * 4 * (L22 + L16), (rs, L22, L16)     # passes of 3 + 1 clips: (B, L22) -> (B, L16), nothing else
    eng.ctx.profile_start(4000)
    eng.patch_file(x16, sr, GAPS, batch=3, **KW)
    rec = {e["name"]: e for e in eng.ctx.profile_stop() if e["launches"] > 0}
    n_file = x16.numel()
    assert "cut_rate" not in rec and rec["cut_clips"]["launches"] == 2 and rec["resample_sinc"]["launches"] == 3
    assert rec["resample_sinc"]["bytes"] == rs["bytes"] + 4.0 * (n_file + audio.design_kaiser_best(sr, 22050, n_file)["n_out"])      # the default route: + the whole file


@pytest.mark.parametrize("sr", ROUTE_RATES)
def test_against_the_whole_file_feed(sr):
    """clips22 against the slices of the whole-file resample: within 2^-23 max(|a|, |b|) + S tau_j, tau_j = (j + 2) 2^-53 (j Q / P),
    the integer-time outputs (j a multiple of P) and those at or past int(n ratio) left out.  Labels and `patched`: reported."""
    eng = _engine()
    P, Q = G.rate_ratio(sr)
    x32, x16 = _file(sr)
    got = eng.patch_file(x16, sr, GAPS, return_windows=True, feed="contexts", **KW)
    old = eng.patch_file(x16, sr, GAPS, return_windows=True, feed="recording", **KW)
    wave22 = eng.resample(x32.to(eng.device)[None], sr, 22050)[0]
    torch.cuda.synchronize()
    assert old["contexts"] == got["contexts"] and wave22.numel() == F.n22(x16.numel(), sr)
    starts = [441 * c["start"] for c in got["contexts"]]
    L22 = CLIP * 441
    a = torch.cat([p["clips22"] for p in got["passes"]]).cpu().numpy().astype(np.float64)
    b = np.stack([wave22[s:s + L22].cpu().numpy() for s in starts]).astype(np.float64)
    assert np.array_equal(b.astype(np.float32), torch.cat([p["clips22"] for p in old["passes"]]).cpu().numpy())
    _, _, S = _clip_ref(x16, sr, 41, starts, L22)
    j = np.asarray(starts, dtype=np.int64)[:, None] + np.arange(L22)[None, :]
    tol = 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b)) + S * ((j + 2) * 2.0 ** -53 * (j * Q / P))
    keep = (j % P != 0) & (j < int(x16.numel() * (22050.0 / sr)))
    d = np.abs(a - b)
    assert not (d[keep] > tol[keep]).any(), (sr, float((d[keep] / tol[keep]).max()))
    whole = ~keep
    labels = int((got["labels"] != old["labels"]).sum())
    dp = (got["patched"].to(torch.int32) - old["patched"].to(torch.int32)).abs()
    print(f"   feeds at {sr} Hz: {int((d[keep] != 0).sum())} of {int(keep.sum())} clip samples change bits (max {float(d[keep].max()):.3e}); "
          f"{int((d[whole] != 0).sum())} of {int(whole.sum())} left-out samples differ (max {float(d[whole].max()):.3e}); "
          f"{labels} of {got['labels'].numel()} labels differ; patched.wav differs in {int((dp != 0).sum())} samples by up to {int(dp.max())} int16 steps")


def test_predict_entry_point_with_feed_contexts(tmp_path, monkeypatch, capsys):
    """predict.py with `long: {rate: file, feed: contexts}` on a 48 kHz int16 file: _main_long_file passes the key on, and patched.wav
    holds patch_file's result."""
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
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
masks:
  - {{start_pos_in_sec: 2.0, end_pos_in_sec: 2.125}}
  - {{start_pos_in_sec: 0.5, end_pos_in_sec: 0.625}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts}}
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
    assert kw["feed"] == "contexts" and "cut_rate" in names and "cut_clips" not in names and gaps == [(25, 6), (100, 6)]
    rate, wav = wavfile.read(tmp_path / "prediction" / "call" / "patched.wav")
    assert rate == sr and wav.dtype == np.int16 and np.array_equal(wav, patched)
    keep = np.ones(n, dtype=bool)
    for p, l in gaps:
        keep[960 * p - 240:960 * (p + l) + 240] = False               # 960 samples per frame, the default fade: 5 ms = 240
        assert not np.array_equal(wav[960 * p:960 * (p + l)], pcm_in[960 * p:960 * (p + l)])
    assert np.array_equal(wav[keep], pcm_in[keep])
