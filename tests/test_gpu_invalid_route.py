"""The route of DESIGN.md 4.30: engine.conceal_file / conceal_recording / find_gaps with kind="invalid", the ceiling on its way into
patch_file / patch_recording, and `detect: {kind: invalid}` in predict.yaml, with the tiny random model.

The damage here is the sample VALUES: blocks of NaN, +-inf and 3e38, single NaNs, a block that touches sample 0.  The feeds stage such
a sample as +0.0, so everything the model sees equals, bit for bit, what it sees for the file with those samples replaced by +0.0 --
while `patched` is still blended against the caller's own samples.  Without the ceiling the same gaps leave NaN OUTSIDE the masked
spans of the clips: that contrast is why the feed exists."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from tests import invalid_ref as V
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 300, 75, 15
KW = dict(clip_frames=CLIP, min_context=CTX, merge_frames=1)
PK = dict(clip_frames=CLIP, min_context=CTX)
INF = float("inf")
_FILES = {}


def _engine(voc="fp32"):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", voc, key=("patch", voc))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.int16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _speech(sr, seed, frames=N_REC, extra=77):
    """A valid recording at `sr` Hz on the int16 grid: int16 values and the fp32 file v / 32768."""
    from speech_inpainting_amd import synth
    n = -(-frames * sr // 50) + extra
    v = (synth.synth_wave(1, n, seed, sr=sr)[0] * 32767.0).to(torch.int16).numpy()
    return v, (v.astype(np.float32) / np.float32(32768.0))


def _float_file(sr, seed=47, frames=N_REC):
    """-> (x, blocks, want_gaps): two whole-frame blocks (NaN patterns, +-inf and one 3e38 deep inside; all NaN), a NaN at the last
    sample of frame 150, a scatter of single NaNs inside frame 170, and a block that touches sample 0."""
    key = (sr, seed, frames)
    if key not in _FILES:
        _, x = _speech(sr, seed, frames)
        per = sr // 50
        assert per * 50 == sr
        bad = np.concatenate([V.bits(V.NAN_BITS), np.float32([np.inf, -np.inf])])
        (a0, al), (b0, bl) = G.file_spans([(100, 10), (200, 10)], sr)
        x[a0:a0 + al] = bad[np.arange(al) % bad.size]
        x[a0 + al // 2] = np.float32(3e38)                              # finite: valid without a ceiling, and far from the block's edges
        x[b0:b0 + bl] = V.bits([0xFFC00000])[0]
        x[150 * per + per - 1] = np.nan
        for k in (0, 7, 8, per // 2, per - 1):
            x[170 * per + k] = np.nan
        x[0:per // 2] = V.bits([0x7F800001])[0]                         # the edge block, with a payload that must survive
        blocks = [(a0, al), (b0, bl), (150 * per + per - 1, 1), (170 * per, per)]
        _FILES[key] = (x, blocks, [(100, 10), (150, 1), (170, 1), (200, 10)])
    return _FILES[key]


def _weight_sets(n, gaps, sr, fade_ms=5.0):
    """(w == 1, w > 0) per file sample for `gaps` (frames) with the default cross-fade: inside a span, inside a span widened by the fade."""
    one, some = np.zeros(n, bool), np.zeros(n, bool)
    fade = G.file_fade(fade_ms, sr)
    for s, l in G.file_spans(gaps, sr):
        one[s:s + l] = True
        some[max(s - fade, 0):s + l + fade] = True
    return one, some


def _compare_patched(got, want, x, gaps, sr, skipped_cover):
    """patched against the call on clean(x): equal where x is valid or w == 1; x's own bits, payload included, where w == 0; finite
    outside the skipped covers."""
    xt = torch.as_tensor(x)
    valid = torch.from_numpy(~V.invalid_mask(np.asarray(x), INF))
    one, some = (torch.from_numpy(m) for m in _weight_sets(xt.shape[0], gaps, sr))
    g, w = got.cpu(), want.cpu()
    keep = valid | one
    assert torch.equal(_bits(g)[keep], _bits(w)[keep])
    assert torch.equal(_bits(g)[~some], _bits(xt)[~some])
    fin = torch.isfinite(g)
    for a, b in skipped_cover:
        fin[a:b] = True
    assert bool(fin.all()) and not bool(torch.isfinite(g[:skipped_cover[0][1]]).all())    # the edge block stays, as reported


@pytest.mark.parametrize("clips16", ["file", "resampled"])
def test_invalid_blocks_in_a_48_khz_fp32_file(clips16):
    eng = _engine()
    sr = 48000
    x, blocks, want_gaps = _float_file(sr)
    per = sr // 50
    xt = torch.from_numpy(x)
    rows = V.invalid_runs_ref(x).tolist()
    # the edge block, block A split in two by its 3e38, the single NaN, the scatter's four runs (7 and 8 are one), block B
    assert len(rows) == 1 + 2 + 1 + 4 + 1 and rows[0] == [0, per // 2]
    found = eng.find_gaps(xt, sr, min_ms=0, kind="invalid", merge_frames=1)
    assert found["runs"].tolist() == rows and found["gaps"] == want_gaps and found["skipped"] == [(0, 1, "edge")] and found["threshold"] == INF
    eng.ctx.profile_start(8000)
    got = eng.conceal_file(xt, sr, min_ms=0, kind="invalid", feed="contexts", clips16=clips16, return_windows=True, **KW)
    names = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    assert got["gaps"] == want_gaps and got["skipped"] == [(0, 1, "edge")] and got["threshold"] == INF
    assert "detect_bits" in names and "cut_rate" in names and not names & {"detect_dead", "detect_peak", "resample_sinc"} - ({"resample_sinc"} if clips16 == "resampled" else set())
    same = eng.patch_file(xt, sr, want_gaps, feed="contexts", clips16=clips16, ceiling=INF, **PK)          # the route adds no arithmetic
    want = eng.patch_file(torch.from_numpy(V.clean(x)), sr, want_gaps, feed="contexts", clips16=clips16, return_windows=True, **PK)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got["patched"]), _bits(same["patched"])) and torch.equal(got["labels"], same["labels"])
    assert torch.equal(got["labels"], want["labels"]) and got["label_off"] == want["label_off"] and len(got["passes"]) == len(want["passes"]) >= 1
    for a, b in zip(got["passes"], want["passes"]):
        assert a["contexts"] == b["contexts"]
        for k in ("gen", "clips22", "gain") + (("clips16",) if clips16 == "file" else ()):
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
        assert bool(torch.isfinite(a["gen"]).all()) and bool(torch.isfinite(a["clips22"]).all())
    _compare_patched(got["patched"], want["patched"], x, want_gaps, sr, [(0, per)])
    for s, l in blocks[:2]:
        assert bool(torch.isfinite(got["patched"][s:s + l]).all()) and bool((got["patched"][s:s + l].cpu() != 0).any())
    assert _bits(got["patched"])[:per // 2].cpu().tolist() == [0x7F800001] * (per // 2)                      # the edge block's payload
    # the contrast: the same gaps WITHOUT the ceiling -- the parent's call -- leave non-finite samples outside every masked span
    plain = eng.patch_file(xt, sr, want_gaps, feed="contexts", clips16=clips16, return_windows=True, **PK)
    rows_seen = 0
    for p in plain["passes"]:
        for b, c in enumerate(p["contexts"]):
            outside = torch.ones(p["clips22"].shape[1], dtype=torch.bool)
            for q, l in c["own"] + c["foreign"]:
                outside[441 * q:441 * (q + l)] = False
            assert int((~torch.isfinite(p["clips22"][b].cpu()) & outside).sum()) > 0, c
            rows_seen += 1
    assert rows_seen >= 2


def test_the_other_kinds_find_none_of_the_float_blocks():
    eng = _engine()
    sr = 48000
    x, blocks, _ = _float_file(sr)
    xt = torch.from_numpy(x)
    touching = lambda gaps: [g for g in gaps for s, l in blocks if g[0] * sr < (s + l) * 50 and (g[0] + g[1]) * sr > s * 50]
    for kind, thr, kw in (("quiet", 0.0, {}), ("held", 0.0, {}), ("level", 16.0 / 32768, {"win_ms": 2.0}), ("burst", 1.15, {"win_ms": 4.0})):
        found = eng.find_gaps(xt, sr, thr, kind=kind, merge_frames=1, **kw)
        assert touching(found["gaps"]) == [], (kind, found["gaps"])
    with pytest.raises(ValueError, match="rel_threshold = 0.5 with kind = 'invalid'"):
        eng.conceal_file(xt, sr, kind="invalid", rel_threshold=0.5, feed="contexts", **KW)
    with pytest.raises(ValueError, match="held_tol = 1.0 with kind = 'invalid'"):
        eng.conceal_file(xt, sr, kind="invalid", held_tol=1.0, feed="contexts", **KW)
    with pytest.raises(ValueError, match=r'patch_file: ceiling = inf needs feed="contexts" at 48000 Hz'):
        eng.conceal_file(xt, sr, min_ms=0, kind="invalid", **KW)                                      # feed="recording", the default
    with pytest.raises(ValueError, match="kind = 'invalid' with detect_on"):
        eng.conceal_recording(xt[:22050], detect_on=xt, sr=sr, kind="invalid", **KW)


def test_invalid_blocks_in_a_22_khz_recording():
    """conceal_recording(kind="invalid", min_ms=0): si_cut_clips_valid on the 22.05 kHz route, a caller's wave16 under the same ceiling."""
    eng = _engine()
    sr = 22050
    x, blocks, want_gaps = _float_file(sr, seed=43)
    xt = torch.from_numpy(x)
    eng.ctx.profile_start(8000)
    got = eng.conceal_recording(xt, min_ms=0, kind="invalid", **KW)
    names = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    want = eng.patch_recording(torch.from_numpy(V.clean(x)), want_gaps, **PK)
    torch.cuda.synchronize()
    assert got["gaps"] == want_gaps and got["skipped"] == [(0, 1, "edge")] and got["threshold"] == INF and "cut_clips" in names and "detect_bits" in names
    assert torch.equal(got["labels"], want["labels"])
    one = np.zeros(x.size, bool)
    some = np.zeros(x.size, bool)
    for p, l in want_gaps:
        one[441 * p:441 * (p + l)] = True
        some[441 * p - 110:441 * (p + l) + 110] = True
    valid = torch.from_numpy(~V.invalid_mask(x, INF) | one)
    g, w = got["patched"].cpu(), want["patched"].cpu()
    assert torch.equal(_bits(g)[valid], _bits(w)[valid]) and torch.equal(_bits(g)[torch.from_numpy(~some)], _bits(xt)[torch.from_numpy(~some)])
    assert bool(torch.isfinite(g[441:]).all()) and not bool(torch.isfinite(g[:441]).all())
    # a caller's 16 kHz recording with the same damage: its clips are cleaned under the same ceiling
    w16 = eng.resample(torch.from_numpy(V.clean(x))[None].to(eng.device), 22050, 16000)[0].contiguous()
    d16 = w16.clone()
    for p, l in want_gaps:
        d16[320 * p:320 * (p + l)] = float("nan")
    a = eng.patch_recording(xt, want_gaps, wave16=d16, ceiling=INF, **PK)
    d16z = torch.where(torch.isfinite(d16), d16, torch.zeros_like(d16))
    b = eng.patch_recording(torch.from_numpy(V.clean(x)), want_gaps, wave16=d16z, **PK)
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(_bits(a["patched"].cpu())[valid], _bits(b["patched"].cpu())[valid])


def test_invalid_blocks_in_channel_1_of_a_stereo_file():
    """detect="each": the damage is repaired in the channel it is in, the other channel keeps its bytes."""
    eng = _engine()
    sr = 48000
    right, blocks, want_gaps = _float_file(sr)
    left = _speech(sr, 53)[1]
    x = np.stack([left, right], axis=1)
    xt = torch.from_numpy(x)
    got = eng.conceal_file(xt, sr, min_ms=0, kind="invalid", feed="contexts", detect="each", **KW)
    want = eng.patch_file(torch.from_numpy(np.stack([left, V.clean(right)], axis=1)), sr, channel_gaps=[[], want_gaps], feed="contexts", **PK)
    torch.cuda.synchronize()
    assert got["gaps"] == [[], want_gaps] and got["skipped"] == [[], [(0, 1, "edge")]] and got["threshold"] == [INF, INF]
    assert torch.equal(got["labels"], want["labels"]) and torch.equal(_bits(got["patched"][:, 0].cpu()), _bits(xt[:, 0]))
    _compare_patched(got["patched"][:, 1], want["patched"][:, 1], right, want_gaps, sr, [(0, sr // 50)])
    joint = eng.conceal_file(xt, sr, min_ms=0, kind="invalid", feed="contexts", detect="joint", **KW)
    assert joint["gaps"] == [] and torch.equal(_bits(joint["patched"].cpu()), _bits(xt))              # no time is invalid in every channel


def test_a_clipped_run_in_an_int16_file():
    """threshold = 32766 in the file's own steps marks the clipped samples of an int16 file."""
    eng = _engine()
    sr = 48000
    v, _ = _speech(sr, 47)
    v = (v // 2).astype(np.int16)
    (s, l), = G.file_spans([(120, 3)], sr)
    v[s:s + l] = np.where(np.arange(l) % 400 < 200, 32767, -32768)
    rows = V.invalid_runs_ref(v, 32766.0).tolist()
    assert rows == [[s, l]] and V.invalid_runs_ref(v, 32767.0).tolist() != rows
    vt = torch.from_numpy(v)
    found = eng.find_gaps(vt, sr, 32766.0, min_ms=0, kind="invalid", merge_frames=1)
    assert found["runs"].tolist() == rows and found["gaps"] == [(120, 3)] and found["threshold"] == 32766.0
    assert eng.find_gaps(vt, sr, min_ms=0, kind="invalid", merge_frames=1)["gaps"] == []                 # no ceiling: PCM is always valid
    got = eng.conceal_file(vt, sr, 32766.0, min_ms=0, kind="invalid", feed="contexts", **KW)
    same = eng.patch_file(vt, sr, [(120, 3)], feed="contexts", ceiling=32766.0, **PK)
    want = eng.patch_file(torch.from_numpy(V.clean(v, 32766.0)), sr, [(120, 3)], feed="contexts", **PK)
    torch.cuda.synchronize()
    assert got["patched"].dtype == torch.int16 and torch.equal(got["patched"], same["patched"]) and torch.equal(got["labels"], want["labels"])
    one, some = _weight_sets(v.size, [(120, 3)], sr)
    keep = torch.from_numpy(one | ~some)
    assert torch.equal(got["patched"].cpu()[keep], want["patched"].cpu()[keep])
    assert int((got["patched"][s:s + l].cpu().abs() >= 32767).sum()) < l // 4                           # the clipping was replaced


def test_predict_entry_point_with_kind_invalid(tmp_path, monkeypatch, capsys):
    """predict.py with `detect: {kind: invalid}` on a 48 kHz float WAV with a NaN block and a single NaN: gaps.json names the kind and
    the ceiling (null: none), patched.wav is finite and keeps the input's bits outside the blends.  With `feed: recording` the run ends
    with the engine's refusal."""
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
    _, x = _speech(sr, 47, frames=150)
    n = x.size
    x[25 * 960:31 * 960] = np.nan
    x[100 * 960 + 959] = -np.inf
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, x)
    text = f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: FEED}}
detect: {{kind: invalid}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
"""
    (tmp_path / "predict.yaml").write_text(text.replace("FEED", "contexts"))
    rows = V.invalid_runs_ref(x).tolist()
    assert rows == [[25 * 960, 6 * 960], [100 * 960 + 959, 1]]
    n_rec = -(-n * 147 // 320) // 441
    gaps, skipped = G.runs_to_gaps(rows, n, sr, n_rec, merge_frames=2)
    assert gaps == [(25, 6), (100, 1)] and skipped == []
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    assert json.loads((out / "gaps.json").read_text()) == {"gaps": [[25, 6], [100, 1]], "skipped": [], "kind": "invalid", "ceiling": None}
    printed = capsys.readouterr().out
    assert "Detection kind = invalid, ceiling = none (full scale)" in printed and "Detected gap 1 = frames [100, 101)" in printed
    rate, wav = wavfile.read(out / "patched.wav")
    assert rate == sr and wav.dtype == np.float32 and len(wav) == n and np.isfinite(wav).all()
    keep = np.ones(n, dtype=bool)
    for p, l in gaps:
        keep[960 * p - 240:960 * (p + l) + 240] = False
    assert np.array_equal(wav[keep].view(np.uint32), x[keep].view(np.uint32))
    assert np.abs(wav[25 * 960:31 * 960]).max() > 0
    (tmp_path / "predict.yaml").write_text(text.replace("FEED", "recording"))
    with pytest.raises(ValueError, match=r'patch_file: ceiling = inf needs feed="contexts" at 48000 Hz'):
        main([])
