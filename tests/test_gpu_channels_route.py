"""The route of DESIGN.md 4.18: engine.patch_file / conceal_file / find_gaps on interleaved (n, ch) files and `long: {rate: file}` of
predict.yaml on a stereo WAV, with the tiny random model of tests/test_gpu_feed_route.py.

The reference is the mono route on the de-interleaved channel: channel c of `patched`, and the labels of channel c's gaps, must equal
patch_file(x[:, c].contiguous(), sr, channel_gaps[c]) byte for byte, for both feeds and every batch size; a channel without gaps, and
every sample outside the cross-faded regions, must equal the file's bytes.  Channel 0 is recorded at a tenth of the other channels'
level."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 300, 75, 15
GAPS = [(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)]              # test_gpu_long.py's
SHORT = [(2, 3), (30, 4), (35, 4), (50, 8)]
KW = dict(clip_frames=CLIP, min_context=CTX)
DETECT = {"detect_bits_ch", "detect_carry", "detect_count", "detect_offsets", "detect_emit"}
# name -> (sr, channels, int16?, frames, extra samples, the gap lists: shared | one channel empty | channels differing)
FILES = {
    "stereo 48k int16": (48000, 2, True, N_REC, 77, (GAPS, [GAPS, []], [GAPS, [(50, 4), (200, 6)]])),
    "three channels 16k fp32": (16000, 3, False, N_REC, 77, (GAPS, [GAPS[:2], [], GAPS[2:]], [[(10, 3)], GAPS, [(50, 4), (200, 6)]])),
    "short 44.1k int16": (44100, 2, True, 60, 57, (SHORT, [[], SHORT], [SHORT, [(10, 5)]])),
    "stereo 22.05k int16": (22050, 2, True, N_REC, 77, (GAPS, [[], GAPS], [GAPS, [(50, 4), (200, 6)]])),
}
_FILES, _MONO = {}, {}


def _engine(voc="fp32"):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", voc, key=("patch", voc))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.int16 else torch.int32)


def _file(name):
    """The interleaved host file (n, ch): independent synthetic recordings, channel 0 at a tenth of the others' level, no sample zero."""
    from speech_inpainting_amd import synth
    if name not in _FILES:
        sr, ch, pcm, frames, extra, _ = FILES[name]
        n = -(-frames * sr // 50) + extra
        cols = [synth.synth_wave(1, n, 61 + 7 * c, sr=sr)[0] * (0.1 if c == 0 else 1.0) for c in range(ch)]
        x = torch.stack(cols, dim=1).contiguous()
        if pcm:
            x = (x * 32767.0).to(torch.int16)
            x[x == 0] = 1
        else:
            x[x == 0] = 1e-4
        _FILES[name] = x
    return _FILES[name]


def _mono(eng, name, c, gaps, feed, batch=32):
    """The reference: the mono route on the de-interleaved channel, once per (file, channel, gaps, feed, batch)."""
    key = (name, c, tuple(gaps), feed, batch)
    if key not in _MONO:
        out = eng.patch_file(_file(name)[:, c].contiguous(), FILES[name][0], list(gaps), feed=feed, batch=batch, **KW)
        _MONO[key] = {k: out[k] for k in ("patched", "labels", "label_off", "contexts")}
    return _MONO[key]


def _per_channel(name, which):
    gaps = FILES[name][5][which]
    return [gaps] * FILES[name][1] if which == 0 else gaps


def _check_against_mono(eng, name, got, per, feed, batch=32):
    sr, ch = FILES[name][:2]
    x = _file(name)
    fade_f = G.file_fade(5.0, sr)
    assert got["patched"].shape == x.shape and got["patched"].dtype == x.dtype and len(got["channel_off"]) == ch + 1
    assert got["channel_off"] == [sum(len(g) for g in per[:c]) for c in range(ch + 1)]
    assert [k["channel"] for k in got["contexts"]] == sorted(k["channel"] for k in got["contexts"])
    lo, co = got["label_off"], got["channel_off"]
    assert len(lo) == co[-1] + 1 and got["labels"].numel() == lo[-1]
    for c in range(ch):
        ref = _mono(eng, name, c, per[c], feed, batch)
        assert torch.equal(_bits(got["patched"][:, c]), _bits(ref["patched"])), (name, c, feed, int((got["patched"][:, c] != ref["patched"]).sum()))
        assert torch.equal(got["labels"][lo[co[c]]:lo[co[c + 1]]], ref["labels"]), (name, c, feed)
        assert [v - lo[co[c]] for v in lo[co[c]:co[c + 1] + 1]] == ref["label_off"]
        mine = [k for k in got["contexts"] if k["channel"] == c]
        assert [(k["start"], k["own"], k["foreign"]) for k in mine] == [(k["start"], k["own"], k["foreign"]) for k in ref["contexts"]]
        keep = np.ones(x.shape[0], dtype=bool)
        for s, l in G.file_spans(per[c], sr):
            keep[max(s - fade_f, 0):s + l + fade_f] = False
            assert not torch.equal(got["patched"][s:s + l, c].cpu(), x[s:s + l, c]), (name, c, s)              # the gap was filled
        assert torch.equal(_bits(got["patched"][:, c].cpu()[torch.from_numpy(keep)]), _bits(x[:, c][torch.from_numpy(keep)])), (name, c)
        if not per[c]:
            assert torch.equal(_bits(got["patched"][:, c].cpu()), _bits(x[:, c])), (name, c)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["shared gaps", "one channel empty", "channels differ"])
@pytest.mark.parametrize("name", list(FILES))
def test_every_channel_equals_the_mono_route_on_it(name, which):
    """Every file x every gap set, both feeds, batch = 1, 2 and 32: at batch 1 every context is a pass of its own, at 2 a pass boundary
    falls inside a channel or a pass holds the last context of one channel and the first of the next (for the file shorter than one
    clip: the two channels' single contexts share a pass or do not), and a channel without gaps is absent from every pass."""
    eng = _engine()
    sr = FILES[name][0]
    per = _per_channel(name, which)
    kw = dict(gaps=per[0]) if which == 0 else dict(channel_gaps=per)
    for feed in ("contexts", "recording") if sr != 22050 else ("contexts",):
        first = None
        for batch in (1, 2, 32):                                                 # each against the mono route at the same batch, and all three alike
            got = eng.patch_file(_file(name), sr, feed=feed, batch=batch, **kw, **KW)
            torch.cuda.synchronize()
            _check_against_mono(eng, name, got, per, feed, batch)
            first = first or got
            assert torch.equal(_bits(got["patched"]), _bits(first["patched"])) and torch.equal(got["labels"], first["labels"]), (name, feed, batch)
            assert got["label_off"] == first["label_off"] and got["contexts"] == first["contexts"] and got["channel_off"] == first["channel_off"]


def test_batching_changes_no_byte_and_a_pass_holds_several_channels():
    """batch = 1, 2 and 32 on the three-channel file with differing gaps: the same `patched` and labels; at batch 2 a pass boundary
    falls inside a channel, at 32 one pass holds all three, with one cut and one write-back launch per channel present."""
    eng = _engine()
    name = "three channels 16k fp32"
    sr, per = FILES[name][0], _per_channel(name, 2)
    eng.patch_file(_file(name), sr, channel_gaps=per, feed="contexts", **KW)                     # warm: the filters are built outside the profile
    eng.ctx.profile_start(4000)
    full = eng.patch_file(_file(name), sr, channel_gaps=per, batch=32, feed="contexts", return_windows=True, **KW)
    prof = {e["name"]: e["launches"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    torch.cuda.synchronize()
    assert [k["channel"] for k in full["contexts"]] == [0, 1, 1, 1, 1, 2, 2] and len(full["passes"]) == 1
    assert prof["cut_rate_ch"] == 3 and prof["patch_rate_ch"] == 3 and not {"cut_rate", "patch_rate", "cut_clips"} & set(prof), prof
    assert [c for c, _ in full["passes"][0]["tables"]] == [0, 1, 2]
    _check_against_mono(eng, name, full, per, "contexts")
    for batch in (1, 2):
        got = eng.patch_file(_file(name), sr, channel_gaps=per, batch=batch, feed="contexts", **KW)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got["patched"]), _bits(full["patched"])) and torch.equal(got["labels"], full["labels"]), batch
        assert got["label_off"] == full["label_off"] and got["contexts"] == full["contexts"] and got["channel_off"] == full["channel_off"]
    with pytest.raises(ValueError, match="both gaps and channel_gaps"):
        eng.patch_file(_file(name), sr, GAPS, channel_gaps=per, **KW)
    with pytest.raises(ValueError, match="2 lists for a file of 3 channels"):
        eng.patch_file(_file(name), sr, channel_gaps=per[:2], **KW)
    with pytest.raises(ValueError, match="9 channels, at most 8"):
        eng.patch_file(torch.zeros(1000, 9), sr, GAPS, **KW)


def test_conceal_file_each_and_joint():
    """A joint dropout in both channels and one in channel 1 alone: "each" finds both in channel 1 and one in channel 0, "joint" only
    the joint one; each result is patch_file on the gaps it found.  Nothing to find: an exact copy, only the detection launched."""
    eng = _engine()
    name = "stereo 48k int16"
    sr = FILES[name][0]
    clean = _file(name)
    x = clean.clone()
    joint, solo = (100, 5), (200, 6)
    (sj, lj), (ss, ls) = G.file_spans([joint, solo], sr)
    x[sj:sj + lj, :] = 0
    x[ss:ss + ls, 1] = 0
    each = eng.conceal_file(x, sr, threshold=0.0, feed="contexts", detect="each", **KW)
    both = eng.conceal_file(x, sr, threshold=0.0, feed="contexts", detect="joint", **KW)
    assert each["gaps"] == [[joint], [joint, solo]] and each["skipped"] == [[], []]
    assert both["gaps"] == [joint] and both["skipped"] == []
    assert eng.find_gaps(x, sr, channel=1)["gaps"] == [joint, solo] and eng.find_gaps(x, sr, channel=-1)["runs"].tolist() == [[sj, lj]]
    ref_each = eng.patch_file(x, sr, channel_gaps=each["gaps"], feed="contexts", **KW)
    ref_both = eng.patch_file(x, sr, [joint], feed="contexts", **KW)
    torch.cuda.synchronize()
    for got, ref in ((each, ref_each), (both, ref_both)):
        assert got["patched"].dtype == torch.int16 and torch.equal(got["patched"], ref["patched"]) and torch.equal(got["labels"], ref["labels"])
        assert int((got["patched"][sj:sj + lj] != 0).sum()) > lj
    assert int((each["patched"][ss:ss + ls, 1] != 0).sum()) > ls // 2 and bool((both["patched"][ss:ss + ls, 1] == 0).all())
    with pytest.raises(ValueError, match="detect = 'all'"):
        eng.conceal_file(x, sr, detect="all", **KW)
    for mode in ("each", "joint"):
        eng.ctx.profile_start(200)
        none = eng.conceal_file(clean, sr, feed="contexts", detect=mode, **KW)
        prof = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
        torch.cuda.synchronize()
        assert prof == DETECT, prof
        assert none["gaps"] == ([[], []] if mode == "each" else []) and none["contexts"] == [] and none["label_off"] == [0]
        assert none["channel_off"] == [0, 0, 0] and torch.equal(none["patched"].cpu(), clean) and none["patched"].data_ptr() != clean.data_ptr()


def test_one_dimensional_and_single_column_inputs_take_the_mono_route():
    eng = _engine()
    name = "stereo 48k int16"
    sr = FILES[name][0]
    col = _file(name)[:, 1].contiguous()
    eng.patch_file(col, sr, GAPS, feed="contexts", **KW)
    eng.ctx.profile_start(4000)
    flat = eng.patch_file(col, sr, GAPS, feed="contexts", **KW)
    prof = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    assert {"cut_rate", "patch_rate"} <= prof and not {n for n in prof if n.endswith("_ch")}, prof
    eng.ctx.profile_start(4000)
    column = eng.patch_file(col[:, None], sr, GAPS, feed="contexts", **KW)
    assert {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0} == prof
    by_list = eng.patch_file(col[:, None], sr, channel_gaps=[GAPS], feed="contexts", **KW)
    torch.cuda.synchronize()
    assert flat["patched"].shape == col.shape and column["patched"].shape == (col.numel(), 1) and "channel_off" not in flat
    assert torch.equal(column["patched"][:, 0], flat["patched"]) and torch.equal(by_list["patched"], column["patched"])
    assert torch.equal(column["labels"], flat["labels"]) and column["label_off"] == flat["label_off"]
    zeroed = col.clone()
    for s, l in G.file_spans(GAPS, sr):
        zeroed[s:s + l] = 0
    eng.ctx.profile_start(4000)
    a = eng.conceal_file(zeroed, sr, merge_frames=1, feed="contexts", **KW)
    names = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    b = eng.conceal_file(zeroed[:, None], sr, merge_frames=1, feed="contexts", **KW)
    torch.cuda.synchronize()
    assert a["gaps"] == GAPS == b["gaps"] and "detect_bits" in names and not {n for n in names if n.endswith("_ch")}
    assert b["patched"].shape == (col.numel(), 1) and torch.equal(b["patched"][:, 0], a["patched"])
    assert eng.find_quiet_runs(zeroed[:, None], 0.0, 100, channel=0).tolist() == eng.find_quiet_runs(zeroed, 0.0, 100).tolist()
    with pytest.raises(ValueError, match="takes `gaps`"):
        eng.patch_file(col, sr, channel_gaps=[GAPS], **KW)


def test_predict_entry_point_on_a_stereo_file(tmp_path, monkeypatch, capsys):
    """predict.py with `long: {rate: file, feed: contexts}` and `detect: {channels: each}` on a stereo int16 WAV whose channel 1 alone
    is damaged: patched.wav is stereo, int16, at the file's rate and holds patch_file's result, gaps.json holds one list per channel,
    and channel 0 is the input's, byte for byte."""
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
    pcm_in = np.stack([(synth.synth_wave(1, n, 5 + c, sr=sr)[0].numpy() * 32767).astype(np.int16) for c in range(2)], axis=1)
    pcm_in[pcm_in == 0] = 1
    gaps = [(25, 6), (100, 6)]
    for s, l in G.file_spans(gaps, sr):
        pcm_in[s:s + l, 1] = 0
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts}}
detect: {{channels: each}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    calls = []
    inner = InpaintingEngine.patch_file

    def spy(self, x, sr_, gaps=None, **kw):
        out = inner(self, x, sr_, gaps, **kw)
        calls.append((kw, out["patched"].cpu().numpy().copy(), tuple(x.shape)))
        return out

    monkeypatch.setattr(InpaintingEngine, "patch_file", spy)
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    kw, patched, shape = calls[0]
    assert shape == (n, 2) and kw["feed"] == "contexts" and kw["channel_gaps"] == [[], gaps]
    out = tmp_path / "prediction" / "call"
    assert json.loads((out / "gaps.json").read_text()) == {"gaps": [[], [list(g) for g in gaps]], "skipped": [[], []]}
    files = {}
    for f in ("orig.wav", "masked.wav", "patched.wav"):
        rate, files[f] = wavfile.read(out / f)
        assert rate == sr and files[f].dtype == np.int16 and files[f].shape == (n, 2), f
    assert np.array_equal(files["orig.wav"], pcm_in) and np.array_equal(files["masked.wav"], pcm_in)
    assert np.array_equal(files["patched.wav"], patched) and np.array_equal(files["patched.wav"][:, 0], pcm_in[:, 0])
    for s, l in G.file_spans(gaps, sr):
        assert int((files["patched.wav"][s:s + l, 1] != 0).sum()) > l // 2
    printed = capsys.readouterr().out
    assert "Detected gap 1 of channel 1 = frames [100, 106)" in printed and "Predicted codewords, channel 1, gap 0 = frames [25, 31)" in printed
