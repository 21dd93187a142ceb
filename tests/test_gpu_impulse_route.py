"""The route of DESIGN.md 4.33: engine.find_gaps / conceal_file with kind="impulse", and `detect: {kind: impulse}` in predict.yaml, with
the tiny random model and the recordings of tests/test_gpu_level_route.py.

The damage is clicks of one to three IN-RANGE samples (+-20 000 int16 steps added, clipped), 9 000 samples apart, plus one 200 ms zeroed
block.  Each builder first asserts with the CPU reference (tests/impulse_ref.py, its conditions included) that the clean file has no run
and that every click outside the block lies in a run of at most 16 samples.  conceal_file(kind="impulse", feed="contexts", min_ms=0,
mend_ms=1.0) must then find the reference's runs, mend the clicks in place (status AR), leave every other sample's bits alone and write
exactly what engine.mend_runs writes on the reference's rows; the quiet, level and burst detectors at their documented settings find no
click, and kind quiet still finds the block."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import impulse_ref as I
from tests import s24_ref as S
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 150, 75, 15
BLOCK = [(100, 10)]                                                   # one zeroed block of 200 ms
KW = dict(clip_frames=CLIP, min_context=CTX, merge_frames=1)
IMP = dict(kind="impulse", min_ms=0, mend_ms=1.0, feed="contexts")
D = G.IMPULSE_DEFAULTS
_FILES = {}


def _engine(voc="fp32"):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", voc, key=("patch", voc))


def _file(sr, seed, kind="int16", frames=N_REC, block=BLOCK):
    """-> (x as numpy in the reference's dtype, clean, clicks [(start, len)] outside the block, the block (start, len), reference rows)."""
    from speech_inpainting_amd import synth
    key = (sr, seed, kind, frames, tuple(block))
    if key not in _FILES:
        n = -(-frames * sr // 50) + 77
        clean = (synth.synth_wave(1, n, seed, sr=sr)[0] * 32767.0).to(torch.int16).numpy()
        x = clean.astype(np.int32)
        rng = np.random.default_rng(seed)
        clicks = [(10000 + 9000 * k, 1 + k % 3) for k in range((n - 12000) // 9000)]
        for s, m in clicks:
            x[s:s + m] += rng.choice((-1, 1), m) * 20000
        x = np.clip(x, -32768, 32767)
        (bs, bl), = G.file_spans(block, sr) if block else [(n, 0)]
        x[bs:bs + bl] = 0
        clicks = [(s, m) for s, m in clicks if s + m + 600 < bs or s > bs + bl + 600]
        if kind == "fp32":
            x, clean = (x / 32768.0).astype(np.float32), (clean / 32768.0).astype(np.float32)
        elif kind == "s24":
            low = rng.integers(0, 256, n).astype(np.int32)
            x, clean = np.where(x == 0, 0, x * 256 + low).astype(np.int32), (clean.astype(np.int32) * 256 + low).astype(np.int32)
        else:
            x = x.astype(np.int16)
        half = G.level_half(D["win_ms"], sr)
        case = I.Case(f"route file {key}", x, I.base_kw(order=D["order"], half=half, guard=D["guard"], pad=D["pad"], ratio=D["ratio"]))
        rows, _, _ = I.check(case)
        rows = rows.tolist()
        assert I.impulse_runs_ref(clean, D["order"], half, D["guard"], D["pad"], D["ratio"])[0].shape == (0, 2)
        assert all(any(a <= s and s + m <= a + l and l <= 16 for a, l in rows) for s, m in clicks), (rows, clicks)
        assert len(clicks) >= 8
        _FILES[key] = (x, clean, clicks, (bs, bl), rows)
    return _FILES[key]


def _hits(gaps, clicks, sr):
    """The gaps (frames) that touch a click."""
    return [g for g in gaps for s, m in clicks if g[0] * sr < (s + m) * 50 and (g[0] + g[1]) * sr > s * 50]


def _route(eng, x, sr, ref, clicks, block, rows, channel=None, threshold_scale=1.0, others=True):
    """The assertions every file shares.  x: the device input; ref: the host tensor of the same layout."""
    found = eng.find_gaps(x, sr, kind="impulse", min_ms=0, merge_frames=1, channel=channel)
    assert found["runs"].tolist() == rows and found["threshold"] == 0.0
    eng.ctx.profile_start(4000)
    got = eng.conceal_file(x, sr, **IMP, **KW)
    names = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    torch.cuda.synchronize()
    assert "detect_dead" in names and "patch_rate" in names and not names & {"detect_bits", "detect_bits_ch", "detect_peak"}
    mended = got["mended"] if channel is None else got["mended"][channel]
    gaps = got["gaps"] if channel is None else got["gaps"][channel]
    assert [(s, l) for s, l, _ in mended] == [tuple(r) for r in rows if r[1] <= 48]
    status = {(s, l): st for s, l, st in mended}
    for s, m in clicks:
        (a, l), = [(a, l) for a, l in rows if a <= s and s + m <= a + l]
        assert status[(a, l)] == native.MEND_AR, (s, m, status[(a, l)])
    assert _hits(gaps, clicks, sr) == []                                # no click costs a generated frame
    want, st = eng.mend_runs(ref, [tuple(r) for r in rows if r[1] <= 48], max_len=48, **({} if channel is None else {"channel": channel}))
    filled = [(s, l) for (s, l, c) in mended if c in (native.MEND_AR, native.MEND_LINE)]
    keep = torch.ones(ref.shape[0], dtype=torch.bool)
    for s, l in filled:
        keep[s:s + l] = False
    for p, k in gaps:
        keep[max(p * sr // 50 - sr // 100, 0):(p + k) * sr // 50 + sr // 100] = False
    patched = got["patched"].cpu()
    assert patched.dtype == ref.dtype and patched.shape == ref.shape
    assert torch.equal(patched[keep], ref[keep])                       # every sample outside the mended runs keeps its bits
    for s, l in filled:
        assert torch.equal(patched[s:s + l], want.cpu()[s:s + l]) and not torch.equal(patched[s:s + l], ref[s:s + l])
    if others:
        full = threshold_scale
        for kind, thr, kw in (("quiet", 0.0, {}), ("level", 16.0 / 32768.0 * full, {"win_ms": 2.0}), ("burst", 1.15 * full, {"win_ms": 4.0})):
            none = eng.conceal_file(x, sr, thr, kind=kind, feed="contexts", **kw, **KW)
            g = none["gaps"] if channel is None else none["gaps"][channel]
            assert _hits(g, clicks, sr) == [], (kind, g)
            if kind == "quiet" and block[1]:
                assert any(p * sr <= (block[0] + 960) * 50 and (p + k) * sr >= (block[0] + block[1] - 960) * 50 for p, k in g), g
    return got


def test_clicks_in_a_48_khz_int16_file():
    eng = _engine()
    x, clean, clicks, block, rows = _file(48000, 47)
    ref = torch.from_numpy(x)
    got = _route(eng, ref, 48000, ref, clicks, block, rows, threshold_scale=32768.0)
    # mend_ms = 0 stays legal: every click then costs a generated frame
    plain = eng.conceal_file(ref, 48000, kind="impulse", min_ms=0, feed="contexts", **KW)
    assert "mended" not in plain and len(_hits(plain["gaps"], clicks, 48000)) >= len(clicks) - 2
    # min_ms at its 5 ms default drops every click; win_ms and the impulse_* keywords reach the detector
    assert eng.find_gaps(ref, 48000, kind="impulse")["runs"].shape[0] == 0
    half = G.level_half(10.0, 48000)
    alt = eng.find_gaps(ref, 48000, kind="impulse", min_ms=0, win_ms=10.0, impulse_order=8, impulse_guard=8, impulse_pad=3, impulse_ratio=8.0)
    assert alt["runs"].tolist() == I.impulse_runs_ref(x, 8, half, 8, 3, 8.0)[0].tolist() != rows
    with pytest.raises(ValueError, match="held_tol = 1.0 with kind = 'impulse'"):
        eng.conceal_file(ref, 48000, kind="impulse", held_tol=1.0, **KW)
    with pytest.raises(ValueError, match=r"half \+ pad = 1026 samples \(win_ms = 42.65 at 48000 Hz\), above 1024: lower win_ms to 42.583 or less"):
        eng.conceal_file(ref, 48000, kind="impulse", win_ms=42.65, **KW)
    assert got["threshold"] == 0.0


def test_clicks_in_a_48_khz_fp32_file():
    eng = _engine()
    x, clean, clicks, block, rows = _file(48000, 43, "fp32")
    ref = torch.from_numpy(x)
    _route(eng, ref, 48000, ref, clicks, block, rows, threshold_scale=1.0)
    # a floor under the prediction error: relative to the peak, T comes back
    found = eng.find_gaps(ref, 48000, kind="impulse", min_ms=0, rel_threshold=0.5)
    assert found["threshold"] == float(np.float32(0.5) * np.abs(x).max())
    assert found["runs"].tolist() == I.impulse_runs_ref(x, 16, G.level_half(23.0, 48000), 4, 2, 10.0, rel=0.5)[0].tolist()


def test_clicks_in_one_channel_of_a_stereo_file():
    eng = _engine()
    left = torch.from_numpy(_file(48000, 53, block=[])[1])             # a clean channel
    x, clean, clicks, block, rows = _file(48000, 47)
    ref = torch.stack([left, torch.from_numpy(x)], dim=1).contiguous()
    got = _route(eng, ref, 48000, ref, clicks, block, rows, channel=1, threshold_scale=32768.0, others=False)
    assert got["mended"][0] == [] and got["gaps"][0] == [] and torch.equal(got["patched"][:, 0].cpu(), ref[:, 0])


def test_clicks_in_a_packed_24_bit_file():
    eng = _engine()
    v, clean, clicks, block, rows = _file(48000, 47, "s24")
    ref = torch.from_numpy(S.pack(v))
    _route(eng, ref, 48000, ref, clicks, block, rows, threshold_scale=8388608.0)


def test_predict_entry_point_with_kind_impulse(tmp_path, monkeypatch, capsys):
    """predict.py with `detect: {kind: impulse, min_ms: 0, mend_ms: 1}` on a 48 kHz int16 file: the clicks are mended, gaps.json names the
    kind, T, win_ms, ratio, order, guard and pad, and counts the mended runs by status."""
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
    pcm_in, clean, clicks, block, rows = _file(sr, 47, block=[])
    n = len(pcm_in)
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts}}
detect: {{kind: impulse, min_ms: 0, mend_ms: 1}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    report = json.loads((out / "gaps.json").read_text())
    assert {k: report[k] for k in ("kind", "T", "win_ms", "ratio", "order", "guard", "pad")} == \
        {"kind": "impulse", "T": 0.0, "win_ms": 23.0, "ratio": 10.0, "order": 16, "guard": 4, "pad": 2}
    assert report["mended"].get("AR", 0) >= len(clicks) and sum(report["mended"].values()) == len(rows)
    assert "Detection kind = impulse, effective threshold T = 0.0 (int16 steps), window win_ms = 23.0, ratio = 10.0, order = 16, guard = 4, pad = 2" in capsys.readouterr().out
    rate, wav = wavfile.read(out / "patched.wav")
    assert rate == sr and wav.dtype == np.int16 and len(wav) == n
    for s, m in clicks:
        assert not np.array_equal(wav[s:s + m], pcm_in[s:s + m])
        assert int(np.abs(wav[s:s + m].astype(np.int32) - clean[s:s + m]).max()) < 5000        # the click was +-20 000 steps
