"""The route of DESIGN.md 4.31: engine.conceal_file(mend_ms=...) and `detect: {mend_ms: ...}` in predict.yaml, with the tiny random
model.  A 48 kHz float file carries forty stray NaNs, three 8-sample NaN runs, one 200 ms NaN block and a NaN at the file's edge: with
mend_ms = 1 the short runs are filled from their own neighbourhood and only the block reaches the inpainter; with mend_ms = 0 the call is
the parent's, bit for bit and launch for launch, and regenerates a frame for every stray sample."""
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import invalid_ref as V
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

N_REC, CLIP, CTX = 300, 75, 15
KW = dict(clip_frames=CLIP, min_context=CTX, merge_frames=1)
SR, PER = 48000, 960
BLOCK = (100, 10)                                      # the 200 ms block, in frames
AR, EDGE, NONFINITE = native.MEND_AR, native.MEND_EDGE, native.MEND_NONFINITE
_FILES = {}


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", "fp32", key=("patch", "fp32"))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.int16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _speech(seed, frames=N_REC, extra=77):
    from speech_inpainting_amd import synth
    n = frames * PER + extra
    v = (synth.synth_wave(1, n, seed, sr=SR)[0] * 32767.0).to(torch.int16).numpy()
    return v, (v.astype(np.float32) / np.float32(32768.0))


def _file(edge):
    """-> (x, short rows, the edge row): 40 single NaNs in frames 8 .. 220, 8-sample NaN runs in frames 235, 250 and 265, the block, and
    the edge damage: `edge` = (3, 1) is one NaN at sample 3, (0, 4) a run that touches sample 0."""
    if edge not in _FILES:
        _, x = _speech(47)
        frames = [8 + 5 * i for i in range(18)] + [115 + 5 * (i - 18) for i in range(18, 40)]      # five frames apart: one context serves neighbours
        short = [(f * PER + 10 + (37 * i) % 900, 1) for i, f in enumerate(frames)] + [(f * PER + 100, 8) for f in (235, 250, 265)]
        for s, m in short + [edge]:
            x[s:s + m] = V.bits([0x7FC00001])[0]
        x[BLOCK[0] * PER:(BLOCK[0] + BLOCK[1]) * PER] = np.nan
        _FILES[edge] = (x, sorted(short), edge)
    return _FILES[edge]


def _launches(eng, call):
    eng.ctx.profile_start(8000)
    out = call()
    prof = {e["name"]: e["launches"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    torch.cuda.synchronize()
    return out, prof


def _blend_set(n, gaps, fade_ms=5.0):
    """The file samples a patch may change: the gaps' spans widened by the cross-fade."""
    some = np.zeros(n, bool)
    fade = G.file_fade(fade_ms, SR)
    for s, l in G.file_spans(gaps, SR):
        some[max(s - fade, 0):s + l + fade] = True
    return some


@pytest.mark.parametrize("edge", [(3, 1), (0, 4)], ids=["nan-at-3", "nan-0-to-3"])
def test_short_runs_are_mended_and_only_the_block_is_inpainted(edge):
    """The edge damage cannot be mended (status EDGE) and goes on to gaps.runs_to_gaps with the block.  A run that touches sample 0 is
    skipped there as "edge" and stays in the output, listed; one NaN at sample 3 does not touch sample 0, so runs_to_gaps makes it the
    gap (0, 1) -- with mend_ms = 0 just the same -- and the inpainter replaces it."""
    eng = _engine()
    x, short, edge = _file(edge)
    xt = torch.from_numpy(x)
    rows = V.invalid_runs_ref(x).tolist()
    assert len(rows) == 45 and rows[0] == list(edge) and [BLOCK[0] * PER, BLOCK[1] * PER] in rows
    got, prof = _launches(eng, lambda: eng.conceal_file(xt, SR, min_ms=0, kind="invalid", feed="contexts", mend_ms=1.0, **KW))
    touches = edge[0] == 0
    assert got["gaps"] == ([BLOCK] if touches else [(0, 1), BLOCK]) and got["skipped"] == ([(0, 1, "edge")] if touches else [])
    assert got["mended"] == [(edge[0], edge[1], EDGE)] + [(s, m, AR) for s, m in short] and got["threshold"] == float("inf")
    assert prof["patch_rate"] == 1 + 1                                  # the mending launch, in patch_rate's family, and one pass
    y, status = eng.mend_runs(xt, rows, max_len=48, order=32, context=512)
    torch.cuda.synchronize()
    assert status.tolist() == [EDGE] + [AR] * 18 + [native.MEND_LONG] + [AR] * 25
    patched = got["patched"].cpu()
    mended = np.zeros(x.size, bool)
    for s, m in short:
        mended[s:s + m] = True
    mt = torch.from_numpy(mended)
    assert torch.equal(_bits(patched)[mt], _bits(y.cpu())[mt]) and bool(torch.isfinite(patched[mt]).all())      # engine.mend_runs' samples, bit for bit
    rest = torch.from_numpy(~mended & ~_blend_set(x.size, got["gaps"]))
    assert torch.equal(_bits(patched)[rest], _bits(xt)[rest])           # every other sample outside the covers is x's, payload included
    fin = torch.isfinite(patched)
    if touches:
        assert not bool(fin[:4].any()) and torch.equal(_bits(patched)[:4], _bits(xt)[:4])      # the edge run stays, as listed
        fin[:4] = True
    assert bool(fin.all())


def test_without_mend_ms_the_call_is_the_parent_s():
    eng = _engine()
    x, short, _ = _file((3, 1))
    xt = torch.from_numpy(x)
    base, prof0 = _launches(eng, lambda: eng.conceal_file(xt, SR, min_ms=0, kind="invalid", feed="contexts", **KW))
    zero, prof1 = _launches(eng, lambda: eng.conceal_file(xt, SR, min_ms=0, kind="invalid", feed="contexts", mend_ms=0.0, mend_order=8, mend_context=64, **KW))
    assert len(base["gaps"]) > 40 and base["gaps"] == zero["gaps"] and base["skipped"] == zero["skipped"] and "mended" not in zero and "mended" not in base
    assert prof0 == prof1 and prof0["patch_rate"] >= 1
    assert torch.equal(_bits(base["patched"]), _bits(zero["patched"])) and torch.equal(base["labels"], zero["labels"])
    changed = int((_bits(base["patched"].cpu()) != _bits(xt)).sum())
    mend = eng.conceal_file(xt, SR, min_ms=0, kind="invalid", feed="contexts", mend_ms=1.0, **KW)
    assert int((_bits(mend["patched"].cpu()) != _bits(xt)).sum()) < changed // 3      # forty frames of good speech are no longer replaced


def test_channel_1_of_a_stereo_file():
    """detect="each": each channel mends its own runs; the clean channel keeps its bytes and lists nothing."""
    eng = _engine()
    right, short, edge = _file((0, 4))
    left = _speech(53)[1]
    xt = torch.from_numpy(np.stack([left, right], axis=1))
    got = eng.conceal_file(xt, SR, min_ms=0, kind="invalid", feed="contexts", detect="each", mend_ms=1.0, **KW)
    assert got["gaps"] == [[], [BLOCK]] and got["skipped"] == [[], [(0, 1, "edge")]]
    assert got["mended"] == [[], [(0, 4, EDGE)] + [(s, m, AR) for s, m in short]]
    y, status = eng.mend_runs(xt, V.invalid_runs_ref(right).tolist(), max_len=48, channel=1)
    torch.cuda.synchronize()
    patched = got["patched"].cpu()
    assert torch.equal(_bits(patched[:, 0]), _bits(xt[:, 0])) and torch.equal(_bits(y[:, 0].cpu()), _bits(xt[:, 0]))
    keep = torch.from_numpy(~_blend_set(right.size, [BLOCK]))
    assert torch.equal(_bits(patched[:, 1])[keep], _bits(y[:, 1].cpu())[keep]) and bool(torch.isfinite(patched[4:, 1]).all())


def test_clipped_peaks_in_an_int16_file():
    """threshold = 32766 in the file's own steps: three clipped peaks of 3 samples are mended as int16, the clipped block is inpainted."""
    eng = _engine()
    v, _ = _speech(47)
    v = (v // 2).astype(np.int16)
    (s, l), = G.file_spans([(120, 3)], SR)
    v[s:s + l] = np.where(np.arange(l) % 400 < 200, 32767, -32768)
    peaks = [(40 * PER + 17, 3), (60 * PER + 500, 3), (200 * PER + 901, 3)]
    for a, m in peaks:
        v[a:a + m] = 32767
    vt = torch.from_numpy(v)
    got = eng.conceal_file(vt, SR, 32766.0, min_ms=0, kind="invalid", feed="contexts", mend_ms=1.0, **KW)
    y, status = eng.mend_runs(vt, peaks, max_len=48)
    torch.cuda.synchronize()
    assert got["gaps"] == [(120, 3)] and got["skipped"] == [] and got["mended"] == [(a, m, AR) for a, m in peaks] and status.tolist() == [AR] * 3
    patched = got["patched"].cpu()
    keep = torch.from_numpy(~_blend_set(v.size, [(120, 3)]))
    assert patched.dtype == torch.int16 and torch.equal(patched[keep], y.cpu()[keep])
    for a, m in peaks:
        assert int(patched[a:a + m].abs().max()) < 32767 and torch.equal(patched[a - 600:a], vt[a - 600:a])


def test_a_joint_run_stays_a_gap_unless_every_channel_filled_it():
    eng = _engine()
    left, right = _speech(53)[1], _speech(47)[1]
    t0, t1 = 120 * PER + 500, 200 * PER + 300
    for t in (t0, t1):
        left[t] = right[t] = np.nan
    left[t0 + 200] = np.nan                                             # inside channel 0's context of t0; no joint run: channel 1 is valid there
    xt = torch.from_numpy(np.stack([left, right], axis=1))
    got = eng.conceal_file(xt, SR, min_ms=0, kind="invalid", feed="contexts", detect="joint", mend_ms=1.0, **KW)
    torch.cuda.synchronize()
    assert got["mended"] == [(t0, 1, NONFINITE), (t1, 1, AR)] and got["gaps"] == [(120, 1)] and got["skipped"] == []
    patched = got["patched"].cpu()
    y0, _ = eng.mend_runs(xt, [(t1, 1)], max_len=48, channel=0)
    y1, _ = eng.mend_runs(xt, [(t0, 1), (t1, 1)], max_len=48, channel=1)
    assert torch.equal(_bits(patched[t1]), _bits(torch.stack([y0[t1, 0], y1[t1, 1]]).cpu())) and bool(torch.isfinite(patched).all())
    with pytest.raises(ValueError, match="min_ms = 1.0 is not under mend_ms = 1.0"):
        eng.conceal_file(xt, SR, min_ms=1.0, kind="invalid", feed="contexts", mend_ms=1.0, **KW)
    with pytest.raises(ValueError, match="max_len = 96 samples, at most 64: lower mend_ms"):
        eng.conceal_file(xt, SR, min_ms=0, kind="invalid", feed="contexts", mend_ms=2.0, **KW)


def test_predict_entry_point_writes_mended_into_gaps_json(tmp_path, monkeypatch, capsys):
    """predict.py with `detect: {kind: invalid, mend_ms: 1.0}` on a 48 kHz float WAV: gaps.json records `mended` as a count by status."""
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
    _, x = _speech(47, frames=150)
    n = x.size
    x[25 * PER:31 * PER] = np.nan
    singles = [40 * PER + 7, 90 * PER + 959, 100 * PER + 400]
    for s in singles:
        x[s] = np.nan
    x[0:2] = np.nan
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", SR, x)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file, feed: contexts}}
detect: {{kind: invalid, mend_ms: 1.0}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    assert json.loads((out / "gaps.json").read_text()) == {"gaps": [[25, 6]], "skipped": [[0, 1, "edge"]], "kind": "invalid", "ceiling": None,
                                                           "mended": {"EDGE": 1, "AR": 3}}
    printed = capsys.readouterr().out
    assert "Mended runs of at most 1.0 ms, by status: {'EDGE': 1, 'AR': 3}" in printed and "Detected gap 0 = frames [25, 31)" in printed
    rate, wav = wavfile.read(out / "patched.wav")
    assert rate == SR and wav.dtype == np.float32 and len(wav) == n and np.isfinite(wav[2:]).all() and np.isnan(wav[:2]).all()
    keep = np.ones(n, dtype=bool)
    keep[PER * 25 - 240:PER * 31 + 240] = False
    keep[singles] = False
    assert np.array_equal(wav[keep].view(np.uint32), x[keep].view(np.uint32))
