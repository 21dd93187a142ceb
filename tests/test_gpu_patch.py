"""Patch mode: the generated audio of the gaps spliced into the caller's own 22.05 kHz samples -- si_wave_peak,
si_gather_windows, si_patch_compose, engine.patch_multigap_batch / patch_from_wave, `patch=` of predict_* and stream.Request, and the
`patch:` key of predict.yaml.

Common shapes: a tiny HuBERT + the V1 generator on clips of 1.5 s (n16 = 24000, n22 = 33075: T = 74, Tm = 75, 129 stretched frames,
n_out = 33024 < n22), the gaps below (none / clip start / near the end / two gaps one frame apart) and fades of 0, 110 and 300 samples
(at 300 the ramps of (30, 4) and (35, 4) overlap: their spans are 441 samples apart)."""
import json

import numpy as np
import pytest
import torch

from tests.cases import CHUNK, FADES, HOP, N_OUT, _weights64
from tests.cases import _patch_engine as _engine
from tests.common import case_engine, load_case

pytestmark = pytest.mark.gpu

GAPS = [[(20, 5)], [(0, 3), (60, 10)], [], [(30, 4), (35, 4)]]
GAPS_B4 = [[(20, 5), (90, 10), (150, 20)], [(60, 10)], [], [(5, 3), (40, 8), (100, 12), (170, 15)]]      # tests/test_gpu_multigap.py
N16, N22, T_OUT = 24000, 33075, 129              # (N_OUT, HOP, FADES and CHUNK: tests/cases.py, shared with test_gpu_long.py)
U = 2.0 ** -24                                   # fp32 unit roundoff


def _clips(B=4, seed=31):
    from speech_inpainting_amd import synth
    return synth.synth_wave(B, N16, seed).cuda(), synth.synth_wave(B, N22, seed + 1, sr=22050).cuda()


def _seam_spans(fade):
    """Spans placed against the compose kernel's chunk seams (multiples of CHUNK): a seam inside a rising ramp (or on the span's first
    sample at fade 0), inside a gap, a region whose FIRST sample is the first of a chunk and one whose LAST sample is the last of one."""
    return [(CHUNK + fade // 2, 300),                            # seam 2048 inside the rise [2048 - fade / 2, ...)
            (2 * CHUNK + fade + 700, 3 * CHUNK - (2 * CHUNK + fade + 700) + 50),     # seam 6144 inside the gap
            (4 * CHUNK + fade, 500),                              # region starts at sample 8192 exactly
            (6 * CHUNK - fade - 400, 400)]                        # region ends at sample 12287: its last sample closes chunk 5


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("fade", FADES)
@pytest.mark.parametrize("n22,ragged", [(N22, False), (N22 + 1, False), (N22, True)])
def test_compose_kernel_against_float64(n22, ragged, fade):
    """si_patch_compose on random orig / gen / gain with the tables of GAPS plus a clip of spans set against the chunk seams.
    weight 0 (float64): the output's int32 view equals orig's (a planted -0.0, a NaN payload and the tail m >= lim among them);
    weight 1: torch.equal with the fp32 product gain * gen; elsewhere |o - ref64| <= c * 2^-24 * (|orig| + |gain * gen|), c = 6: the
    kernel rounds 1 - w, (1 - w) * orig, gain * gen and the fma (or, uncontracted, w * g and the sum): at most five roundings, each at
    most 2^-24 relative to a term bounded by |orig| + |gain * gen|, plus one unit for the second-order terms.
    N22 = 33075 leaves rows 1 .. 3 off the 16-byte grid (scalar copy), 33076 keeps every row on it (16-byte copy + scalar tail)."""
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import native
    eng = _engine()
    dev = eng.device
    B = 5
    lens = [n22, 30001, n22, 29000, n22] if ragged else [n22] * B
    spans = G.spans22(GAPS, lens[:4]) + [_seam_spans(fade)]
    plan = eng._patch_tables(eng.plan_patch(spans, lens, fade))
    assert [len(w) for w in plan["windows"]] == [1, 2, 0, 1, len(plan["windows"][4])] and len(plan["windows"][4]) >= 1
    g = torch.Generator().manual_seed(7 + fade)
    orig = (torch.rand(B, n22, generator=g) * 2 - 1) * 0.7
    wins = plan["wins"]
    Lrow = max(w1 - w0 for _, w0, w1 in wins) * HOP
    gen = torch.tanh(torch.randn(len(wins), Lrow, generator=g))
    gain = torch.rand(B, generator=g) * 0.5 + 0.1
    w64, who = zip(*[_weights64(spans[b], plan["lim"][b], fade, n22) for b in range(B)])
    w64, who = np.stack(w64), np.stack(who)
    # plant -0.0 and a NaN with a payload where the weight is zero: in front of a region, in the tail past lim, in the clip without gaps
    assert plan["lim"][0] == min(lens[0], N_OUT) < n22
    plants = [(0, 5), (0, n22 - 2), (0, plan["lim"][0]), (2, 4097), (4, CHUNK - fade // 2 - 1 if fade else CHUNK - 1), (1, n22 - 1)]
    bits = orig.view(torch.int32)
    for i, (b, m) in enumerate(plants):
        assert w64[b, m] == 0
        bits[b, m] = -2 ** 31 if i % 2 == 0 else 0x7fc12345
    orig_d, gen_d, gain_d = orig.to(dev), gen.to(dev), gain.to(dev)
    tab = native.SpanTable(spans, dev)
    out, pcm = eng.ctx.patch_compose(orig_d, tab, plan["table"], gen_d, gain_d, sample_len=lens if ragged else None, f32=True, pcm=True)
    only_pcm = eng.ctx.patch_compose(orig_d, tab, plan["table"], gen_d, gain_d, sample_len=lens if ragged else None, f32=False, pcm=True)[1]
    ref_pcm = eng.to_int16(out)
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(pcm, ref_pcm) and torch.equal(only_pcm, ref_pcm)
    # gen at every sample, through the window of the span that owns it
    starts = [w0 * HOP for _, w0, _ in wins]
    off = np.cumsum([0] + [len(s) for s in spans])
    gsel = np.zeros((B, n22), dtype=np.float32)
    gen_np = gen.numpy()
    for b in range(B):
        for m in np.flatnonzero(w64[b]):
            wi = plan["span_win"][off[b] + who[b, m]]
            gsel[b, m] = gen_np[wi, m - starts[wi]]
    gg = gain[:, None] * torch.from_numpy(gsel)                  # the fp32 product
    zero, one = torch.from_numpy(w64 == 0), torch.from_numpy(w64 == 1)
    assert int(zero.sum()) > 0 and int(one.sum()) > 0
    assert torch.equal(out.view(torch.int32)[zero], orig.view(torch.int32)[zero])
    assert bool(zero[:, N_OUT:].all()) and bool(zero[2].all())
    assert torch.equal(out[one], gg[one])
    mid = ~zero & ~one
    if fade:
        assert int(mid.sum()) >= 2 * fade
        w = torch.from_numpy(w64)
        ref = (1 - w) * orig.double() + w * (gain[:, None].double() * torch.from_numpy(gsel).double())
        err = (out.double() - ref).abs()[mid]
        bound = (6 * U * (orig.double().abs() + gg.double().abs()))[mid]
        print(f"compose fade {fade}: max err / bound = {float((err / bound).max()):.3f} over {int(mid.sum())} samples")
        assert bool((err <= bound).all()), float((err / bound).max())
    else:
        assert int(mid.sum()) == 0
    # the chunk seams the spans of clip 4 were set against
    if fade:
        assert 0 < w64[4, CHUNK - 1] < 1 and 0 < w64[4, CHUNK] < 1                      # inside a ramp
    assert w64[4, 3 * CHUNK - 1] == 1 and w64[4, 3 * CHUNK] == 1                         # inside a gap
    assert w64[4, 4 * CHUNK - 1] == 0 and w64[4, 4 * CHUNK] > 0                          # a region's first sample
    assert w64[4, 6 * CHUNK - 1] > 0 and w64[4, 6 * CHUNK] == 0                          # a region's last sample


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("wmax", [None, 47, 48])
def test_gather_windows_against_torch_slicing(wmax):
    """Windows at w0 % 4 = 0, 1, 2, 3, clip-edge windows at both ends, rows of Wmax a multiple of 4 and not: torch.equal with the
    slices, zero past each window's own frames."""
    eng = _engine()
    B, D = 3, 80
    ext = torch.randn(B, D, T_OUT, generator=torch.Generator().manual_seed(3)).cuda()
    wins = [(0, 0, 31), (0, 44, 84), (1, 5, 45), (1, 86, 129), (2, 18, 19), (2, 23, 63), (0, 100, 129), (2, 0, 129)]
    if wmax is not None:
        wins = [(b, w0, min(w1, w0 + wmax - (i % 3))) for i, (b, w0, w1) in enumerate(wins)]
    assert {w0 % 4 for _, w0, _ in wins} == {0, 1, 2, 3}
    out = eng.ctx.gather_windows(ext, wins, wmax)
    torch.cuda.synchronize()
    assert out.shape == (len(wins), D, wmax or 129)
    for i, (b, w0, w1) in enumerate(wins):
        assert torch.equal(out[i, :, :w1 - w0], ext[b, :, w0:w1]), i
        assert bool((out[i, :, w1 - w0:] == 0).all()), i


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_windowed_route_equals_the_full_pass_route_bit_for_bit(voc):
    """patch_multigap_batch (the generator over the windows the blend regions need) against patch_from_wave on a FULL generator pass
    of the same spliced mel: torch.equal for every fade, in the fp32 and the fp16-stream vocoder; the clip without gaps is its input;
    the windows of clips 0 and 3 are a fraction of the clip."""
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import native
    eng = _engine(voc)
    wave, wave22 = _clips()
    full = None
    for fade in FADES:
        out = eng.patch_multigap_batch(wave, wave22, GAPS, fade=fade, pcm=True)
        assert "wave" not in out and out["patched"].shape == wave22.shape
        if full is None:
            full = eng.vocode(out["mel"], stretch=True)
            assert full.shape == (4, N_OUT)
        tab22 = native.SpanTable(G.spans22(out["gaps"], [N22] * 4), eng.device)
        ref, ref_pcm = eng.patch_from_wave(wave22, full, tab22, fade, pcm=True)
        torch.cuda.synchronize()
        assert torch.equal(out["patched"], ref), (fade, float((out["patched"] - ref).abs().max()))
        assert torch.equal(out["patched_pcm"], ref_pcm) and torch.equal(ref_pcm, eng.to_int16(ref))
        assert torch.equal(out["patched"][2].view(torch.int32), wave22[2].view(torch.int32))
        assert not torch.equal(out["patched"][0], wave22[0])
        wins = out["patch_windows"]
        assert wins[2] == [] and len(wins[3]) == 1 and len(wins[1]) == 2
        for b in (0, 3):
            assert 0 < sum(w1 - w0 for w0, w1 in wins[b]) < T_OUT
        # inside the gaps: exactly gain * the full pass
        gain = eng.ctx.wave_peak(wave22, tab22) / 0.95
        for b, clip in enumerate(G.spans22(out["gaps"], [N22] * 4)):
            for s, l in clip:
                e = min(s + l, N_OUT)
                assert torch.equal(out["patched"][b, s:e], gain[b] * full[b, s:e])


# ------------------------------------------------------------------------------------------------------------ 4
def test_level_follows_the_recording():
    """The clips scaled by 0.1: `patched` inside a gap is 0.1 x the unscaled run's, to the fp32 roundings of the gain.
    The clips are first snapped to the grid 10 j 2^-14, on which the fp32 product with 0.1f is EXACTLY j 2^-14 (0.1f = 0.1 (1 + 2^-26.0..),
    less than half an ulp away): then peak' = peak / 10 exactly (si_wave_peak is the front-end's own divisor: max |x| over the clip with
    its spans zeroed, asserted below against torch), x' / peak' and x / peak are the correctly rounded quotient of the same real number,
    so the normalised clips, the mel, the labels and the generator's samples are identical and only the gain differs:
        gain  = fl(peak / 0.95) = (peak / 0.95)(1 + e1),  gain' = fl(peak' / 0.95) = (peak / 9.5)(1 + e2),
        patched = fl(gain gen) = gain gen (1 + e3),        patched' = gain' gen (1 + e4),            |e_i| <= 2^-24
    => |patched' - 0.1 patched| <= 4 * 2^-24 * |0.1 patched| to first order; asserted with 5 (second-order terms, the double 0.1)."""
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import native
    eng = _engine()
    wave, wave22 = _clips(seed=55)
    snap = lambda x: torch.round(x * (2.0 ** 14 / 10)) * (10 * 2.0 ** -14)
    wave, wave22 = snap(wave), snap(wave22)
    tenth = torch.tensor(0.1, dtype=torch.float32, device=wave.device)
    wave_s, wave22_s = wave * tenth, wave22 * tenth
    assert torch.equal(wave22_s, torch.round(wave22 * (2.0 ** 14 / 10)) * 2.0 ** -14)
    spans = G.spans22(G.normalize_gaps(GAPS), [N22] * 4)
    tab22 = native.SpanTable(spans, eng.device)
    masked = wave22.clone()
    for b, clip in enumerate(spans):
        for s, l in clip:
            masked[b, s:s + l] = 0
    peak, peak_s = eng.ctx.wave_peak(wave22, tab22), eng.ctx.wave_peak(wave22_s, tab22)
    assert torch.equal(peak, masked.abs().amax(dim=1)) and torch.equal(peak_s.double() * 10, peak.double())
    a = eng.patch_multigap_batch(wave, wave22, GAPS)
    b_ = eng.patch_multigap_batch(wave_s, wave22_s, GAPS)
    torch.cuda.synchronize()
    assert torch.equal(a["mel_masked"], b_["mel_masked"])
    assert torch.equal(a["labels"], b_["labels"]), "the scaled 16 kHz clips decided other codewords: the level check needs equal labels"
    for b, clip in enumerate(spans):
        for s, l in clip:
            e = min(s + l, N_OUT)
            want = 0.1 * a["patched"][b, s:e].double()
            err = (b_["patched"][b, s:e].double() - want).abs()
            print(f"level clip {b} span {s}: max err / bound = {float((err / (5 * U * want.abs()).clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= 5 * U * want.abs() + 2.0 ** -149).all())
            assert float(want.abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------------------------ 5
def test_headline_arithmetic_end_to_end():
    """base_b4 with the gaps of the multi-gap tests, bf16 encoder / fp16 vocoder, 4 s clips (the one test at the workload's length):
    outside every blend region the output is wave22 bit for bit, inside the gaps it is gain x the full pass's wave."""
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import native, synth
    c = load_case("base_b4")
    eng = case_engine(c, "bf16", "fp16")
    wave = c["wave"].cuda()
    B, n16 = wave.shape
    n22 = n16 * 441 // 320
    wave22 = synth.synth_wave(B, n22, 72, sr=22050).cuda()
    out = eng.patch_multigap_batch(wave, wave22, GAPS_B4, pcm=True)
    full = eng.predict_multigap_batch(wave, wave22, GAPS_B4)
    torch.cuda.synchronize()
    assert torch.equal(out["labels"], full["labels"]) and torch.equal(out["mel"], full["mel"])
    spans = G.spans22(out["gaps"], [n22] * B)
    gain = eng.ctx.wave_peak(wave22, native.SpanTable(spans, eng.device)) / 0.95
    n_out = full["wave"].shape[1]
    for b in range(B):
        w = torch.from_numpy(G.blend_weights(spans[b], n22, n_out, 110))
        zero = (w == 0).cuda()
        assert torch.equal(out["patched"][b].view(torch.int32)[zero], wave22[b].view(torch.int32)[zero])
        assert int(zero.sum()) == n22 - sum(l + 220 for _, l in spans[b])
        for s, l in spans[b]:
            assert torch.equal(out["patched"][b, s:s + l], gain[b] * full["wave"][b, s:s + l])
        assert sum(w1 - w0 for w0, w1 in out["patch_windows"][b]) < n_out // HOP
    assert torch.equal(out["patched_pcm"], eng.to_int16(out["patched"]))


def test_ragged_batch_of_two_equals_each_clip_alone():
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.predict import predict_clips, predict_clips_ragged
    eng = _engine("fp16")
    n16 = [24000, 19000]
    w16 = [synth.synth_wave(1, n, 80 + i)[0].numpy() for i, n in enumerate(n16)]
    w22 = [synth.synth_wave(1, -(-n * 441 // 320), 90 + i, sr=22050)[0].numpy() for i, n in enumerate(n16)]
    gaps = [[(20, 5), (60, 10)], [(0, 3), (51, 8)]]               # (51, 8) ends at clip 1's last frame
    out = predict_clips_ragged(eng, w16, w22, gaps=gaps, patch=True, fade=110)
    assert "wave" not in out and out["patched"].shape == (2, len(w22[0]))
    for b in range(2):
        alone = predict_clips(eng, [w16[b]], [w22[b]], gaps=[gaps[b]], patch=True, fade=110)
        n = len(w22[b])
        assert torch.equal(out["patched"][b, :n], alone["patched"][0]), b
        assert not torch.equal(alone["patched"][0].cpu(), torch.from_numpy(w22[b]))
    # the single gap of mask_pos / mask_frames is one gap per clip on the same route; diagnostics keep the full passes and add `patched`
    one = predict_clips_ragged(eng, w16, w22, mask_pos=[20, 0], mask_frames=5, patch=True)
    ref = predict_clips_ragged(eng, w16, w22, gaps=[[(20, 5)], [(0, 5)]], patch=True)
    diag = predict_clips_ragged(eng, w16, w22, gaps=[[(20, 5)], [(0, 5)]], patch=True, diagnostics=True)
    torch.cuda.synchronize()
    assert torch.equal(one["patched"], ref["patched"]) and torch.equal(diag["patched"], ref["patched"])
    assert "wave" in diag and "hifi_masked" in diag


def test_stream_request_with_patch_equals_the_resident_route():
    """stream.Request(patch=True) through the request front (its patch tables staged with the gap tables) against the resident route:
    the PCM is equal and as long as each clip's own 22.05 kHz input."""
    from speech_inpainting_amd import audio, synth
    from speech_inpainting_amd.stream import Request, predict_stream
    eng = _engine()
    secs = [[1.5, 1.5, 1.5], [1.5, 1.1], [1.2, 1.2]]
    gaps = [[[(20, 5)], [], [(0, 3), (60, 10)]], [[(30, 4), (35, 4)], [(10, 6)]], None]
    reqs = []
    for r, (ss, g) in enumerate(zip(secs, gaps)):
        clips = [synth.synth_wave(1, int(s * 22050), 700 + 10 * r + i, sr=22050)[0].numpy() for i, s in enumerate(ss)]
        reqs.append(Request(clips, gaps=g, patch=True, fade=110 if r else 300, tag=r) if g is not None else
                    Request(clips, [8, 30], 5, patch=True, tag=r))
    got = list(predict_stream(eng, reqs, sr_in=22050, depth=2))
    for rq, res in zip(reqs, got):
        lens = [len(c) for c in rq.clips]
        ragged = min(lens) != max(lens)
        raw = torch.zeros(len(lens), max(lens))
        for i, c in enumerate(rq.clips):
            raw[i, :lens[i]] = torch.from_numpy(c)
        raw = raw.cuda()
        w16 = eng.resample(raw, 22050, 16000, lens=lens if ragged else None)
        n16 = [audio.resampled_len(n, 22050, 16000) for n in lens]
        g = rq.gaps if rq.gaps is not None else [[(int(p), rq.mask_frames)] for p in rq.mask_pos]
        ref = eng.patch_multigap_batch(w16, raw, g, fade=rq.fade, len16=n16 if ragged else None, len22=lens if ragged else None, pcm=True)
        torch.cuda.synchronize()
        assert torch.equal(res.labels, ref["labels"].cpu())
        for i, n in enumerate(lens):
            assert res.pcm[i].dtype == np.int16 and len(res.pcm[i]) == n
            assert np.array_equal(res.pcm[i], ref["patched_pcm"][i, :n].cpu().numpy()), (rq.tag, i)


def test_predict_entry_point_with_a_patch_key(tmp_path, monkeypatch):
    """predict.py on a YAML with a `patch:` mapping: patched.wav holds the clip's n22 samples -- the input's own outside the blend
    region, to the int16 grid -- next to the five files of the reference."""
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
    labdir = kdir / "label_dir" / "validation"
    labdir.mkdir(parents=True)
    torch.save(torch.arange(75).reshape(1, 75) % 100, labdir / "clip_labels.pt")
    n22 = N22
    w22 = synth.synth_wave(1, n22, 5, sr=22050)[0].numpy()          # 1.5 s at 22.05 kHz
    (tmp_path / "wavs").mkdir()
    pcm_in = (w22 * 32767).astype(np.int16)
    wavfile.write(tmp_path / "wavs" / "clip.wav", 22050, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/clip.wav', save_pred: '{tmp_path}/prediction'}}}}
mask: {{start_pos_in_sec: 0.5, end_pos_in_sec: 0.75}}
patch: {{fade_ms: 5}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "clip"
    for f in ("orig.wav", "masked.wav", "hifi_masked.wav", "expected_inpaint.wav", "inpainted.wav", "patched.wav"):
        assert (out / f).exists(), f
    sr, patched = wavfile.read(out / "patched.wav")
    assert sr == 22050 and patched.dtype == np.int16 and len(patched) == n22
    s, e = 8000 * 22050 // 16000, 12000 * 22050 // 16000                       # I_ea/predict.py:99-100 for 0.5 s .. 0.75 s
    keep = np.ones(n22, dtype=bool)
    keep[s - 110:e + 110] = False
    # outside the region the fp32 samples are the file's own (int16 / 32768): back on the int16 grid they are the file's samples
    assert np.array_equal(patched[keep], pcm_in[keep])
    assert not np.array_equal(patched[s:e], pcm_in[s:e])
    _, inp = wavfile.read(out / "inpainted.wav")
    assert len(inp) == N_OUT


# ------------------------------------------------------------------------------------------------------------ 6
def test_malformed_patch_tables_are_refused_before_any_launch():
    """Straight at the C ABI: each malformed table returns an error code and a message, launches nothing and leaves the outputs untouched."""
    import ctypes as C
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import native
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    B = 4
    spans = G.spans22(GAPS, [N22] * B)
    plan = eng._patch_tables(eng.plan_patch(spans, [N22] * B, 110))
    tab = native.SpanTable(spans, dev)
    wins = plan["wins"]
    Lrow = max(w1 - w0 for _, w0, w1 in wins) * HOP
    orig = torch.rand(B, N22, device=dev)
    gen = torch.rand(len(wins), Lrow, device=dev)
    out = torch.full((B, N22), 7.0, device=dev)
    pcm = torch.full((B, N22), 7, dtype=torch.int16, device=dev)
    ext = torch.rand(B, 80, T_OUT, device=dev)
    gout = torch.full((len(wins), 80, 64), 7.0, device=dev)
    rows = [(b, w0 * HOP, (w1 - w0) * HOP) for b, w0, w1 in wins]

    def refused(fn):
        ctx.profile_start(100)
        rc = fn()
        msg = ctx.lib.si_last_error(ctx._h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        torch.cuda.synchronize()
        assert rc != 0 and msg and launched == [], (rc, msg, launched)
        assert bool((out == 7.0).all()) and bool((pcm == 7).all()) and bool((gout == 7.0).all())
        return msg

    def compose(ts=None, tp=None, o=out, q=pcm, lens=None, lrow=Lrow):
        ts = tab.struct() if ts is None else ts
        tp = plan["table"].struct() if tp is None else tp
        ln = None if lens is None else np.asarray(lens, dtype=np.int32)
        return lambda: ctx.lib.si_patch_compose(ctx._h, native._ptr(orig), C.byref(ts) if ts else None, None if ln is None else ln.ctypes.data_as(C.c_void_p),
                                                C.byref(tp) if tp else None, native._ptr(gen), lrow, None, B, N22, native._ptr(o), native._ptr(q), ctx._stream())

    def table(rows_=rows, span_win=plan["span_win"], lim=plan["lim"], fade=110):
        t = native.PatchTable(rows_, span_win, lim, max(fade, 0), dev)
        st = t.struct()
        st.fade = fade
        keep.append(t)
        return st

    keep = []
    assert "both outputs" in refused(compose(o=None, q=None))
    assert "size mismatch" in refused(compose(tp=False)) and "size mismatch" in refused(compose(ts=False))
    st = plan["table"].struct()
    st.struct_size -= 8
    assert "size mismatch" in refused(compose(tp=st))
    assert "fade" in refused(compose(tp=table(fade=-1)))
    st = plan["table"].struct()
    st.lim = None
    assert "NULL" in refused(compose(tp=st))
    bad = list(rows)
    bad[0] = (B, rows[0][1], rows[0][2])
    assert "outside its clip" in refused(compose(tp=table(rows_=bad)))                      # a window of a clip that does not exist
    bad[0] = (rows[0][0], N22 - 100, rows[0][2])
    assert "outside its clip" in refused(compose(tp=table(rows_=bad)))                      # a window past the end of its clip
    assert "outside its clip" in refused(compose(lrow=Lrow - HOP))                          # a window longer than the rows of gen
    sw = list(plan["span_win"])
    sw[0] = len(wins)
    assert "names window" in refused(compose(tp=table(span_win=sw)))                        # window index out of range
    sw[0] = 1
    assert "belongs to clip" in refused(compose(tp=table(span_win=sw)))                     # a window of another clip
    bad = list(rows)
    bad[0] = (rows[0][0], rows[0][1], 20 * HOP)                                             # the row ends inside the gap's region
    assert "its window's row holds" in refused(compose(tp=table(rows_=bad)))
    bad[0] = (rows[0][0], 8820 - 50, rows[0][2])                                            # the row starts inside the rising ramp
    assert "its window's row holds" in refused(compose(tp=table(rows_=bad)))
    assert "lim" in refused(compose(tp=table(lim=[N22 + 1] + plan["lim"][1:])))
    assert "lim" in refused(compose(lens=[N_OUT - 1, N22, N22, N22]))                      # lim past the clip's own samples
    assert "batch of" in refused(compose(ts=native.SpanTable(spans[:3], dev).struct()))

    def gather(w, wmax=64):
        words = ctx.window_words(w)
        d = torch.from_numpy(words).to(dev)
        keep.append((words, d))
        return lambda: ctx.lib.si_gather_windows(ctx._h, native._ptr(ext), B, T_OUT, words.ctypes.data_as(C.c_void_p), native._ptr(d), len(w), wmax,
                                                 native._ptr(gout), ctx._stream())
    assert "names clip" in refused(gather([(B, 0, 10)]))
    assert "outside its clip" in refused(gather([(0, 100, T_OUT + 1)]))
    assert "outside its clip" in refused(gather([(0, 10, 10)]))
    assert "rows hold" in refused(gather([(0, 0, 65)]))
    # and the same calls with good tables work
    o2, q2 = ctx.patch_compose(orig, tab, plan["table"], gen, None, pcm=True)
    torch.cuda.synchronize()
    assert torch.equal(q2, eng.to_int16(o2)) and torch.equal(o2[2], orig[2])


def test_patch_with_blind_is_refused():
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.predict import predict_resident
    from speech_inpainting_amd.stream import Request, predict_stream
    eng = _engine()
    wave, wave22 = _clips(2)
    with pytest.raises(ValueError, match="blind"):
        predict_resident(eng, wave, wave22, [0, 0], 5, blind=True, patch=True)
    clips = [synth.synth_wave(1, 22050, 900 + i, sr=22050)[0].numpy() for i in range(2)]
    with pytest.raises(ValueError, match="blind"):
        list(predict_stream(eng, [Request(clips, [0, 0], 5, blind=True, patch=True)]))
    with pytest.raises(ValueError, match="raw"):
        eng.patch_multigap_batch(wave, torch.zeros(2, 80, 75, device=eng.device), [[(3, 4)], []])
    torch.cuda.synchronize()
