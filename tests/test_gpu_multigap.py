"""Several gaps per clip in ONE pass (si_*_spans entry points, engine.predict_multigap_batch, predict.py `gaps=` / `masks:`).

The reference for the whole path is the committed oracle composed here (`oracle_multigap`): the spans are zeroed on a host copy of the
raw clips, `mask_and_normalize` runs with no mask of its own, one `custom_model_forward`, then per gap the oracle's gather / arg-max /
splice, and one `extend_mel` + `generator_forward`.  fp32 bounds are those `test_fp32_matches_reference_goldens` holds the single-gap path
to; a one-gap table must reproduce the single-gap entry points bit for bit in every arithmetic mode."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests import encoder_ref as E
from tests.common import case_engine as _engine
from tests.common import load_case, rms

pytestmark = pytest.mark.gpu

torch.set_num_threads(16)

# (first 20 ms frame, frame count) per clip: 3 / 1 / 0 / 4 gaps, 83 masked frames
GAPS_B4 = [[(20, 5), (90, 10), (150, 20)], [(60, 10)], [], [(5, 3), (40, 8), (100, 12), (170, 15)]]
GAPS_TINY = {"tiny_group": [[(1, 4), (12, 6)], [(3, 3), (15, 8)], [(0, 5), (18, 7)]],
             "tiny_layer": [[(2, 3), (10, 5)], [(0, 4), (12, 6)]]}
MEL_ATOL = 2e-4          # tests/test_gpu_frontend.py: the HIP mel front-end against torch's FFT-based one


def zero_spans16(wave, gaps):
    x = wave.clone()
    for b, clip in enumerate(gaps):
        for p, l in clip:
            s, n = R.mask_samples_from_frames(p, l)
            x[b, s:s + n] = 0.0
    return x


def zero_spans22(wave22, gaps):
    x = np.array(wave22, dtype=np.float32, copy=True)
    for b, clip in enumerate(gaps):
        for p, l in clip:
            x[b, p * 320 * 22050 // 16000:(p + l) * 320 * 22050 // 16000] = 0.0      # I_ea/predict.py:99-102
    return x


def oracle_multigap(hsd, harch, gsd, varch, cb, wave16, mel, gaps, vocode=True):
    """-> dict(feats, labels (flat: clip, gap, frame), mel, wave, margin (top-two cosine margin per masked frame), values)."""
    B = wave16.shape[0]
    with torch.no_grad():
        x = R.mask_and_normalize(zero_spans16(wave16, gaps), [0] * B, [0] * B)
        feats = R.custom_model_forward(hsd, harch, x)
        mel2 = mel.clone().float()
        labels, margins, values = [], [], []
        _, cc = R.codebook_tables(cb)
        for b, clip in enumerate(sorted(g) for g in gaps):
            for p, l in clip:
                v = R.gather_masked_frames(feats[b:b + 1], [p], l)
                lab = R.codebook_argmax(v, cb)
                mel2[b:b + 1] = R.splice_centroids(mel2[b:b + 1], lab, cb, [p])
                labels.append(lab.reshape(-1))
                values.append(v.reshape(-1, v.shape[-1]))
                top = F.cosine_similarity(v.reshape(-1, 1, v.shape[-1]), cc[None], dim=-1).topk(2, dim=1).values
                margins.append(top[:, 0] - top[:, 1])
        out = {"feats": feats, "mel": mel2,
               "labels": torch.cat(labels) if labels else torch.zeros(0, dtype=torch.int64),
               "margin": torch.cat(margins) if margins else torch.zeros(0),
               "values": torch.cat(values) if values else torch.zeros(0, feats.shape[-1])}
        if vocode:
            out["wave"] = R.generator_forward(gsd, varch, R.extend_mel(mel2))[:, 0, :]
    return out


def _cpu(out):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


def _assert_fp32_bounds(tag, got, ref):
    """The bounds of test_fp32_matches_reference_goldens."""
    ef = rms(got["feats"], ref["feats"])
    em = float((got["mel"] - ref["mel"]).abs().max())
    ew = rms(got["wave"], ref["wave"])
    print(f"{tag}: feats rms err {ef:.3e} (rms {rms(ref['feats']):.3f}), labels equal {bool(torch.equal(got['labels'], ref['labels']))} "
          f"({ref['labels'].numel()} frames, {len(set(ref['labels'].tolist()))} distinct, min margin {float(ref['margin'].min()):.2e}), "
          f"mel max err {em:.3e}, wave rms err {ew:.3e}")
    assert got["feats"].shape == ref["feats"].shape
    assert ef <= 1e-4 * max(rms(ref["feats"]), 1.0)
    assert torch.equal(got["labels"], ref["labels"])
    assert em <= 1e-6
    assert ew <= 1e-4


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", ["base_b4", "tiny_group", "tiny_layer"])
def test_fp32_multigap_matches_the_composed_oracle(name):
    """3 / 1 / 0 / 4 gaps in the four base_b4 clips (83 masked frames, none excluded: the oracle's smallest top-two margin over them
    is 2.3e-3, three orders above the fp32 feature error) and two gaps per clip of the tiny cases (both conv0 flavours)."""
    c = load_case(name)
    gaps = GAPS_B4 if name == "base_b4" else GAPS_TINY[name]
    ref = oracle_multigap(c["hsd"], c["harch"], c["gsd"], c["varch"], c["cb"], c["wave"], c["mel"], gaps)
    assert float(ref["margin"].min()) >= 1e-4, "move the gap: the reference itself has a near-tie here"
    eng = _engine(c)
    out = _cpu(eng.predict_multigap_batch(c["wave"].cuda(), c["mel"].cuda(), gaps))
    n = [sum(l for _, l in g) for g in gaps]
    assert out["label_off"] == [sum(n[:i]) for i in range(len(n) + 1)] and out["labels"].shape == (sum(n),)
    if name == "base_b4":
        assert out["labels"].numel() == 83
    _assert_fp32_bounds(name, out, ref)


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("enc,voc", [("fp32", "fp32"), ("bf16", "fp16"), ("bf16", "bf16x3")])
@pytest.mark.parametrize("name", ["base_4s", "base_b4"])
def test_one_gap_per_clip_equals_the_single_gap_path(name, enc, voc):
    """A span table with exactly one gap per clip (equal lengths) against predict_batch: feats, labels, mel and wave bit-identical."""
    c = load_case(name)
    m = c["meta"]
    eng = _engine(c, enc, voc)
    wave, mel = c["wave"].cuda(), c["mel"].cuda()
    pos = torch.tensor(c["frame_pos"], dtype=torch.int32, device="cuda")
    one = eng.predict_batch(wave, mel, pos, m["lm"])
    got = eng.predict_multigap_batch(wave, mel, [[(p, m["lm"])] for p in c["frame_pos"]])
    torch.cuda.synchronize()
    assert torch.equal(got["feats"], one["feats"]), float((got["feats"] - one["feats"]).abs().max())
    assert torch.equal(got["labels"].view(m["B"], m["lm"]), one["labels"])
    assert torch.equal(got["mel"], one["mel"])
    assert torch.equal(got["wave"], one["wave"]), float((got["wave"] - one["wave"]).abs().max())
    assert not torch.equal(one["feats"], eng.encode(wave))                     # (the mask does reach the features)


# ------------------------------------------------------------------------------------------------------------ 3
def test_clips_of_a_multigap_batch_equal_themselves_alone():
    """Headline arithmetic (bf16 encoder, fp16 vocoder): each clip of the batch of test 1 is bit-identical to that clip run alone with
    its own gaps; the clip without gaps equals `encode` without a mask and `vocode` of its unmodified mel."""
    c = load_case("base_b4")
    eng = _engine(c, "bf16", "fp16")
    wave, mel = c["wave"].cuda(), c["mel"].cuda()
    out = eng.predict_multigap_batch(wave, mel, GAPS_B4)
    off = out["label_off"]
    for b in range(4):
        alone = eng.predict_multigap_batch(wave[b:b + 1].contiguous(), mel[b:b + 1].contiguous(), [GAPS_B4[b]])
        torch.cuda.synchronize()
        assert torch.equal(out["feats"][b], alone["feats"][0]), b
        assert torch.equal(out["labels"][off[b]:off[b + 1]], alone["labels"]), b
        assert torch.equal(out["mel"][b], alone["mel"][0]), b
        assert torch.equal(out["wave"][b], alone["wave"][0]), b
    assert torch.equal(out["feats"][2], eng.encode(wave[2:3].contiguous())[0])
    assert torch.equal(out["mel"][2], mel[2])
    assert torch.equal(out["wave"][2], eng.vocode(mel[2:3].contiguous())[0])
    assert int(out["labels"].min()) >= 0


# ------------------------------------------------------------------------------------------------------------ 4
def _ragged_clips():
    from speech_inpainting_amd import synth
    g = torch.Generator().manual_seed(4321)
    secs = (4.0 + 6.0 * torch.rand(4, generator=g)).tolist()                    # U[4 s, 10 s]
    w16 = [synth.synth_wave(1, int(round(s * 16000)), 300 + i)[0].numpy() for i, s in enumerate(secs)]
    w22 = [synth.synth_wave(1, -(-len(w) * 441 // 320), 800 + i, sr=22050)[0].numpy() for i, w in enumerate(w16)]
    return secs, w16, w22


def _ragged_gaps(harch, w16, w22, seed=11):
    """(seed 11: the oracle's smallest top-two margin is 4.4e-2 on the shortest clip and 1.5e-3 on the longest; seeds 7, 23 and 99 put a
    gap of the longest clip on a frame whose margin is 0.8 .. 1.7e-4 -- the gap is moved, no frame is excluded)"""
    from speech_inpainting_amd.arch import mel_frames
    g = torch.Generator().manual_seed(seed)
    gaps = []
    for i, (a, b) in enumerate(zip(w16, w22)):
        lim = min(harch.num_frames(len(a)), mel_frames(len(b)))
        k = 2 + i % 2                                                           # two or three gaps
        seg = lim // k
        gaps.append([(j * seg + int(torch.randint(2, seg - 30, (1,), generator=g)), int(torch.randint(3, 20, (1,), generator=g)))
                     for j in range(k)])
    gaps[-1][-1] = (min(harch.num_frames(len(w16[-1])), mel_frames(len(w22[-1]))) - 6, 6)      # one gap ends at the clip's last frame
    return gaps


@pytest.mark.parametrize("enc,voc", [("fp32", "fp32"), ("bf16", "fp16")])
def test_ragged_multigap_batch(enc, voc):
    """Four clips of different lengths (U[4 s, 10 s], seeded), two or three gaps each, through the ragged route (raw 22.05 kHz clips:
    the mel front-end zeroes the 22.05 kHz spans): every clip bit-identical to itself alone through the uniform route; in fp32 the
    shortest and the longest clip are held to the oracle at test 1's bounds."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.engine import InpaintingEngine
    from speech_inpainting_amd.predict import predict_clips, predict_clips_ragged
    harch, varch = HubertArch.base(), VocoderArch.v1()
    hsd, gsd, cb = synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100)
    eng = InpaintingEngine(harch, varch, 100, "cuda:0", enc, voc).load_state(hsd, gsd, cb)
    secs, w16, w22 = _ragged_clips()
    gaps = _ragged_gaps(harch, w16, w22)
    assert len({len(w) for w in w16}) == 4 and sorted(len(g) for g in gaps) == [2, 2, 3, 3]
    out = predict_clips_ragged(eng, w16, w22, gaps=gaps)
    off = out["label_off"]
    for i in range(4):
        alone = predict_clips(eng, [w16[i]], [w22[i]], gaps=[gaps[i]])
        torch.cuda.synchronize()
        T, Tm, nw = out["frames"][i], out["mel_len"][i], out["wave_len"][i]
        assert alone["feats"].shape[1] == T and alone["mel"].shape[2] == Tm and alone["wave"].shape[1] == nw
        assert torch.equal(out["feats"][i, :T], alone["feats"][0]), (i, "feats")
        assert torch.equal(out["labels"][off[i]:off[i + 1]], alone["labels"]), (i, "labels")
        assert torch.equal(out["mel"][i, :, :Tm], alone["mel"][0]), (i, "mel")
        assert torch.equal(out["wave"][i, :nw], alone["wave"][0]), (i, "wave")
        assert not out["wave"][i, nw:].any() and not out["feats"][i, T:].any()
    if enc != "fp32":
        return
    # the oracle: its own FFT-based mel of the pre-zeroed 22.05 kHz clips goes in through `mel_len=` (the same ragged route after the
    # front-end), so the WHOLE spliced mel is held to 1e-6 as in test 1; the HIP front-end on these spans is held to the oracle's mel
    # at tests/test_gpu_frontend.py's tolerance on the columns that are not spliced
    mels = [R.masked_mel(zero_spans22(w22[i][None], [gaps[i]]), None, None) for i in range(4)]
    mlen = [m.shape[2] for m in mels]
    assert mlen == out["mel_len"]
    mel_pad = torch.zeros(4, mels[0].shape[1], max(mlen))
    w16_pad = torch.zeros(4, max(len(w) for w in w16))
    for i in range(4):
        mel_pad[i, :, :mlen[i]] = mels[i][0]
        w16_pad[i, :len(w16[i])] = torch.from_numpy(w16[i])
    om = eng.predict_multigap_batch(w16_pad.cuda(), mel_pad.cuda(), gaps, len16=[len(w) for w in w16], mel_len=mlen)
    assert om["label_off"] == off
    for i in (min(range(4), key=lambda k: secs[k]), max(range(4), key=lambda k: secs[k])):
        ref = oracle_multigap(hsd, harch, gsd, varch, cb, torch.from_numpy(w16[i])[None], mels[i], [gaps[i]])
        assert float(ref["margin"].min()) >= 1e-4, "move the gap: the reference itself has a near-tie here"
        T, Tm, nw = om["frames"][i], om["mel_len"][i], om["wave_len"][i]
        got = {"feats": om["feats"][i:i + 1, :T].cpu(), "labels": om["labels"][off[i]:off[i + 1]].cpu(),
               "mel": om["mel"][i:i + 1, :, :Tm].cpu(), "wave": om["wave"][i:i + 1, :nw].cpu()}
        _assert_fp32_bounds(f"ragged clip {i} ({secs[i]:.2f} s, gaps {gaps[i]})", got, ref)
        cols = torch.zeros(Tm, dtype=torch.bool)
        for p, l in gaps[i]:
            cols[p:p + l] = True
        d = (out["mel"][i, :, :Tm].cpu() - ref["mel"][0]).abs()
        print(f"    raw 22.05 kHz route: labels equal {bool(torch.equal(out['labels'][off[i]:off[i + 1]].cpu(), ref['labels']))}, "
              f"front-end mel max err {float(d[:, ~cols].max()):.3e}")
        assert torch.equal(out["labels"][off[i]:off[i + 1]].cpu(), ref["labels"])
        assert float(d[:, cols].max()) <= 1e-6 and float(d[:, ~cols].max()) <= MEL_ATOL


# ------------------------------------------------------------------------------------------------------------ 5
def test_headline_arithmetic_on_the_gaps_of_test_1():
    """bf16 encoder + fp16 vocoder on the 83 frames of test 1: every flipped label is a near-tie of the REFERENCE's own cosines (its
    margin <= 2 |u_ref - u_got| + 1e-6, the bound of test_bf16_labels_flip_only_where_...), agreement >= 0.6 (the floor that test
    asserts for these weights and this arithmetic), waveform <= 1e-3 rms against the oracle's vocoder on this run's spliced mel, and
    the first / last 2048 samples (which no gap of test 1 reaches) <= 1e-3 against the oracle's waveform."""
    c = load_case("base_b4")
    ref = oracle_multigap(c["hsd"], c["harch"], c["gsd"], c["varch"], c["cb"], c["wave"], c["mel"], GAPS_B4)
    eng = _engine(c, "bf16", "fp16")
    out = _cpu(eng.predict_multigap_batch(c["wave"].cuda(), c["mel"].cuda(), GAPS_B4))
    v_got = torch.cat([out["feats"][b, p:p + l] for b, g in enumerate(GAPS_B4) for p, l in g])
    v_ref = ref["values"]
    _, cc = R.codebook_tables(c["cb"])
    sim = F.cosine_similarity(v_ref[:, None, :], cc[None], dim=-1)
    want, got = ref["labels"], out["labels"]
    du = (F.normalize(v_ref, dim=1) - F.normalize(v_got, dim=1)).norm(dim=1)
    flipped = (want != got).nonzero().reshape(-1).tolist()
    agree = 1.0 - len(flipped) / want.numel()
    print(f"multi-gap headline arithmetic: agreement {agree:.3f} ({len(flipped)} of {want.numel()} flipped), unit-feature shift median "
          f"{float(du.median()):.3e} max {float(du.max()):.3e}")
    for i in flipped:
        margin = float(sim[i, want[i]] - sim[i, got[i]])
        print(f"    frame {i}: reference label {int(want[i])} -> {int(got[i])}, fp32 margin {margin:.3e}, bound {2 * float(du[i]):.3e}")
        assert 0.0 <= margin <= 2.0 * float(du[i]) + 1e-6
    assert agree >= 0.6
    assert bool(torch.isfinite(out["wave"]).all())
    ref2 = R.generator_forward(c["gsd"], c["varch"], R.extend_mel(out["mel"]))[:, 0, :]
    err2 = rms(out["wave"], ref2)
    head = max(rms(out["wave"][:, :2048], ref["wave"][:, :2048]), rms(out["wave"][:, -2048:], ref["wave"][:, -2048:]))
    print(f"multi-gap headline arithmetic: waveform vs the oracle's vocoder on this run's mel {err2:.3e}; head / tail vs the oracle {head:.3e}")
    assert err2 <= 1e-3 and head <= 1e-3


# ------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_windowed_passes_over_merged_windows_equal_full_passes(voc):
    """diagnostics=True with the gaps of test 1 (+ a fifth clip whose two gaps (90, 10), (104, 6) are close enough that their
    windows merge) and given target labels: one full generator pass, `wave` and `expected_inpaint` from windowed passes over the
    merged windows -- bit-identical to full passes, in the fp32 and the fp16-stream vocoder."""
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.engine import InpaintingEngine
    from speech_inpainting_amd.predict import predict_resident
    harch, varch = HubertArch.tiny(), VocoderArch.v1()
    eng = InpaintingEngine(harch, varch, 100, "cuda:0", "fp32", voc).load_state(
        synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100))
    gaps = GAPS_B4 + [[(90, 10), (104, 6)]]
    B, n16 = 5, 64000
    n22 = n16 * 441 // 320
    wave = synth.synth_wave(B, n16, 71).cuda()
    wave22 = synth.synth_wave(B, n22, 72, sr=22050).cuda()
    nf = sum(l for g in gaps for _, l in g)
    tgt = torch.randint(0, 100, (nf,), generator=torch.Generator().manual_seed(3))
    out = predict_resident(eng, wave, wave22, gaps=gaps, diagnostics=True, target_labels=tgt)
    full_inp = eng.vocode(out["mel"], stretch=True)
    full_masked = eng.vocode(out["mel_masked"], stretch=True)
    exp = out["mel_masked"].clone()
    eng.splice_labels_spans(tgt.cuda(), out["frame_clip"], out["frame_pos"], exp)
    full_exp = eng.vocode(exp, stretch=True)
    torch.cuda.synchronize()
    assert not torch.equal(full_inp, full_masked) and not torch.equal(full_exp, full_masked)
    assert torch.equal(out["hifi_masked"], full_masked)
    assert torch.equal(out["wave"], full_inp), float((out["wave"] - full_inp).abs().max())
    assert torch.equal(out["expected_inpaint"], full_exp), float((out["expected_inpaint"] - full_exp).abs().max())
    # given labels land where the table says: column p + j of clip b holds the raw centroid of its label
    cb = synth.synth_codebook(100)
    k = 0
    for b, g in enumerate(gaps):
        for p, l in g:
            assert torch.equal(exp[b, :, p:p + l].cpu(), cb[tgt[k:k + l]].T)
            k += l
    # the merged window, and windows that are a fraction of the clip
    Tout = out["mel"].shape[2] * 441 // 256
    Rf = -(-eng.receptive_radius() // 256)
    assert len(G.plan_windows(gaps[4], Tout, Rf)) == 1 and len(G.plan_windows(gaps[3], Tout, Rf)) >= 2
    assert G.plan_windows(gaps[2], Tout, Rf) == []
    # the metrics over the frame table against the oracle's loss on the same frames
    vals = torch.cat([out["feats"][b, p:p + l] for b, g in enumerate(gaps) for p, l in g]).cpu()
    loss, pred, cpt = R.cos_sim_loss(vals[None], tgt[None], cb)
    assert abs(float(out["loss"]) - float(loss)) <= 1e-4 * max(1.0, abs(float(loss)))
    assert float((out["cos_pred_target"].cpu() - cpt).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------ 7
def _edge_clip(N, seed):
    """A clip and spans at the edges the loaders have: sample 0, the last sample, 4-sample vector boundaries (on and across), the
    conv0_apply row-block boundary (64 rows = sample 320), the conv0 chunk boundary (SI_C0_TCH = 512 rows = sample 2560, with two
    TOUCHING spans meeting on it; [2560, 2570) covers conv0 row 512 whole).  Samples next to every span edge are large, so that a
    span off by one sample moves the clip's mean and variance by 1e-4 relative."""
    from speech_inpainting_amd import synth
    x = synth.synth_wave(1, N, seed)[0].clone()
    spans = [(0, 7), (318, 5), (1024, 8), (2046, 5), (2555, 5), (2560, 10), (N - 5, 5)]
    for s, l in spans:
        for i, v in ((s - 1, 0.9), (s, -0.8), (s + l - 1, 0.85), (s + l, -0.95)):
            if 0 <= i < N:
                x[i] = v
    return x, spans


def _normalised_operands(x, spans):
    """The fp32 operands conv0 sees: zero mask, statistics in float64 (wave_stats), rounded to fp32, (x - mean) * rstd in fp32."""
    xm = x.clone()
    for s, l in spans:
        xm[s:s + l] = 0.0
    d = xm.double()
    mean = d.mean()
    var = (d * d).mean() - mean * mean
    rstd = 1.0 / torch.sqrt(var + 1e-7)
    return (xm - mean.float()) * rstd.float(), float(mean), float(rstd)


@pytest.mark.parametrize("flavour", ["group", "layer"])
@pytest.mark.parametrize("N", [6000, 6003])
def test_multispan_encoder_loaders_against_float64(flavour, N):
    """wave_stats, conv0_lagsums and both conv0 apply flavours with a span table, through the `conv0` tap of an fp32 encoder, against
    float64 references with the bounds tests/encoder_ref.py derives (conv0 + GroupNorm + GELU; conv0 + bias = a 10-term fp32 sum).
    N = 6000 takes the 16-byte loads of wave_stats, 6003 its scalar loop.  Row 512 of the layer flavour lies wholly in a span: its
    value is bias - mean * rstd * sum(w), the statistics themselves."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.engine import InpaintingEngine
    from speech_inpainting_amd.native import SpanTable
    kw = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True) if flavour == "layer" else {}
    harch = HubertArch.tiny(**kw)
    hsd = synth.synth_hubert_state(harch, 31)
    eng = InpaintingEngine(harch, VocoderArch.tiny(), 50, "cuda:0").load_state(hsd, synth.synth_generator_state(VocoderArch.tiny()),
                                                                                 synth.synth_codebook(50))
    x0, spans0 = _edge_clip(N, 5)
    x1 = synth.synth_wave(1, N, 6)[0]
    wave = torch.stack([x0, x1, x0]).cuda()                                   # clip 1: no span; clip 2: one span only
    table = [spans0, [], [spans0[3]]]
    L1, C = harch.feat_lengths(N)[1], harch.conv_dim[0]
    cap = {"conv0": 3 * L1 * C}
    eng.ctx.clear_captures()
    caps = eng.ctx.capture(list(cap), capacity=cap)
    feats = eng.encode(wave, spans=SpanTable(table, eng.device))
    torch.cuda.synchronize()
    y = caps["conv0"].cpu().view(3, L1, C)
    eng.ctx.clear_captures()
    assert bool(torch.isfinite(feats).all())
    pre = "base_model.feature_extractor.conv_layers.0."
    w = hsd[pre + "conv.weight"][:, 0, :]
    for b in range(3):
        xh, mean, rstd = _normalised_operands(wave[b].cpu(), table[b])
        rows = E.conv_rows(xh.double()[:, None], 10, 5, torch.arange(L1))
        if flavour == "group":
            ref, bound = E.conv0_groupnorm_ref(rows, w, hsd[pre + "layer_norm.weight"], hsd[pre + "layer_norm.bias"])
        else:
            ref, bound = E.linear_ref(rows, w, hsd[pre + "conv.bias"], round_w=False)
        r = E.check_f32(y[b], ref, bound)
        print("   " + E.fmt(f"conv0 ({flavour}) with {len(table[b])} spans, N = {N}, clip {b}", r))
        assert r["bad"] == 0, E.fmt(f"clip {b}", r)
        if flavour == "layer" and b == 0:
            want = hsd[pre + "conv.bias"].double() - mean * rstd * w.double().sum(1)
            assert float((y[0, 512].double() - want).abs().max()) <= float(bound[512].max()) + 4 * E.U * float(want.abs().max())
    # the single-span kernels on the one-span clip: the same bits
    s, l = table[2][0]
    one = eng.encode(wave[2:3].contiguous(), torch.tensor([s], dtype=torch.int32, device="cuda"), torch.tensor([l], dtype=torch.int32, device="cuda"))
    assert torch.equal(one[0], feats[2])


@pytest.mark.parametrize("n22", [22064, 22063])
def test_multispan_mel_frontend_against_the_oracle(n22):
    """wave_peak and mel_frames with a span table against the oracle's mel of the pre-zeroed clips, at tests/test_gpu_frontend.py's
    tolerances.  Spans at sample 0, at the last sample, on and across a 4-sample vector boundary, over the sample the first frame's
    reflection turns on (312 = the reflect pad) and inside the part the last frame reads reflected; the clip's largest sample lies
    INSIDE a span (the peak must not see it).  n22 = 22064 takes wave_peak's 16-byte loads, 22063 its scalar loop."""
    from speech_inpainting_amd import native, synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch, mel_frames
    ctx = native.NativeContext(native.make_desc(HubertArch.tiny(), VocoderArch.tiny(), 10), torch.device("cuda:0"))
    B = 3
    w = synth.synth_wave(B, n22, 11, sr=22050).numpy() * np.array([[0.3], [1.7], [0.05]], dtype=np.float32)
    spans = [[(0, 5), (300, 20), (1024, 8), (2046, 5), (9000, 3000), (n22 - 320, 15), (n22 - 3, 3)], [], [(1, 1), (n22 - 700, 699)]]
    w[0, 1026] = 5.0
    w[0, 10000] = -7.0
    w[2, n22 - 100] = 3.0
    z = w.copy()
    for b, clip in enumerate(spans):
        for s, l in clip:
            z[b, s:s + l] = 0.0
    ref = R.masked_mel(z, None, None)
    got = ctx.mel_frontend_spans(torch.from_numpy(w).cuda(), native.SpanTable(spans, torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (B, 80, mel_frames(n22))
    err = (got.cpu() - ref).abs()
    print(f"multi-span mel front-end, n22 = {n22}: max err {float(err.max()):.3e}, mean {float(err.mean()):.3e}")
    assert float(err.max()) <= MEL_ATOL, float(err.max())
    assert float(err.mean()) <= 2e-5, float(err.mean())
    # one span per clip through the table = the single-span entry point, bit for bit
    s1 = [(300, 20), (0, 0), (n22 - 700, 699)]
    a = ctx.mel_frontend_spans(torch.from_numpy(w).cuda(), native.SpanTable([[s] for s in s1], torch.device("cuda:0")))
    b = ctx.mel_frontend(torch.from_numpy(w).cuda(), torch.tensor([s for s, _ in s1], dtype=torch.int32, device="cuda"),
                         torch.tensor([s + l for s, l in s1], dtype=torch.int32, device="cuda"))
    assert torch.equal(a, b)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ 8
def test_bad_span_tables_are_refused_before_any_launch():
    """Straight at the C ABI: more spans than SI_MAX_SPANS, an overlapping table, an unsorted one, a table for another batch size, a
    wrong struct size and NULL offsets each return an error code and a message, launch nothing and leave the output untouched."""
    import ctypes as C
    from speech_inpainting_amd import native
    c = load_case("tiny_group")
    eng = _engine(c)
    ctx = eng.ctx
    wave = c["wave"].cuda()
    B, N = wave.shape
    dev = torch.device("cuda:0")
    ok = native.SpanTable([[(100, 50), (150, 10)], [], [(0, 5)]], dev)
    feats_ok = ctx.hubert_forward_spans(wave, ok)
    torch.cuda.synchronize()
    out = torch.full_like(feats_ok, 7.0)
    ws = ctx.workspace(B, N, 0)
    mel_out = torch.full((B, 80, ctx.mel_frames(N)), 7.0, device=dev)
    wsm = ctx._mel_workspace(B, N)

    def call(st, which="enc"):
        ctx.profile_start(100)
        if which == "enc":
            rc = ctx.lib.si_hubert_forward_spans(ctx._h, native._ptr(wave), C.byref(st) if st is not None else None, None, 1, B, N,
                                                 native._ptr(out), native._ptr(ws), ws.numel(), ctx._stream())
        else:
            rc = ctx.lib.si_mel_frontend_spans(ctx._h, native._ptr(wave), C.byref(st) if st is not None else None, None, 1, B, N,
                                               native._ptr(mel_out), native._ptr(wsm), wsm.numel(), ctx._stream())
        msg = ctx.lib.si_last_error(ctx._h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        torch.cuda.synchronize()
        assert rc != 0 and msg and launched == [], (rc, msg, launched)
        assert bool((out == 7.0).all()) and bool((mel_out == 7.0).all())
        return msg

    many = native.SpanTable([[(10 * i, 5) for i in range(native.SI_MAX_SPANS + 1)], [], []], dev)
    for which in ("enc", "mel"):
        assert "SI_MAX_SPANS" in call(many.struct(), which)
        assert "overlaps" in call(native.SpanTable([[(100, 50), (149, 10)], [], []], dev).struct(), which)
        assert "overlaps or precedes" in call(native.SpanTable([[(500, 50), (100, 10)], [], []], dev).struct(), which)
        assert "batch of" in call(native.SpanTable([[(100, 50)], []], dev).struct(), which)
        st = ok.struct()
        st.struct_size -= 8
        assert "size mismatch" in call(st, which)
        assert "size mismatch" in call(None, which)
        st = ok.struct()
        st.host_off = None
        assert "NULL offsets" in call(st, which)
        st = ok.struct()
        st.span_off = None
        assert "NULL offsets" in call(st, which)
    # the Python layer refuses the same before it builds a table, naming clip and gap
    with pytest.raises(ValueError, match="clip 0"):
        eng.predict_multigap_batch(wave, c["mel"].cuda(), [[(0, 3), (2, 3)], [], []])
    with pytest.raises(ValueError, match="clip 1"):
        eng.predict_multigap_batch(wave, c["mel"].cuda(), [[], [(20, 6)], []])           # min(T, Tm) = 25
    # and the context still works
    assert torch.equal(ctx.hubert_forward_spans(wave, ok), feats_ok)


# ------------------------------------------------------------------------------------------------------------ 9
def test_predict_entry_point_with_a_masks_list(tmp_path, monkeypatch):
    """predict.py on a YAML with a `masks:` list: the five wavs are written, masked.wav is zero exactly on the union of the
    reference's spans (I_ea/predict.py:133 per gap), and inpainted.wav is the oracle's multi-gap result to within int16 rounding."""
    import joblib
    from scipy.io import wavfile
    from sklearn.cluster import MiniBatchKMeans
    from speech_inpainting_amd import audio, synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.config import load_predict_config
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
    torch.save(torch.arange(150).reshape(1, 150) % 100, labdir / "clip_labels.pt")
    w22 = synth.synth_wave(1, 66150, 5, sr=22050)[0].numpy()          # 3 s at 22.05 kHz
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "clip.wav", 22050, (w22 * 32767).astype(np.int16))
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/clip.wav', save_pred: '{tmp_path}/prediction'}}}}
masks:
  - {{start_pos_in_sec: 2.0, end_pos_in_sec: 2.25}}
  - {{start_pos_in_sec: 0.5, end_pos_in_sec: 0.75}}
  - {{start_pos_in_sec: 1.25, end_pos_in_sec: 1.5}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "clip"
    for f in ("orig.wav", "masked.wav", "hifi_masked.wav", "expected_inpaint.wav", "inpainted.wav"):
        assert (out / f).exists(), f
    cfg = load_predict_config(str(tmp_path / "predict.yaml"))
    gaps = cfg.gaps
    assert gaps == [(25, 12), (62, 12), (100, 12)]
    sr16, masked = wavfile.read(out / "masked.wav")
    _, orig = wavfile.read(out / "orig.wav")
    union = np.zeros(len(masked), dtype=bool)
    for p, l in gaps:
        union[p * 320 + 80:(p + l) * 320 + 79 - 80] = True                         # I_ea/predict.py:133
    assert sr16 == 16000 and not masked[union].any()
    assert np.array_equal(masked[~union], orig[~union]) and orig[union].any()
    # the oracle on the same glue
    raw, _ = audio.read_wav(str(tmp_path / "wavs" / "clip.wav"))
    w16 = R.resample_kaiser_best(raw, 22050, 16000).astype(np.float32)
    z22 = np.array(raw, dtype=np.float32, copy=True)[None]
    for a, b in cfg.spans22:
        z22[0, a:b] = 0.0
    mel = R.masked_mel(z22, None, None)
    ref = oracle_multigap(hsd, harch, gsd, varch, cb, torch.from_numpy(w16)[None], mel, [gaps])
    sr, pcm = wavfile.read(out / "inpainted.wav")
    ref_pcm = audio.to_int16_pcm(ref["wave"][0])
    assert sr == 22050 and pcm.dtype == np.int16 and pcm.shape == ref_pcm.shape
    diff = np.abs(pcm.astype(np.int32) - ref_pcm.astype(np.int32))
    assert diff.max() <= 2 and (diff > 1).mean() < 0.001, (diff.max(), (diff > 0).mean())
