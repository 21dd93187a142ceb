"""Several gaps per clip through the request front (speech_inpainting_amd/stream.py: the gap tables are staged in pinned memory and
cross on the copy stream with the clips) and through the ragged diagnostics route: both must return exactly what the un-pipelined /
full-pass calls return."""
import numpy as np
import pytest
import torch

from tests.harness import build_engine

pytestmark = pytest.mark.gpu


def _engine(enc="fp32", voc="fp32"):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.tiny(), 50, enc, voc)


# (seconds per clip, gaps per clip): uniform and ragged batches, 0 .. 3 gaps per clip, a request without gaps between them, batch sizes
# and table sizes that differ from one use of a slot to the next
REQUESTS = [
    ([1.2, 1.2, 1.2], [[(3, 4), (20, 6)], [], [(0, 2), (10, 3), (30, 5)]]),
    ([1.0, 2.3, 1.6, 0.9], [[(5, 5)], [(2, 3), (40, 10), (80, 7)], [(10, 4), (50, 6)], []]),
    ([1.5, 1.5], None),
    ([2.0, 1.1, 1.7], [[(0, 3), (3, 4), (60, 12)], [(30, 8)], [(7, 2), (25, 2)]]),
    ([0.8] * 5, [[(4 + i, 3), (20 + 2 * i, 4)] for i in range(5)]),
    ([1.3, 1.3], [[], []]),
]


@pytest.mark.parametrize("enc,voc", [("fp32", "fp32"), ("bf16", "fp16")])
def test_stream_front_with_gaps_equals_the_unpipelined_path(enc, voc):
    """Six requests through predict_stream (depth 2: every slot is reused with other shapes and other table sizes) against, per
    request, engine.resample -> predict_clips / predict_clips_ragged(gaps=) -> audio.to_int16_pcm: labels, label_off and PCM equal."""
    from speech_inpainting_amd import audio, synth
    from speech_inpainting_amd.predict import predict_clips, predict_clips_ragged
    from speech_inpainting_amd.stream import Request, predict_stream
    eng = _engine(enc, voc)
    reqs = []
    for r, (secs, gaps) in enumerate(REQUESTS):
        clips = [synth.synth_wave(1, int(s * 22050), 500 + 10 * r + i, sr=22050)[0].numpy() for i, s in enumerate(secs)]
        if gaps is None:
            reqs.append(Request(clips, [8 + 3 * i for i in range(len(secs))], 5, tag=r))
        else:
            reqs.append(Request(clips, gaps=gaps, tag=r))
    got = list(predict_stream(eng, reqs, sr_in=22050, depth=2))
    assert [g.tag for g in got] == list(range(len(REQUESTS)))
    for rq, g in zip(reqs, got):
        lens = [len(c) for c in rq.clips]
        raw = torch.zeros(len(lens), max(lens))
        for i, c in enumerate(rq.clips):
            raw[i, :lens[i]] = torch.from_numpy(c)
        ragged = min(lens) != max(lens)
        w16 = eng.resample(raw.cuda(), 22050, 16000, lens=lens if ragged else None).cpu().numpy()
        n16 = [audio.resampled_len(n, 22050, 16000) for n in lens]
        a16 = [w16[i, :n16[i]] for i in range(len(lens))]
        kw = dict(gaps=rq.gaps) if rq.gaps is not None else dict(mask_pos=rq.mask_pos, mask_frames=rq.mask_frames)
        if ragged:
            ref = predict_clips_ragged(eng, a16, list(rq.clips), **kw)
            waves = [ref["wave"][i, :ref["wave_len"][i]] for i in range(len(lens))]
        else:
            ref = predict_clips(eng, a16, list(rq.clips), **kw)
            waves = [ref["wave"][i] for i in range(len(lens))]
        assert g.labels.shape == ref["labels"].shape and torch.equal(g.labels, ref["labels"].cpu()), rq.tag
        if rq.gaps is not None:
            n = [sum(l for _, l in clip) for clip in rq.gaps]
            assert g.label_off == ref["label_off"] == [sum(n[:i]) for i in range(len(n) + 1)], rq.tag
        else:
            assert g.label_off is None
        for i in range(len(lens)):
            assert g.pcm[i].dtype == np.int16 and np.array_equal(g.pcm[i], audio.to_int16_pcm(waves[i])), (rq.tag, i)


def test_stream_front_refuses_bad_gaps_and_blind_with_gaps():
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.stream import Request, predict_stream
    eng = _engine()
    clips = [synth.synth_wave(1, 22050, 900 + i, sr=22050)[0].numpy() for i in range(2)]
    with pytest.raises(ValueError, match="clip 1: gap 1"):
        list(predict_stream(eng, [Request(clips, gaps=[[(3, 4)], [(5, 5), (8, 2)]])]))
    with pytest.raises(ValueError, match="blind"):
        list(predict_stream(eng, [Request(clips, blind=True, gaps=[[(3, 4)], []])]))
    torch.cuda.synchronize()


def test_stream_front_refuses_a_malformed_gap_before_it_sizes_a_slot():
    """A gap that is not a (first frame, frame count) pair is refused with the ValueError that names clip and gap, and the slot's
    pinned buffers are the ones the request before it left (nothing was resized for the refused request)."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.stream import Request, RequestFront
    eng = _engine()
    clips = [synth.synth_wave(1, 22050, 900 + i, sr=22050)[0].numpy() for i in range(2)]
    front = RequestFront(eng, sr_in=22050, depth=1)
    assert len(list(front.run([Request(clips, gaps=[[(3, 4)], [(20, 2)]])]))) == 1
    slot = front.slots[0]
    before = (slot.pin_tab.data_ptr(), slot.pin_tab.numel(), slot.pin_lab.data_ptr(), slot.pin_lab.numel())
    with pytest.raises(ValueError, match="clip 1: gap 2"):
        list(front.run([Request(clips, gaps=[[(3, 4)], [(5, 5), (12, 30), (44, 4, 1)]])]))
    with pytest.raises(ValueError, match="clip 0: gap 0"):
        list(front.run([Request(clips, gaps=[[(30, 4000)], [(0, 20)]])]))          # past the end, with a frame count that would size a large label buffer
    assert before == (slot.pin_tab.data_ptr(), slot.pin_tab.numel(), slot.pin_lab.data_ptr(), slot.pin_lab.numel())
    torch.cuda.synchronize()


@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_ragged_diagnostics_over_windows_equal_full_passes(voc):
    """predict_clips_ragged(gaps=, diagnostics=True, target_labels=) on three clips of different lengths (the shorter ones are
    re-stretched at their own last frame inside vocode_windows; one gap ends at a clip's last frame, one clip has no gap): `wave`
    and `expected_inpaint` from the windowed passes are bit-identical to full ragged generator passes, and `hifi_masked` is the full
    pass over the masked mel."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch, mel_frames
    from speech_inpainting_amd.engine import InpaintingEngine
    from speech_inpainting_amd.predict import predict_clips_ragged
    harch, varch = HubertArch.tiny(), VocoderArch.v1()
    eng = InpaintingEngine(harch, varch, 100, "cuda:0", "fp32", voc).load_state(
        synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100))
    n16 = [64000, 41000, 52333, 30000]
    w16 = [synth.synth_wave(1, n, 40 + i)[0].numpy() for i, n in enumerate(n16)]
    w22 = [synth.synth_wave(1, -(-n * 441 // 320), 60 + i, sr=22050)[0].numpy() for i, n in enumerate(n16)]
    last = min(harch.num_frames(n16[1]), mel_frames(len(w22[1])))
    gaps = [[(20, 5), (90, 10), (104, 6), (150, 20)], [(10, 8), (last - 6, 6)], [], [(0, 4), (40, 12)]]
    nf = sum(l for g in gaps for _, l in g)
    tgt = torch.randint(0, 100, (nf,), generator=torch.Generator().manual_seed(5))
    out = predict_clips_ragged(eng, w16, w22, gaps=gaps, diagnostics=True, target_labels=tgt)
    mlen = out["mel_len"]
    full_inp = eng.vocode_ragged(out["mel"], mlen, stretch=True)
    full_masked = eng.vocode_ragged(out["mel_masked"], mlen, stretch=True)
    exp = out["mel_masked"].clone()
    eng.splice_labels_spans(tgt.cuda(), out["frame_clip"], out["frame_pos"], exp)
    full_exp = eng.vocode_ragged(exp, mlen, stretch=True)
    plain = predict_clips_ragged(eng, w16, w22, gaps=gaps)
    torch.cuda.synchronize()
    assert not torch.equal(full_inp, full_masked) and not torch.equal(full_exp, full_masked)
    assert torch.equal(out["hifi_masked"], full_masked)
    assert torch.equal(out["wave"], full_inp), float((out["wave"] - full_inp).abs().max())
    assert torch.equal(out["expected_inpaint"], full_exp), float((out["expected_inpaint"] - full_exp).abs().max())
    for k in ("feats", "labels", "mel", "wave"):
        assert torch.equal(out[k], plain[k]), k
    assert out["label_off"] == plain["label_off"] and out["wave_len"] == plain["wave_len"]
    assert torch.equal(out["wave"][2], full_masked[2])                               # the clip without a gap
