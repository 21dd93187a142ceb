"""The request front's reference (speech_inpainting_amd/stream.py): what one stream.Request returns when nothing is
pipelined -- the clips padded to the longest, engine.resample to both rates, each row cut to audio.resampled_len, the unpipelined
predict call of the request's mode, audio.to_int16_pcm.  A plain module: importing it needs no GPU."""
import numpy as np
import torch


def reference_result(eng, rq, sr_in):
    """-> dict(labels (host tensor), label_off (list or None), pcm (one int16 array per clip)) for the stream.Request `rq` whose clips
    are at `sr_in` Hz: mask_pos / mask_frames, blind, gaps= and patch=True, uniform or ragged."""
    from speech_inpainting_amd import audio
    from speech_inpainting_amd.predict import predict_clips, predict_clips_ragged
    lens = [len(c) for c in rq.clips]
    B = len(lens)
    ragged = min(lens) != max(lens)
    raw = torch.zeros(B, max(lens))
    for i, c in enumerate(rq.clips):
        raw[i, :lens[i]] = torch.from_numpy(np.asarray(c, dtype=np.float32))
    raw = raw.cuda()
    at = lambda sr: raw if sr == sr_in else eng.resample(raw, sr_in, sr, lens=lens if ragged else None)
    w16, w22 = at(16000), at(22050)
    n16 = [audio.resampled_len(n, sr_in, 16000) for n in lens]
    n22 = [audio.resampled_len(n, sr_in, 22050) for n in lens]
    assert w16.shape == (B, max(n16)) and w22.shape == (B, max(n22))
    if rq.patch:
        g = rq.gaps if rq.gaps is not None else [[(int(p), int(rq.mask_frames))] for p in rq.mask_pos]
        ref = eng.patch_multigap_batch(w16, w22, g, fade=int(rq.fade), len16=n16 if ragged else None, len22=n22 if ragged else None, pcm=True)
        torch.cuda.synchronize()
        pcm = [ref["patched_pcm"][i, :n22[i]].cpu().numpy() for i in range(B)]
        return dict(labels=ref["labels"].cpu(), label_off=ref["label_off"], pcm=pcm)
    a16 = [w16[i, :n16[i]].cpu().numpy() for i in range(B)]
    a22 = [w22[i, :n22[i]].cpu().numpy() for i in range(B)]
    kw = dict(gaps=rq.gaps) if rq.gaps is not None else dict(mask_pos=rq.mask_pos, mask_frames=rq.mask_frames, blind=rq.blind)
    if ragged:
        ref = predict_clips_ragged(eng, a16, a22, **kw)
        waves = [ref["wave"][i, :ref["wave_len"][i]] for i in range(B)]
    else:
        ref = predict_clips(eng, a16, a22, **kw)
        waves = [ref["wave"][i] for i in range(B)]
    torch.cuda.synchronize()
    return dict(labels=ref["labels"].cpu(), label_off=ref.get("label_off") if rq.gaps is not None else None,
                pcm=[audio.to_int16_pcm(w) for w in waves])


def assert_same(result, ref, what=""):
    """stream.Result against reference_result's dictionary: dtype, every length and every element of labels, label_off and PCM."""
    assert result.labels.dtype == ref["labels"].dtype == torch.int64, (what, result.labels.dtype, ref["labels"].dtype)
    assert result.labels.shape == ref["labels"].shape, (what, tuple(result.labels.shape), tuple(ref["labels"].shape))
    assert torch.equal(result.labels, ref["labels"]), (what, "labels")
    if ref["label_off"] is None:
        assert result.label_off is None, (what, result.label_off)
    else:
        assert result.label_off is not None and [int(v) for v in result.label_off] == [int(v) for v in ref["label_off"]], (what, "label_off")
    assert len(result.pcm) == len(ref["pcm"]), (what, len(result.pcm), len(ref["pcm"]))
    for i, (a, b) in enumerate(zip(result.pcm, ref["pcm"])):
        assert a.dtype == np.int16 and b.dtype == np.int16, (what, i, a.dtype, b.dtype)
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        assert np.array_equal(a, b), (what, i, int(np.count_nonzero(a != b)), "PCM samples differ")
