"""Recordings longer than one clip: si_cut_clips, si_patch_regions, engine.patch_recording and the `long:` key of
predict.yaml.  The route adds no arithmetic, so every comparison is bit for bit (torch.equal on int32 views).

Common shape: a recording of 300 frames + 123 samples (132423 samples at 22.05 kHz: 6 s and an odd tail, off the 16-byte grid), context
clips of 75 frames (n22 = 33075, n16 = 24000, T = 74, Tm = 75: 74 usable frames), 15 frames of context, the gaps below -- four
contexts: one clamped at frame 0, one clamped at frame 225, one with two gaps one frame apart (at fade 300 their ramps overlap) that
holds the first two frames of (140, 6) as a foreign gap cut by its end, and one that holds (106, 4) whole as a foreign gap at its local
frame 0 -- fades of 0, 110 and 300 samples, the fp32 and the fp16-stream vocoder."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests.cases import CHUNK, FADES, HOP, N_OUT, _weights64
from tests.cases import _patch_engine as _engine

pytestmark = pytest.mark.gpu

N_REC, TAIL, CLIP, CTX, LIM = 300, 123, 75, 15, 74
N22 = N_REC * 441 + TAIL                          # 132423
N16 = -(-N22 * 320 // 441)                        # the same recording at 16 kHz
L22, L16 = CLIP * 441, CLIP * 320                 # 33075, 24000
GAPS = [(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)]
KW = dict(clip_frames=CLIP, min_context=CTX)


def _i32(t):
    return t.contiguous().view(torch.int32)


def _recording(seed=41):
    from speech_inpainting_amd import synth
    return synth.synth_wave(1, N22, seed, sr=22050)[0].cuda(), synth.synth_wave(1, N16, seed + 1)[0].cuda()


def _plan(gaps=GAPS):
    from speech_inpainting_amd import gaps as G
    return G.plan_contexts(gaps, N_REC, CLIP, CTX, lim_frames=LIM)


def test_the_plan_of_the_common_shape_holds_every_case():
    plan = _plan()
    assert [c["start"] for c in plan] == [0, 68, 106, 225]
    assert plan[0]["start"] == 0 and (2 + 5) // 2 - CLIP // 2 < 0                              # clamped at frame 0
    assert plan[3]["start"] == N_REC - CLIP and (292 + 297) // 2 - CLIP // 2 > N_REC - CLIP    # clamped at frame 225
    (p0, l0), (p1, _) = plan[1]["own"]
    assert p1 - (p0 + l0) == 1 and 441 < 2 * 300                                               # one frame apart: the ramps overlap at fade 300
    assert plan[1]["foreign"] == [(140 - 68, 2)] and 68 + LIM == 142                           # (140, 6) cut by the context's end
    assert plan[2]["foreign"] == [(0, 4)] and plan[2]["start"] == 106                          # (106, 4) whole, at local frame 0


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("L", [L22, L22 + 1])
def test_cut_clips_against_torch_slicing(L):
    """Starts 0 (aligned), 441 (odd: the source row is off the 16-byte grid), 4 * 441 (aligned) and the last valid one; L = 33075
    leaves destination rows 1 .. 3 off the grid, 33076 keeps every row on it.  A planted -0.0 and a NaN payload cross unchanged."""
    from speech_inpainting_amd import native
    eng = _engine()
    ctx = eng.ctx
    src = torch.rand(N22, generator=torch.Generator().manual_seed(L)) - 0.5
    starts = [0, 441, 4 * 441, N22 - L]
    bits = src.view(torch.int32)
    for i, m in enumerate([3, 441 + 2, 441 + 2047, 441 + 2048, 4 * 441 + L - 1, N22 - 1, N22 - L + 5]):
        bits[m] = -2 ** 31 if i % 2 == 0 else 0x7fc12345
    src = src.cuda()
    out = ctx.cut_clips(src, starts, L)
    torch.cuda.synchronize()
    assert out.shape == (4, L)
    for c, s in enumerate(starts):
        assert torch.equal(_i32(out[c]), _i32(src[s:s + L])), c
    assert int((_i32(out) == 0x7fc12345).sum()) >= 3 and int((_i32(out) == -2 ** 31).sum()) >= 3
    # the 16 kHz side through the same call
    out16 = ctx.cut_clips(src[:N16].contiguous(), [320 * 68, 320 * 225], L16)
    assert torch.equal(_i32(out16[0]), _i32(src[320 * 68:320 * 68 + L16])) and torch.equal(_i32(out16[1]), _i32(src[320 * 225:320 * 225 + L16]))
    # bad start tables: refused before the launch, the output keeps its fill
    keep = torch.full((4, L), 7.0, device=eng.device)
    for bad, what in (([0, -1, 441, 882], "clip 1"), ([0, 441, 882, N22 - L + 1], "clip 3"), ([N22, 0, 0, 0], "clip 0")):
        ctx.profile_start(100)
        with pytest.raises(native.NativeError, match=f"si_cut_clips: {what} = samples .* is outside the source's {N22} samples"):
            ctx.cut_clips(src, bad, L, out=keep)
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        torch.cuda.synchronize()
        assert launched == [] and bool((keep == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ 2
def _region_case(eng, fade):
    """The plan of the common shape plus a fifth context, at frame 180, whose spans are set against the chunk seams OF THE RECORDING
    (multiples of 2048 from chunk 40 on: tests/test_gpu_patch.py::_seam_spans, shifted).  -> contexts, their own spans (local samples),
    the plan_patch of those spans, and the seam base."""
    from speech_inpainting_amd import gaps as G
    ctxs = _plan()
    own22 = G.spans22([c["own"] for c in ctxs], [L22] * 4)
    f, base = 180, 40 * CHUNK
    seams = [(base + CHUNK + fade // 2, 300), (base + 2 * CHUNK + fade + 700, CHUNK - fade - 650), (base + 4 * CHUNK + fade, 500),
             (base + 6 * CHUNK - fade - 400, 400)]
    ctxs = ctxs[:3] + [{"start": f}] + ctxs[3:]
    own22 = own22[:3] + [[(s - 441 * f, l) for s, l in seams]] + own22[3:]
    assert all(0 <= s and s + l + fade < N_OUT for s, l in own22[3]) and 441 * (140 + 6) + 2 * fade < seams[0][0]
    return ctxs, own22, eng.plan_patch(own22, [L22] * 5, fade), base


@pytest.mark.parametrize("fade", FADES)
def test_patch_regions_against_the_compose_kernel(fade):
    """Random orig / gen / gain.  Per context, si_patch_compose on the cut clip with that context's own spans is the reference: the
    long output equals it bit for bit at every sample whose weight (float64, from the definition) is non-zero, and equals the
    pre-filled output bit for bit everywhere else -- a sentinel that differs from orig (the samples are NOT written), a planted -0.0
    and a NaN payload.  out_pcm equals to_int16 of the fp32 result where written and keeps its fill elsewhere; an fp32-only and a
    pcm-only call agree with the call that produces both; a repeated call changes nothing."""
    from speech_inpainting_amd import native
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    ctxs, own22, plan, base = _region_case(eng, fade)
    B = len(ctxs)
    eng._patch_tables(plan)
    table = eng._region_table(ctxs, plan, own22)
    assert table.C == B and table.K == sum(len(s) for s in own22) and table.W == len(plan["wins"])
    g = torch.Generator().manual_seed(11 + fade)
    orig = ((torch.rand(N22, generator=g) * 2 - 1) * 0.7).to(dev)
    Lrow = max(w1 - w0 for _, w0, w1 in plan["wins"]) * HOP
    gen = torch.tanh(torch.randn(len(plan["wins"]), Lrow, generator=g)).to(dev)
    gain = (torch.rand(B, generator=g) * 0.5 + 0.1).to(dev)
    # the reference: the existing kernel on the cut clips
    starts = [441 * c["start"] for c in ctxs]
    cut = torch.stack([orig[s:s + L22] for s in starts])
    ref, ref_pcm = ctx.patch_compose(cut, native.SpanTable(own22, dev), plan["table"], gen, gain, f32=True, pcm=True)
    # weights on the recording's axis
    w = np.zeros(N22)
    owner = np.full(N22, -1)
    for b in range(B):
        wb, _ = _weights64(own22[b], plan["lim"][b], fade, L22)
        nz = np.flatnonzero(wb)
        assert np.all(w[starts[b] + nz] == 0)                         # regions of different contexts are disjoint
        w[starts[b] + nz], owner[starts[b] + nz] = wb[nz], b
    written = torch.from_numpy(w != 0).to(dev)
    assert int(written.sum()) == sum(l for s in own22 for _, l in s) + 2 * fade * table.K - (2 * fade - 441 if fade == 300 else 0)
    want = torch.zeros(N22, device=dev)
    want_pcm = torch.zeros(N22, dtype=torch.int16, device=dev)
    for b in range(B):
        sel = torch.from_numpy(owner[starts[b]:starts[b] + L22] == b).to(dev)
        want[starts[b]:starts[b] + L22][sel] = ref[b][sel]
        want_pcm[starts[b]:starts[b] + L22][sel] = ref_pcm[b][sel]
    # the pre-filled outputs: a sentinel that is not orig, -0.0 and a NaN payload where nothing is written
    fill = torch.full((N22,), 7.25, device=dev)
    fb = fill.view(torch.int32)
    plants = [0, 441 * 2 - fade - 1, base + CHUNK - fade // 2 - 1 if fade else base + CHUNK - 1, base + 4 * CHUNK - 1, base + 6 * CHUNK, N22 - 1, 441 * 75 + 7]
    for i, m in enumerate(plants):
        assert w[m] == 0
        fb[m] = -2 ** 31 if i % 2 == 0 else 0x7fc12345
    out, pcm = fill.clone(), torch.full((N22,), 77, dtype=torch.int16, device=dev)
    ctx.patch_regions(orig, table, gen, gain, out, pcm)
    o2, p2 = fill.clone(), pcm.clone().fill_(77)
    ctx.patch_regions(orig, table, gen, gain, o2, None)
    ctx.patch_regions(orig, table, gen, gain, None, p2)
    torch.cuda.synchronize()
    assert torch.equal(_i32(out)[written], _i32(want)[written])
    assert torch.equal(_i32(out)[~written], _i32(fill)[~written])
    assert torch.equal(pcm[written], want_pcm[written]) and torch.equal(pcm[written], eng.to_int16(out)[written])
    assert bool((pcm[~written] == 77).all())
    assert torch.equal(_i32(o2), _i32(out)) and torch.equal(p2, pcm)
    ctx.patch_regions(orig, table, gen, gain, out, pcm)              # orig is read, never out: the same result again
    torch.cuda.synchronize()
    assert torch.equal(_i32(o2), _i32(out)) and torch.equal(p2, pcm)
    # the chunk seams of the recording the fifth context's spans were set against
    if fade:
        assert 0 < w[base + CHUNK - 1] < 1 and 0 < w[base + CHUNK] < 1                      # inside a ramp
    assert w[base + 3 * CHUNK - 1] == 1 and w[base + 3 * CHUNK] == 1                         # inside a gap
    assert w[base + 4 * CHUNK - 1] == 0 and w[base + 4 * CHUNK] > 0                          # a region's first sample
    assert w[base + 6 * CHUNK - 1] > 0 and w[base + 6 * CHUNK] == 0                          # a region's last sample
    if fade == 300:                                                                          # the maximum rule, between (100, 5) and (106, 4)
        m = 441 * 105 + 150
        fall, rise = (_weights64([sp], plan["lim"][1], fade, L22)[0][m - starts[1]] for sp in own22[1])
        assert 0 < rise < fall < 1 and w[m] == fall


def test_malformed_region_tables_are_refused_before_any_launch():
    """Straight at the C ABI: each malformed si_region_table returns an error code and a message naming the entry, launches nothing and
    leaves both outputs untouched."""
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import native
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    fade = 110
    ctxs, own22, plan, base = _region_case(eng, fade)
    good = eng._region_table(ctxs, plan, own22)
    K, W, Q = good.K, good.W, good.Q
    h = good.host
    spans = [tuple(int(h[j * K + k]) for j in range(4)) for k in range(K)]
    wins = [tuple(int(h[4 * K + j * W + w]) for j in range(3)) for w in range(W)]
    chunks = [tuple(int(h[4 * K + 3 * W + j * Q + q]) for j in range(3)) for q in range(Q)]
    assert chunks == G.region_chunks([(max(s - fade, 0), min(s + l + fade, lim)) for s, l, _, lim in spans])
    Lrow = max(l for _, _, l in wins)
    orig = torch.rand(N22, device=dev)
    gen = torch.rand(W, Lrow, device=dev)
    out = torch.full((N22,), 7.0, device=dev)
    pcm = torch.full((N22,), 7, dtype=torch.int16, device=dev)
    keep = []

    def table(spans_=spans, wins_=wins, chunks_=chunks, fade_=fade, n_ctx=len(ctxs)):
        t = native.RegionTable(spans_, wins_, chunks_, n_ctx, max(fade_, 0), dev)
        keep.append(t)
        st = t.struct()
        st.fade = fade_
        return st

    def refused(st=None, o=out, q=pcm, lrow=Lrow, n=N22):
        st = good.struct() if st is None else st
        ctx.profile_start(100)
        rc = ctx.lib.si_patch_regions(ctx._h, native._ptr(orig), n, C.byref(st) if st else None, native._ptr(gen), lrow, None, native._ptr(o),
                                      native._ptr(q), ctx._stream())
        msg = ctx.lib.si_last_error(ctx._h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        torch.cuda.synchronize()
        assert rc != 0 and msg and launched == [], (rc, msg, launched)
        assert bool((out == 7.0).all()) and bool((pcm == 7).all())
        return msg

    def swap(rows, k, **kw):
        names = {"s": 0, "l": 1, "win": 2, "lim": 3} if len(rows[0]) == 4 else {"a": 0, "b": 1, "c": 2}
        r = list(rows[k])
        for key, v in kw.items():
            r[names[key]] = v
        return rows[:k] + [tuple(r)] + rows[k + 1:]

    assert "size mismatch" in refused(st=False)
    st = good.struct()
    st.struct_size -= 8
    assert "size mismatch" in refused(st)
    assert "fade" in refused(table(fade_=-1))
    assert "both outputs" in refused(o=None, q=None)
    assert "at most" in refused(n=2 ** 31 - 1 - 2047)
    assert "unsorted or overlapping" in refused(table(spans[:1] + [spans[2], spans[1]] + spans[3:]))          # unsorted
    assert "span 2 starts" in refused(table(swap(spans, 1, l=spans[2][0] - spans[1][0] + 1)))                  # overlapping
    assert "span 1" in refused(table(swap(spans, 1, l=0))) and "span 0" in refused(table(swap(spans, 0, s=-5)))
    assert "lim" in refused(table(swap(spans, K - 1, lim=N22 + 1))) and "lim" in refused(table(swap(spans, 1, lim=spans[1][0])))
    assert f"names window {W} of {W}" in refused(table(swap(spans, 0, win=W))) and "names window -1" in refused(table(swap(spans, 0, win=-1)))
    assert f"window 1 names context {len(ctxs)}" in refused(table(wins_=swap(wins, 1, a=len(ctxs))))
    assert "window 0 names context 0 of 0" in refused(table(n_ctx=0))
    assert "outside the recording" in refused(lrow=Lrow - HOP)                                              # win_len > Lrow
    assert "outside the recording" in refused(table(wins_=swap(wins, W - 1, b=N22 - 100)))
    assert "span 0 blends" in refused(table(wins_=swap(wins, 0, c=3 * 441)))                                # the row ends inside the gap
    assert "its window's row holds" in refused(table(wins_=swap(wins, 1, b=spans[1][0] - 50)))              # the row starts inside the rise
    assert "not strictly increasing" in refused(table(chunks_=chunks[:1] + [chunks[0]] + chunks[1:]))
    assert "not strictly increasing" in refused(table(chunks_=[chunks[1], chunks[0]] + chunks[2:]))
    assert "at or past" in refused(table(chunks_=chunks + [(-(-N22 // CHUNK), K, K)]))
    assert "walks spans" in refused(table(chunks_=swap(chunks, 0, c=K + 1))) and "walks spans" in refused(table(chunks_=swap(chunks, 0, b=-1)))
    seam = next(q for q, (_, k0, k1) in enumerate(chunks) if k1 - k0 == 1 and q and chunks[q - 1][2] == k1)    # a region's second chunk
    assert f"lacks chunk {chunks[seam][0]}" in refused(table(chunks_=chunks[:seam] + chunks[seam + 1:]))
    assert "lacks chunk" in refused(table(chunks_=chunks[:-1])) and "lacks chunk" in refused(table(chunks_=[]))
    assert f"omits span {chunks[seam][1]}" in refused(table(chunks_=swap(chunks, seam, c=chunks[seam][1])))   # an empty span range
    shared = next(q for q, (_, k0, k1) in enumerate(chunks) if k1 - k0 > 1) if any(k1 - k0 > 1 for _, k0, k1 in chunks) else None
    if shared is not None:
        assert "omits span" in refused(table(chunks_=swap(chunks, shared, b=chunks[shared][1] + 1)))
    # a chunk that no region touches is harmless, and the good table works
    assert all(c != 5 for c, _, _ in chunks)
    extra = sorted(chunks + [(5, 1, 1)])
    t = native.RegionTable(spans, wins, extra, len(ctxs), fade, dev)
    ctx.patch_regions(orig, t, gen, None, out, pcm)
    o2 = torch.full((N22,), 7.0, device=dev)
    ctx.patch_regions(orig, good, gen, None, o2, None)
    torch.cuda.synchronize()
    assert torch.equal(out, o2) and not bool((out == 7.0).all()) and float(out[0]) == 7.0


# ------------------------------------------------------------------------------------------------------------ 3
def _host_pasted_reference(eng, wave22, wave16, gaps, fade, clip=CLIP, ctx_frames=CTX):
    """The per-context route a caller would write: torch slicing, engine.resample (or slices of the 16 kHz recording),
    patch_multigap_batch on own + foreign local gaps, and only the OWN gaps' blend regions pasted into a clone of the recording."""
    from speech_inpainting_amd import gaps as G
    n22 = clip * 441
    lim = min(eng.ctx.num_frames(clip * 320), eng.ctx.mel_frames(n22))
    plan = G.plan_contexts(gaps, wave22.numel() // 441, clip, ctx_frames, lim_frames=lim)
    cut22 = torch.stack([wave22[441 * c["start"]:441 * c["start"] + n22] for c in plan])
    cut16 = eng.resample(cut22, 22050, 16000) if wave16 is None else torch.stack([wave16[320 * c["start"]:320 * c["start"] + clip * 320] for c in plan])
    out = eng.patch_multigap_batch(cut16, cut22, [c["own"] + c["foreign"] for c in plan], fade=fade)
    n_out = eng.ctx.vocoder_samples(eng.ctx.mel_frames(n22), True)
    ref, inside, labels = wave22.clone(), torch.zeros(wave22.numel(), dtype=torch.bool), []
    for b, c in enumerate(plan):
        s0 = 441 * c["start"]
        for a, e in G.blend_regions(G.spans22([c["own"]], [n22])[0], n22, n_out, fade):
            ref[s0 + a:s0 + e] = out["patched"][b, a:e]
            inside[s0 + a:s0 + e] = True
        o = out["label_off"][b]
        for p, l in out["gaps"][b]:
            if (p, l) in c["own"]:
                labels.append(out["labels"][o:o + l])
            o += l
    return ref, inside.to(wave22.device), torch.cat(labels), plan


@pytest.mark.parametrize("with16", [False, True])
@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_patch_recording_equals_the_host_pasted_reference_bit_for_bit(voc, with16):
    """The acceptance test: fades 0 / 110 / 300, the fp32 and the fp16-stream vocoder, contexts resampled from the cut clips and cut
    from a supplied 16 kHz recording.  Outside all own blend regions the output is the recording, bit for bit -- the 123-sample tail
    and the samples of a foreign gap inside a context among them."""
    eng = _engine(voc)
    wave22, wave16 = _recording()
    w16 = wave16 if with16 else None
    for fade in FADES:
        got = eng.patch_recording(wave22, GAPS, wave16=w16, fade=fade, pcm=True, **KW)
        ref, inside, labels, plan = _host_pasted_reference(eng, wave22, w16, GAPS, fade)
        torch.cuda.synchronize()
        assert got["contexts"] == plan and len(plan) == 4
        assert got["patched"].shape == (N22,) and torch.equal(_i32(got["patched"]), _i32(ref)), (fade, int((got["patched"] != ref).sum()))
        assert torch.equal(_i32(got["patched"])[~inside], _i32(wave22)[~inside])
        assert int(inside.sum()) == 441 * sum(l for _, l in GAPS) + 2 * fade * len(GAPS) - (2 * fade - 441 if fade == 300 else 0)
        assert not bool(inside[N_REC * 441:].any())
        for p, l in GAPS:                                               # every gap was filled, by something other than the recording
            assert not torch.equal(got["patched"][441 * p:441 * (p + l)], wave22[441 * p:441 * (p + l)])
        assert torch.equal(got["patched_pcm"], eng.to_int16(got["patched"]))
        assert torch.equal(got["labels"], labels) and got["label_off"] == [0, 3, 8, 12, 18, 23]
    # the gaps in any order, the recording as a host array
    again = eng.patch_recording(wave22.cpu().numpy(), list(reversed(GAPS)), wave16=None if w16 is None else w16.cpu(), fade=FADES[-1], **KW)
    assert torch.equal(_i32(again["patched"]), _i32(got["patched"])) and "patched_pcm" not in again


# ------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_batching_changes_nothing(voc):
    """Contexts one or two per pass equal all four in one pass, bit for bit: every context clip equals itself alone."""
    eng = _engine(voc)
    wave22, _ = _recording(seed=43)
    full = eng.patch_recording(wave22, GAPS, fade=110, batch=32, pcm=True, **KW)
    for batch in (1, 2):
        got = eng.patch_recording(wave22, GAPS, fade=110, batch=batch, pcm=True, **KW)
        torch.cuda.synchronize()
        assert torch.equal(_i32(got["patched"]), _i32(full["patched"])), (batch, int((got["patched"] != full["patched"]).sum()))
        assert torch.equal(got["patched_pcm"], full["patched_pcm"]) and torch.equal(got["labels"], full["labels"])
        assert got["label_off"] == full["label_off"] and got["contexts"] == full["contexts"]


# ------------------------------------------------------------------------------------------------------------ 5, 6
@pytest.mark.parametrize("n22", [L22, 60 * 441 + 57])
def test_a_recording_of_one_clip_or_less_equals_patch_multigap_batch(n22):
    """Exactly one clip (33075 samples at clip_frames = 75) and a recording shorter than a clip: one context, the whole recording with
    its true sample counts, equal to patch_multigap_batch at B = 1 -- also with gaps further apart than a context's budget."""
    from speech_inpainting_amd import synth
    eng = _engine()
    wave22 = synth.synth_wave(1, n22, 47, sr=22050).cuda()
    gaps = [(2, 3), (30, 4), (35, 4), (50, 8)]
    wave16 = eng.resample(wave22, 22050, 16000)
    ref = eng.patch_multigap_batch(wave16, wave22, [gaps], fade=110, pcm=True)
    for w16 in (None, wave16[0]):
        got = eng.patch_recording(wave22[0], gaps, wave16=w16, fade=110, pcm=True, **KW)
        torch.cuda.synchronize()
        assert len(got["contexts"]) == 1 and got["contexts"][0]["own"] == gaps and got["contexts"][0]["foreign"] == []
        assert torch.equal(_i32(got["patched"]), _i32(ref["patched"][0])) and torch.equal(got["patched_pcm"], ref["patched_pcm"][0])
        assert torch.equal(got["labels"], ref["labels"]) and got["label_off"] == [0, 3, 7, 11, 19]
    assert not torch.equal(got["patched"], wave22[0])


def test_no_gaps_is_an_exact_copy_and_launches_no_model_kernel():
    eng = _engine()
    wave22, _ = _recording(seed=45)
    wave22.view(torch.int32)[5] = -2 ** 31
    eng.ctx.profile_start(100)
    got = eng.patch_recording(wave22, [], **KW)
    launched = [e for e in eng.ctx.profile_stop() if e["launches"] > 0]
    torch.cuda.synchronize()
    assert launched == [], launched
    assert got["patched"].data_ptr() != wave22.data_ptr() and torch.equal(_i32(got["patched"]), _i32(wave22))
    assert got["contexts"] == [] and got["labels"].numel() == 0 and got["label_off"] == [0]
    with pytest.raises(ValueError, match=r"gap 0 = frames \[299, 300\) does not fit the usable frames"):
        eng.patch_recording(wave22, [(299, 1)], **KW)
    with pytest.raises(ValueError, match="cross-fades"):
        eng.patch_recording(wave22, [(100, 5), (140, 5), (147, 3)], fade=442, **KW)    # 442 samples: two frames of fade each side


# ------------------------------------------------------------------------------------------------------------ 7
def test_predict_entry_point_with_a_long_key(tmp_path, monkeypatch, capsys):
    """predict.py on a 6 s file with a `long:` mapping and three `masks:`: orig.wav, masked.wav and patched.wav hold the file's own
    sample count, patched.wav equals orig.wav outside the planned regions, and no whole-clip diagnostic is written."""
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
    n22 = 6 * 22050 + 123
    pcm_in = (synth.synth_wave(1, n22, 5, sr=22050)[0].numpy() * 32767).astype(np.int16)
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", 22050, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
masks:
  - {{start_pos_in_sec: 2.0, end_pos_in_sec: 2.125}}
  - {{start_pos_in_sec: 0.5, end_pos_in_sec: 0.625}}
  - {{start_pos_in_sec: 5.0, end_pos_in_sec: 5.25}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    assert sorted(p.name for p in out.iterdir()) == ["masked.wav", "orig.wav", "patched.wav"]
    files = {}
    for f in ("orig.wav", "masked.wav", "patched.wav"):
        sr, files[f] = wavfile.read(out / f)
        assert sr == 22050 and files[f].dtype == np.int16 and len(files[f]) == n22, f
    assert np.array_equal(files["orig.wav"], pcm_in)
    gaps = [(25, 6), (100, 6), (250, 12)]                                 # 0.5 s, 2 s, 5 s on the 20 ms grid; 125 ms = 6 frames
    keep = np.ones(n22, dtype=bool)
    for p, l in gaps:
        keep[441 * p - 110:441 * (p + l) + 110] = False                   # the default fade: 5 ms
        assert not np.array_equal(files["patched.wav"][441 * p:441 * (p + l)], pcm_in[441 * p:441 * (p + l)])
    assert np.array_equal(files["patched.wav"][keep], pcm_in[keep])
    zeroed = pcm_in.copy()
    for p, l in gaps:
        zeroed[441 * p:441 * (p + l)] = 0
    assert np.array_equal(files["masked.wav"], zeroed)
    printed = capsys.readouterr().out
    assert all(f"gap {k} = frames [{p}, {p + l})" in printed for k, (p, l) in enumerate(gaps))
