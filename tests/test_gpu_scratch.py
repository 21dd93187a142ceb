"""no result depends on scratch, on output memory, or on a ragged row's tail.

Every pass that has scratch runs under the three fills of tests/poison.py -- the caller-owned workspaces filled byte-wise with 0x00,
0xFF (NaN in every float format, -1 as an index) and 0x7B (finite and huge) in front of the call -- inside poisoned_allocs(), where
every torch.empty of native.py (outputs, freshly grown workspaces) comes back as NaN / INT_MAX: the outputs must be the same bits, and
finite.  Library-owned scratch has no pointer, so it is poisoned by history: a call that leaves it full, then the calls under test,
each against the same call on a fresh context.  Ragged entry points also get NaN and 1e30 behind each clip's own length, and inside one
call a clip that holds a NaN (or saturates the fp16 stream) must leave the other clips of its batch, and the next chunk, as they were.
The shapes are the smallest that reach each route; the last test holds the union of the families launched here against
poison.SCRATCH_FAMILIES."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import cases
from tests import poison as P
from tests.harness import build_engine, scoped_env, tapped_run
from tests.routes import (VOC_CONFIGS, VOC_RAGGED, VOC_TM, _base, _enc_engine, _encoder_entries, _i32, _large, _mel_engine, _mel_entries,
                          _ragged_mel, _tail, _tiny, _uniform_mel, _voc_engine, _voc_id)

pytestmark = pytest.mark.gpu

FAMILIES = set()                                       # poison.family_of(name) of every launch profiled in this file
T0 = time.time()
TAIL_FILLS = (float("nan"), 1e30)


def _note(prof):
    for n in prof:
        fam = P.family_of(n)
        assert fam is not None, f"launch {n!r} is in neither family list of tests/poison.py"
        FAMILIES.add(fam)
    return set(prof)


def _hold(ctx, run, outputs=None, finite=True, ws=True):
    """run() profiled once (the families it launches; the workspaces reach their size here, so that the baseline below really starts
    from zeros), then under the three fills -> (the baseline's outputs on the CPU, the launch names)."""
    with P.poisoned_allocs():
        _, _, prof = tapped_run(ctx, {}, run, profile=True)
        return P.same_bits(run, ctx if ws else None, outputs, finite=finite), _note(prof)


def _family_bytes(ctx, run, family):
    """The bytes the launchers of one family report to the profile over one run()."""
    ctx.profile_start(4000)
    try:
        run()
    finally:
        prof = ctx.profile_stop()
    return sum(e["bytes"] for e in prof if e["name"] == family)


# ------------------------------------------------------------------------------------------------------------ encoder
def test_the_poisoned_buffers_are_the_ones_the_passes_work_in():
    """The premise of every test below: the tensors poison_scratch fills are the workspaces the library is handed.  After a fill with
    0x7B each pass has overwritten part of its workspace, the workspace is still the same tensor (it was not regrown), and under
    poisoned_allocs() an output that a pass did not write would show: torch.empty hands out NaN."""
    from speech_inpainting_amd import synth
    eng = _mel_engine()
    ctx = eng.ctx
    wave = synth.synth_wave(2, 8000, 5).cuda()
    passes = {"_ws": [lambda: eng.encode(wave), lambda: eng.vocode(cases._mel(2, 20, 6).cuda())], "_ws_mel": [lambda: eng.mel(wave)]}
    with P.poisoned_allocs():
        assert bool(torch.isnan(torch.empty(64, dtype=torch.float32, device="cuda")).all())
        assert bool((torch.empty(64, dtype=torch.uint8, device="cuda") == 255).all())
        for attr, runs in passes.items():
            for run in runs:
                run()                                             # the workspace reaches its size
                ws = getattr(ctx, attr)
                P.poison_scratch(ctx, 0x7B)
                assert bool((ws == 0x7B).all())
                out = run()
                torch.cuda.synchronize()
                assert getattr(ctx, attr) is ws and ws.data_ptr() == getattr(ctx, attr).data_ptr()
                written = int((ws != 0x7B).sum())
                assert 0 < written < ws.numel(), (attr, written, ws.numel())
                assert bool(torch.isfinite(out).all())
        # and same_bits bites on the real workspace: a result that adds 0 * (a word of it the pass leaves alone) is caught by 0xFF, as a
        # kernel's zero weight times a stale word would be, and not by 0x7B (0 * 1.3e36 = 0)
        n4 = ctx._ws.numel() // 4 * 4
        P.poison_scratch(ctx, 0x7B)
        eng.vocode(cases._mel(2, 20, 6).cuda())
        idle = (ctx._ws[:n4] != 0x7B).reshape(-1, 4).any(1).logical_not().nonzero().reshape(-1)  # fp32 words the vocoder pass does not write
        word = int(idle[-1])
        leaky = lambda: eng.vocode(cases._mel(2, 20, 6).cuda()) + 0.0 * ctx._ws[:n4].view(torch.float32)[word]
        with pytest.raises(AssertionError, match="0xff"):
            P.same_bits(leaky, ctx, finite=True)
        P.same_bits(leaky, ctx, finite=True, fills=(0x00, 0x7B))


@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_tiny_encoder_every_entry_point(math):
    """The tiny architecture, B = 3, N = 8000 (24 frames): the six entry points, each under the three fills.  In fp32 every GEMM is a
    tap-GEMM and the attention is attention_f32; in bf16 the widths below 256 stay on the tap-GEMM and lingemm takes the rest."""
    harch = _tiny()
    eng = _enc_engine(harch, math)
    entries, _, lens, _ = _encoder_entries(eng, harch, 3, 8000, 11)
    for name, run in entries.items():
        out, prof = _hold(eng.ctx, run)
        assert any(n.startswith("tapgemm_") for n in prof), (name, sorted(prof))
        if math == "fp32":
            assert "attention_f32" in prof and not any(n.startswith(("lingemm", "gemmcu")) for n in prof), (name, sorted(prof))
        if name in ("varlen", "spans_ragged"):
            for b, n in enumerate(lens):
                assert not bool(out["out"][b, harch.num_frames(n):].any()), (name, b, "rows past the clip's own frames are not zero")


BASE_ENVS = [{}] + [{"SI_ENC_GEMMCU": str(f)} for f in (10, 11, 12, 13, 14, 15, 0)] + [{"SI_ENC_LNFUSE": "0"}, {"SI_ENC_OPREADY": "0"}, {"SI_ATT_BF16": "0"}]


@pytest.mark.parametrize("env", BASE_ENVS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_base_encoder_bf16_routes(env):
    """HuBERT-base's widths in bf16, B = 3, N = 24000 (74 frames): the default route, each forced gemmcu instantiation, lingemm alone, and
    the LayerNorm-fusion, operand-ready and bf16-attention switches turned off; the five entry points on the default route, the uniform
    and the ragged one on the others."""
    harch = _base()
    eng = _enc_engine(harch, "bf16", env)
    entries, _, _, _ = _encoder_entries(eng, harch, 3, 24000, 12, only=None if not env else ("forward", "varlen"))
    for name, run in entries.items():
        _, prof = _hold(eng.ctx, run)
        flag = int(env.get("SI_ENC_GEMMCU", "1"))
        if flag >= 10:
            assert any(n.startswith("gemmcu_bf16_") for n in prof), (name, sorted(prof))
        if flag == 0:
            assert any(n.startswith("lingemm_") for n in prof) and not any(n.startswith("gemmcu") for n in prof), (name, sorted(prof))
        if env.get("SI_ATT_BF16") == "0" or env.get("SI_ENC_OPREADY") == "0":
            assert "attention_f32" in prof and "attention_bf16" not in prof, (name, sorted(prof))
        else:
            assert "attention_bf16" in prof and "attention_f32" not in prof, (name, sorted(prof))
        if env.get("SI_ENC_LNFUSE") == "0":
            # the switch changes no launch and no value, only what the LayerNorms store: with it off they write their fp32 rows again
            default = _enc_engine(harch, "bf16", {})
            entry = _encoder_entries(default, harch, 3, 24000, 12, only=(name,))[0][name]
            assert _family_bytes(eng.ctx, run, "layernorm") > _family_bytes(default.ctx, entry, "layernorm"), name
        if not env:
            assert any(n.startswith("posconv_bf16_c48") for n in prof), (name, sorted(prof))


def test_large_encoder_posconv64_and_layernorm_after_conv():
    """HuBERT-large's widths (one layer), bf16, B = 2, N = 16000: posconv's 64-channel groups, the LayerNorm behind every conv."""
    harch = _large()
    eng = _enc_engine(harch, "bf16")
    entries, _, _, _ = _encoder_entries(eng, harch, 2, 16000, 13, only=("forward", "padded", "varlen", "extract"))
    for name, run in entries.items():
        _, prof = _hold(eng.ctx, run)
        assert any(n.startswith("posconv_bf16_c64") for n in prof) and "conv0_apply" in prof and "conv0_lagsums" not in prof, (name, sorted(prof))


def test_tiled_attention_and_packed_rows_that_end_the_buffer():
    """T = 300 > 256 frames, B = 2: the tiled attention kernel.  And the ragged frame list of test_gpu_encoder_ops.py (the whole-K/V
    kernel; packed rows whose last clip ends the buffer), its row tails holding NaN and 1e30 instead of samples."""
    from speech_inpainting_amd import synth
    harch = _base()
    eng = _enc_engine(harch, "bf16")
    N = 320 * 299 + 400
    assert harch.num_frames(N) == 300
    wave = synth.synth_wave(2, N, 14).cuda()
    _hold(eng.ctx, lambda: eng.encode(wave))
    _hold(eng.ctx, lambda: eng.encode(wave, valid_len=_i32([N, 320 * 256 + 400])))
    frames = [256, 33, 1, 129, 200, 32]
    lens = [320 * (f - 1) + 400 for f in frames]
    wave = synth.synth_wave(len(lens), max(lens), 90).cuda()
    zero = _hold(eng.ctx, lambda: eng.encode_ragged(_tail(wave, lens, 0.0), lens))[0]["out"]
    for b, f in enumerate(frames):
        assert not bool(zero[b, f:].any())
    for v in TAIL_FILLS:
        got = _hold(eng.ctx, lambda: eng.encode_ragged(_tail(wave, lens, v), lens))[0]["out"]
        assert torch.equal(got, zero), ("ragged attention case, row tails", v)


@pytest.mark.parametrize("arch,math", [("tiny", "fp32"), ("tiny", "bf16"), ("base", "bf16"), ("large", "bf16")])
def test_encoder_row_tails_are_ignored(arch, math):
    """"The rest [of a row] is ignored": NaN and 1e30 behind each clip's own samples against zeros, for the ragged entry points and for
    the padded one with normalize = 1 (with normalize = 0 the header defines the tail as input), at the tiny, base and large widths.
    The ragged outputs are zero past a clip's own frames; the padded entry's are defined on all T frames (the header: "as in the
    reference"), so there they are held to be finite and the same whatever the tail held."""
    harch = {"tiny": _tiny, "base": _base, "large": _large}[arch]()
    eng = _enc_engine(harch, math)
    B, N = {"tiny": (3, 8000), "base": (3, 24000), "large": (2, 16000)}[arch]
    entries, wave, lens, (ms, ml, tab) = _encoder_entries(eng, harch, B, N, 15)
    valid = _i32(lens)
    runs = {"varlen": lambda w: eng.encode_ragged(w, lens, ms, ml), "spans_ragged": lambda w: eng.encode_ragged(w, lens, spans=tab),
            "padded": lambda w: eng.encode(w, ms, ml, valid_len=valid)}
    for name, run in runs.items():
        zero = _hold(eng.ctx, lambda: run(_tail(wave, lens, 0.0)))[0]["out"]
        if name != "padded":
            for b, n in enumerate(lens):
                assert not bool(zero[b, harch.num_frames(n):].any()), (name, b, "rows past the clip's own frames are not zero")
        for v in TAIL_FILLS:
            w = _tail(wave, lens, v)
            got = _hold(eng.ctx, lambda: run(w))[0]["out"]
            assert torch.equal(got, zero), (name, v, int((got != zero).sum()))


@pytest.mark.parametrize("arch,math", [("tiny", "fp32"), ("tiny", "bf16"), ("base", "bf16"), ("large", "bf16")])
def test_a_nan_clip_stays_in_its_own_rows_of_the_encoder(arch, math):
    """Stale data inside ONE call: a NaN sample turns every intermediate of its clip NaN -- conv rows, packed transformer rows, the q | k | v
    rows next to its neighbours'.  The other clips of the batch (uniform, padded, ragged; the NaN clip first, in the middle, last) must
    come out bit for bit as without it: a halo row, a tile row or a masked key that is multiplied by zero instead of selected would show."""
    from speech_inpainting_amd import synth
    harch = {"tiny": _tiny, "base": _base, "large": _large}[arch]()
    eng = _enc_engine(harch, math)
    B, N = 3, 8000 if arch == "tiny" else 24000
    wave = synth.synth_wave(B, N, 16).cuda()
    lens = [N, 400 + 320 * 9, (N * 5 // 9) | 1]
    valid = _i32(lens)
    runs = {"uniform": lambda w: eng.encode(w), "padded": lambda w: eng.encode(w, valid_len=valid), "ragged": lambda w: eng.encode_ragged(w, lens)}
    with P.poisoned_allocs():
        for name, run in runs.items():
            clean = run(wave).cpu()
            assert bool(torch.isfinite(clean).all())
            for bad in range(B):
                w = wave.clone()
                w[bad, 200] = float("nan")
                got = run(w).cpu()
                rows = harch.num_frames(lens[bad]) if name == "ragged" else got.shape[1]
                assert not torch.equal(got[bad, :rows], clean[bad, :rows]), (name, bad, "the NaN did not reach the clip's own output")
                for b in range(B):
                    if b != bad:
                        assert torch.equal(got[b], clean[b]), (arch, math, name, f"clip {b} changed when clip {bad} held a NaN")


# ------------------------------------------------------------------------------------------------------------ generator
@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("cfg", VOC_CONFIGS, ids=_voc_id)
def test_generator_uniform_and_ragged(cfg, chunk):
    """si_hifigan_forward at Tm = 1, 57, 130 and si_hifigan_forward_varlen at mel_len = [57, 1, 30], B = 3, with and without the stretch,
    under the three fills; frames behind a clip's own hold NaN / 1e30 against zeros, and the samples behind its own are zero.
    vocoder_chunk = 2: the second chunk, one short clip, runs in the buffers the first chunk left -- the results equal chunk = 0's."""
    arch, math, env = cfg
    eng, varch = _voc_engine(arch, math, env, chunk)
    whole = _voc_engine(arch, math, env, 0)[0] if chunk else None
    seen = set()
    for stretch in (True, False):
        for Tm in VOC_TM:
            mel = _uniform_mel(varch, Tm)
            out, prof = _hold(eng.ctx, lambda: eng.vocode(mel, stretch))
            seen |= prof
            if whole is not None:
                assert torch.equal(out["out"], whole.vocode(mel, stretch).cpu()), (cfg, Tm, stretch, "chunk 2 != one chunk")
        mel = _ragged_mel(varch)
        zero, prof = _hold(eng.ctx, lambda: eng.vocode_ragged(_tail(mel, VOC_RAGGED, 0.0), VOC_RAGGED, stretch))
        seen |= prof
        for b, m in enumerate(VOC_RAGGED):
            assert not bool(zero["out"][b, eng.ctx.vocoder_samples(m, stretch):].any()), (cfg, b, "samples past the clip's own are not zero")
        for v in TAIL_FILLS:
            got = _hold(eng.ctx, lambda: eng.vocode_ragged(_tail(mel, VOC_RAGGED, v), VOC_RAGGED, stretch))[0]
            assert torch.equal(got["out"], zero["out"]), (cfg, stretch, "mel frames behind the clip's own", v)
        if whole is not None:
            assert torch.equal(zero["out"], whole.vocode_ragged(mel, VOC_RAGGED, stretch).cpu()), (cfg, stretch, "ragged: chunk 2 != one chunk")
    if (arch, math) == ("v1", "fp16") and not env:
        for fam in ("respair_f16_c256", "respair_f16_c128", "respair_f16_c64", "reschain_f16_c32", "upsample_f16_c", "gemmcu_f16_", "conv_post"):
            assert any(n.startswith(fam) for n in seen), (fam, sorted(seen))
    if env.get("SI_VOC_FUSE") == "0":
        assert not any(n.startswith(("respair", "reschain")) for n in seen), sorted(seen)
    if env.get("SI_VOC_CHAIN") == "0":
        assert not any(n.startswith("reschain") for n in seen), sorted(seen)


@pytest.mark.parametrize("math", ["fp16", "bf16"])
def test_second_chunk_is_clean_after_a_first_chunk_of_nan_and_saturation(math):
    """Stale data inside ONE call: vocoder_chunk = 2, clip 0 holds a NaN frame, clip 1 is scaled by 3e4 until the fp16 stream saturates
    (test_hot_input_saturates_exactly_where_it_must's scale), clip 2 is short and healthy and runs alone in the second chunk, in the
    buffers the first left.  Its samples equal the same clip run alone, bit for bit."""
    eng, varch = _voc_engine("v1", math, {}, 2)
    lens = [57, 57, 30]
    mel = cases._mel(3, 57, 410).cuda()
    mel[0, :, 20] = float("nan")
    mel[1] *= 3.0e4
    for stretch in (True, False):
        n = eng.ctx.vocoder_samples(lens[2], stretch)
        alone = eng.vocode(mel[2:3, :, :lens[2]].contiguous(), stretch).cpu()[0]
        got = _hold(eng.ctx, lambda: eng.vocode_ragged(mel, lens, stretch), finite=False)[0]["out"]
        print(f"   {math} stretch={stretch}: first chunk left {int(torch.isnan(got[0]).sum())} NaN samples in clip 0, clip 1 peaks at {float(got[1].abs().max()):.3g}")
        assert bool(torch.isfinite(got[2]).all()) and torch.equal(got[2, :n], alone) and not bool(got[2, n:].any()), (math, stretch)


@pytest.mark.parametrize("cfg", VOC_CONFIGS, ids=_voc_id)
def test_a_nan_or_saturated_clip_stays_in_its_own_rows_of_the_generator(cfg):
    """The same inside one chunk of the generator: one clip of three holds a NaN frame, or is scaled by 3e4 (the fp16 stream saturates and
    its stores launder NaN, so that is the fp16 form of the mistake); the two others, uniform and ragged, come out as without it."""
    arch, math, env = cfg
    eng, varch = _voc_engine(arch, math, env, 0)
    mel = cases._mel(3, 57, 420, varch.num_mels).cuda()
    runs = {"uniform": lambda m: eng.vocode(m), "ragged": lambda m: eng.vocode_ragged(m, VOC_RAGGED), "ragged, no stretch": lambda m: eng.vocode_ragged(m, VOC_RAGGED, False)}
    with P.poisoned_allocs():
        for name, run in runs.items():
            clean = run(mel).cpu()
            assert bool(torch.isfinite(clean).all())
            for bad in range(3):
                for what in ("nan", "hot"):
                    m = mel.clone()
                    if what == "nan":
                        m[bad, :, 0] = float("nan")
                    else:
                        m[bad] *= 3.0e4
                    got = run(m).cpu()
                    assert not torch.equal(got[bad], clean[bad])
                    for b in range(3):
                        if b != bad:
                            assert torch.equal(got[b], clean[b]), (cfg, name, what, f"clip {b} changed with clip {bad}")


def test_a_nan_clip_stays_in_its_own_rows_of_the_mel_frontend():
    from speech_inpainting_amd import synth
    eng = _mel_engine()
    N22 = 9999
    wave = synth.synth_wave(3, N22, 22, sr=22050).cuda()
    lens = [N22, 400, 5000]
    runs = {"uniform": lambda w: eng.mel(w), "ragged": lambda w: eng.mel_ragged(w, lens), "no normalisation": lambda w: eng.get_mel(w)}
    with P.poisoned_allocs():
        for name, run in runs.items():
            clean = run(wave).cpu()
            assert bool(torch.isfinite(clean).all())
            for bad in range(3):
                w = wave.clone()
                w[bad, 100] = float("nan")
                got = run(w).cpu()
                assert not torch.equal(got[bad], clean[bad])
                for b in range(3):
                    if b != bad:
                        assert torch.equal(got[b], clean[b]), (name, f"clip {b} changed when clip {bad} held a NaN")


# ------------------------------------------------------------------------------------------------------------ mel front-end
@pytest.mark.parametrize("N22", [22064, 22063])
def test_mel_frontend_every_entry_point(N22):
    """si_mel_frontend, _varlen and _spans, B = 3; the ragged batch holds one clip at the shortest length si_mel_frames accepts (400
    samples: one frame) and one that fills its row; NaN / 1e30 behind each clip's own samples against zeros; frames behind a clip's own are zero."""
    eng = _mel_engine()
    ctx = eng.ctx
    uniform, ragged, wave, lens = _mel_entries(eng, N22)
    for run in uniform:
        _hold(ctx, run)
    for name, run in ragged.items():
        zero = _hold(ctx, lambda: run(_tail(wave, lens, 0.0)))[0]["out"]
        for b, n in enumerate(lens):
            assert not bool(zero[b, :, ctx.mel_frames(n):].any()), (name, b, "frames past the clip's own are not zero")
        for v in TAIL_FILLS:
            w = _tail(wave, lens, v)
            got = _hold(ctx, lambda: run(w))[0]["out"]
            assert torch.equal(got, zero), (name, N22, v)


# ------------------------------------------------------------------------------------------------------------ F0 encoder
def _f0_with_workspace(ctx, desc, w, f0, byte):
    """si_f0_encoder_forward on a workspace of the test's own, filled with `byte` (native.f0_encoder takes a fresh torch.empty per call)."""
    from speech_inpainting_amd.native import _ptr
    d = desc.as_struct()
    B, _, T = f0.shape
    Tp = int(ctx.lib.si_f0_encoder_frames(C.byref(d), T))
    ws = torch.full((int(ctx.lib.si_f0_encoder_workspace_bytes(C.byref(d), B, T)),), byte, dtype=torch.uint8, device=ctx.device)
    out = torch.empty(B, Tp, desc.out_width, dtype=torch.float32, device=ctx.device)
    ctx._check(ctx.lib.si_f0_encoder_forward(ctx._h, C.byref(d), _ptr(w), _ptr(f0), B, T, _ptr(out), _ptr(ws), ws.numel(), ctx._stream()), "si_f0_encoder_forward")
    return out


@pytest.mark.parametrize("case", [("default", 876), ("default", 877), ("default", 878), ("default", 879), ("width=12", 200), ("width=12", 17)],
                         ids=lambda c: f"{c[0]}-T{c[1]}")
def test_f0_encoder_both_routes(case):
    """T = 876 ... 879 (the single launch up to 877, the 37 convolutions past it) and the width-12 descriptor (convolutions at any T).
    native.f0_encoder's workspace is a fresh torch.empty per call, which poisoned_allocs() fills with NaN: there is no 0x7B variant of
    THAT call, so the three fills go through the C ABI with a workspace of the test's own, and native's call must give the same bits."""
    from speech_inpainting_amd import native, synth
    from speech_inpainting_amd.engine import pack_f0_encoder
    name, T = case
    desc = native.F0EncDesc(**({"width": 12} if name == "width=12" else {}))
    ctx = _mel_engine().ctx
    w = pack_f0_encoder(synth.synth_f0_vqvae_state(desc, 20, seed=5), desc).cuda()
    f0 = (torch.randn(2, desc.in_width, T, generator=torch.Generator().manual_seed(T)).abs() * 2.0).cuda()
    with P.poisoned_allocs():
        _, via_native, prof = tapped_run(ctx, {}, lambda: ctx.f0_encoder(desc, w, f0), profile=True)
        _note(prof)
        assert set(prof) == ({"f0enc_fused"} if name == "default" and T <= 877 else {"f0enc_conv1d"}), prof
        fill = iter((0x00,) + P.FILLS)
        base = P.same_bits(lambda: _f0_with_workspace(ctx, desc, w, f0, next(fill)), None, finite=True)["out"]
    assert torch.equal(via_native.cpu(), base)
    with scoped_env({"SI_F0_FUSED": "0"}), P.poisoned_allocs():
        fill = iter((0x00,) + P.FILLS)
        layered = P.same_bits(lambda: _f0_with_workspace(ctx, desc, w, f0, next(fill)), None, finite=True)["out"]
    assert torch.equal(layered, base)


# ------------------------------------------------------------------------------------------------------------ library-owned scratch
def _fresh_ctx():
    """A context of its own: its library-owned scratch has no history (k-means and the detector need no weights)."""
    from speech_inpainting_amd.arch import VocoderArch
    from speech_inpainting_amd.native import NativeContext, make_desc
    return NativeContext(make_desc(_tiny(), VocoderArch.tiny(), 50), torch.device("cuda:0"))


def _on_fresh(call):
    ctx = _fresh_ctx()
    try:
        out = call(ctx)
        torch.cuda.synchronize()
        return [t.cpu() for t in out]
    finally:
        ctx.close()


def _same(a, b, what):
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(P.bits(x), P.bits(y)), what


def test_kmeans_norm_scratch_after_a_larger_codebook():
    """si_kmeans_assign on the MFMA route (D = 768): K = 500 whose centroids overflow |c|^2 (inf and NaN in ctx->km_cnorm), then K = 500
    and K = 50 healthy on the same context -- each equal to the same call on a fresh context."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(300, 768, generator=g).cuda()
    cents = {K: torch.randn(K, 768, generator=g).cuda() for K in (500, 50)}
    hot = cents[500].clone()
    hot[::3] *= 1e30
    hot[1] = float("nan")
    used = _fresh_ctx()
    try:
        with P.poisoned_allocs():
            _, _, prof = tapped_run(used, {}, lambda: used.kmeans_assign(x, hot, with_distance=True), profile=True)
            assert _note(prof) == {"kmeans_assign"}
            for K in (500, 50):
                got = [t.cpu() for t in used.kmeans_assign(x, cents[K], with_distance=True)]
                _same(got, _on_fresh(lambda c: c.kmeans_assign(x, cents[K], with_distance=True)), ("kmeans", K))
                assert int(got[0].min()) >= 0 and int(got[0].max()) < K and bool(torch.isfinite(got[1]).all())
    finally:
        used.close()


def _recording(n, dtype, ch, seed):
    """n sample times (of ch channels): noise with zeroed stretches and held samples placed across the 8-sample, 512-sample and chunk seams."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.9, 0.9, (n, max(ch, 1)))
    x[np.abs(x) < 0.05] = 0.3
    for s in sorted({0, 7, 511, 2047, 2048, 4095, n - 5} & set(range(n))):
        x[s:s + 6] = 0.0                                              # quiet runs on and across the seams
    for s in sorted({20, 2040, 4090, n - 12} & set(range(n))):
        x[s:s + 9] = x[s]                                             # held runs
    x = x if ch else x[:, 0]
    return torch.from_numpy(np.ascontiguousarray((x * 32767).astype(np.int16) if dtype == "int16" else x.astype(np.float32))).cuda()


def _detector_calls(x, ch, max_runs=64):
    """{name: call(ctx) -> [runs, n_runs (, T)]}: si_quiet_runs or si_quiet_runs_ch, and si_dead_runs with rel_threshold > 0 (the peak pass runs)."""
    thr = 3.0 if x.dtype == torch.int16 else 1e-4
    calls = {}
    chans = [None] if not ch else [0, ch - 1, -1]
    for c in chans:
        calls[f"quiet ch={c}"] = lambda ctx, c=c: list(ctx.quiet_runs(x, thr, 2, max_runs, channel=c))
        calls[f"dead ch={c}"] = lambda ctx, c=c: _dead(ctx, x, c, thr, max_runs)
    return calls


def _dead(ctx, x, c, thr, max_runs, rel=0.01, min_len=2):
    T = torch.empty(1, dtype=torch.float32, device=ctx.device)
    runs, n = ctx.dead_runs(x, threshold=thr, rel_threshold=rel, held_tol=0.0, min_len=min_len, max_runs=max_runs, channel=c, threshold_out=T)
    return [runs, n, T]


def _written(out):
    """The part of a detector result the ABI defines: the rows below min(n_runs, max_runs), the count [, T]."""
    n = min(int(out[1][0]), out[0].shape[0])
    return [out[0][:n]] + list(out[1:])


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("ch", [0, 3], ids=["mono", "3ch"])
def test_detector_scratch_after_a_long_quiet_recording(dtype, ch):
    """ctx->det_scratch by history.  First a long recording that is dead from end to end and whose peak is its last sample (rel_threshold
    = 1: T = peak) -- three carry tiles, a bitmap of all ones, lead / trail / carry / peak words set in every chunk.  Then the seam
    lengths of detect_ref.SEAM_N and dead_ref.SEAM_N through si_quiet_runs (_ch) and si_dead_runs on the SAME context: each result equals
    the same call on a fresh context, bit for bit, and a later, longer call finds what the long one left behind its shorter predecessors."""
    from tests import dead_ref as R
    from tests import detect_ref as D
    used = _fresh_ctx()
    try:
        n_long = 2 * 1024 * 2048 + 4101
        long = torch.full((n_long, ch) if ch else (n_long,), 0.25 if dtype == "float32" else 8000, dtype=getattr(torch, dtype)).cuda()
        long[-1] = 0.5 if dtype == "float32" else 16000
        with P.poisoned_allocs():
            chan = -1 if ch else None
            (_, (runs, cnt, T), prof) = tapped_run(used, {}, lambda: _dead(used, long, chan, 0.0, 4, rel=1.0, min_len=1), profile=True)
            _note(prof)
            assert {"detect_peak", "detect_peak_final", "detect_dead", "detect_carry", "detect_count", "detect_offsets", "detect_emit"} <= set(prof)
            assert int(cnt[0]) == 1 and runs[0].tolist() == [0, n_long] and float(T[0]) == float(long.reshape(-1)[-1])
            _, _, prof = tapped_run(used, {}, lambda: used.quiet_runs(long, 1e9, 1, 4, channel=chan), profile=True)
            assert ("detect_bits_ch" if ch else "detect_bits") in _note(prof)
            for n in sorted(set(D.SEAM_N) | set(R.SEAM_N)):
                x = _recording(n, dtype, ch, 1000 + n)
                for name, call in _detector_calls(x, ch).items():
                    got = [t.cpu() for t in call(used)]
                    want = _on_fresh(call)
                    _same(_written(got), _written(want), (dtype, ch, n, name))
                    assert 0 <= int(got[1][0]) <= n
    finally:
        used.close()


# ------------------------------------------------------------------------------------------------------------ ragged tails of the small ops
def test_small_ops_ignore_what_lies_behind_a_clips_own_length():
    """si_resample_sinc (n_len), si_wave_peak (sample_len), si_patch_compose (sample_len, and the rows of `gen` behind a window's samples),
    si_codebook_splice_varlen (frame_cnt: feature rows outside the spliced frames) and si_codebook_metrics (rows outside [pos, pos + Lm):
    it takes no frame_cnt): NaN and 1e30 there against zeros.  The outputs start as NaN / INT_MAX, so an unwritten word shows."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.native import SpanTable
    eng = _mel_engine()
    ctx = eng.ctx
    B, N = 3, 9000
    lens = [9000, 1, 4321]
    wave = synth.synth_wave(B, N, 31, sr=22050).cuda()
    len_dev = _i32(lens)
    tab = SpanTable([[(1000, 300)], [], [(4000, 321)]], eng.device)
    gen = synth.synth_wave(B, N, 32, sr=22050).cuda()
    wl = [8000, 1, 4200]                                   # generated samples per clip: clip 2's span [4000, 4321) is cut at lim = 4200
    feats = torch.randn(B, 24, 80, generator=torch.Generator().manual_seed(33)).cuda()
    pos, cnt, lm = _i32([3, 0, 10]), _i32([5, 0, 2]), 5
    melf = cases._mel(B, 30, 34).cuda()
    target = torch.randint(0, 50, (B, lm), generator=torch.Generator().manual_seed(35)).cuda()

    def rows_outside(f, counts, v):
        keep = torch.zeros(B, 24, dtype=torch.bool)
        for b in range(B):
            keep[b, int(pos[b]):int(pos[b]) + counts[b]] = True
        return torch.where(keep.cuda()[:, :, None], f, torch.full_like(f, v))

    def splice(v):
        m = melf.clone()
        labels = ctx.codebook_splice_varlen(rows_outside(feats, cnt.tolist(), v), pos, cnt, lm, m)
        return {"labels": labels, "mel": m}

    with P.poisoned_allocs():
        ref = {}
        for v in (0.0,) + TAIL_FILLS:
            w, g = _tail(wave, lens, v), _tail(gen, wl, v)
            got = {
                "resample": eng.resample(w, 22050, 16000, lens=lens),
                "peak": ctx.wave_peak(w, tab, len_dev),
                "peak_nospans": ctx.wave_peak(w, None, len_dev),
                "patched": eng.patch_from_wave(w, g, tab, 110, lens, wl)[0],
                "metrics": torch.cat([t.reshape(-1).float() for t in ctx.codebook_metrics(rows_outside(feats, [lm] * B, v), pos, lm, target)]),
            }
            got.update(splice(v))
            torch.cuda.synchronize()
            got = {k: t.cpu() for k, t in got.items()}
            for b, n in enumerate(lens):                              # si_patch_compose copies rows whole: the tail is the input's, bit for bit
                assert torch.equal(P.bits(got["patched"][b, n:]), P.bits(w[b, n:].cpu()))
                got["patched"][b, n:] = 0.0
            if not ref:
                ref = got
                for b, n in enumerate(lens):
                    assert not bool(got["resample"][b, int(n * 16000 / 22050):].any()), "si_resample_sinc: samples past int(len * ratio) are not zero"
                assert bool((got["labels"][1] == -1).all()) and got["labels"][0].tolist()[:5] == got["labels"][0].clamp(0, 49).tolist()[:5]
                assert got["labels"][2, 2:].tolist() == [-1, -1, -1] and int(got["labels"][2, :2].min()) >= 0
                for k, t in got.items():
                    assert not t.is_floating_point() or bool(torch.isfinite(t).all()), (k, "NaN or inf with zero tails")
                continue
            for k in ref:
                assert torch.equal(P.bits(got[k]), P.bits(ref[k])), (k, "depends on what lies behind a clip's own length", v)


# ------------------------------------------------------------------------------------------------------------ history, end to end
def _clips(secs, seed0):
    from speech_inpainting_amd import synth
    w16 = [synth.synth_wave(1, int(round(s * 16000)), seed0 + i)[0].numpy() for i, s in enumerate(secs)]
    w22 = [synth.synth_wave(1, -(-len(w) * 441 // 320), seed0 + 500 + i, sr=22050)[0].numpy() for i, w in enumerate(w16)]
    return w16, w22


E2E = {}


def _e2e_pair(arch, voc):
    """(used engine, fresh engine) of one architecture pair, the same state."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    harch, varch = (HubertArch.tiny(), VocoderArch.tiny()) if arch == "tiny" else (HubertArch.base(), VocoderArch.v1())
    if arch not in E2E:
        E2E[arch] = (synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(50))
    mk = lambda: build_engine(harch, varch, 50, "bf16", voc, state=E2E[arch])
    return mk(), mk(), harch


@pytest.mark.parametrize("arch,voc", [("tiny", "bf16"), ("tiny", "fp16"), ("base", "bf16"), ("base", "fp16")])
def test_a_healthy_request_after_one_that_left_nan_and_a_hot_clip(arch, voc):
    """Request 1, the larger shape: one clip holds a NaN sample (its features, and with them its rows of the workspace, turn NaN) and one
    clip's mel is scaled by 3e4 -- test_hot_input_saturates_exactly_where_it_must's scale: on the fp16 stream the stages' outputs saturate
    at +-65504, which is asserted on the fp16 taps of that very mel; the bf16 generator has nothing that saturates and is left with
    values of ~1e7 instead.  Request 2, smaller, healthy and ragged, on the same engine: feats, labels, mel and wave equal a fresh
    engine's, bit for bit, through predict_ragged.  Then through RequestFront with depth = 1 (the slot and its buffers are reused; a
    Result carries the PCM of the wave and the labels): the front takes waves only, and a scaled wave is normalised away by the mel
    front-end, so that leg carries the NaN history alone."""
    from speech_inpainting_amd.predict import pad_stack, predict_ragged
    from speech_inpainting_amd.stream import Request, RequestFront
    used, fresh, harch = _e2e_pair(arch, voc)
    try:
        lm = 5
        big16, big22 = _clips([2.0, 1.7, 1.2], 700)
        small16, small22 = _clips([1.1, 0.6], 800)
        pos_big, pos_small = [20, 30, 10], [12, 8]
        with P.poisoned_allocs():
            # request 1: predict_ragged's body with the mel in hand, so that one clip's can be scaled
            w16, len16 = pad_stack(big16)
            w22, len22 = pad_stack(big22)
            w16[0, 5000] = float("nan")
            mel = used.mel_ragged(w22.cuda(), len22)
            mel[1] *= 3.0e4
            mel_len = [used.ctx.mel_frames(n) for n in len22]
            out1 = used.predict_ragged_batch(w16.cuda(), len16, mel, mel_len, _i32(pos_big), lm)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out1["feats"][0]).any()), "request 1 left no NaN behind"
            if voc == "fp16":
                v = used.varch
                rows = len(big16) * (used.ctx.vocoder_samples(max(mel_len), True) // used.ctx.vocoder_samples(1, False))
                cap, c = {"pre.f16": rows * v.upsample_initial_channel}, v.upsample_initial_channel
                for i, u in enumerate(v.upsample_rates):
                    rows, c = rows * u, c // 2
                    cap[f"stage{i}.f16"] = rows * cases._padded(c)
                taps, _, _ = tapped_run(used.ctx, cap, lambda: used.vocode_ragged(out1["mel"], mel_len), profile=False)
                hot = {k: int((t.float().abs() == 65504.0).sum()) for k, t in taps.items()}
                print(f"   {arch} {voc}: request 1 left +-65504 in {hot}")
                assert len(taps) == len(cap) and sum(hot.values()) > 0, ("request 1 did not saturate the fp16 stream", hot)
            got = predict_ragged(used, small16, small22, pos_small, lm)
            want = predict_ragged(fresh, small16, small22, pos_small, lm)
            for i in range(len(small16)):
                for k in ("feats", "labels", "mel", "wave"):
                    assert torch.equal(got[i][k].cpu(), want[i][k].cpu()), (arch, voc, "predict_ragged", i, k)
                    assert k == "labels" or bool(torch.isfinite(got[i][k]).all())
            # the request front: one slot, so request 2 reuses request 1's pinned and device buffers
            bad = [c.copy() for c in big22]
            bad[0][7000] = np.nan
            rq = lambda clips, pos: Request(clips=clips, mask_pos=pos, mask_frames=lm)
            res = list(RequestFront(used, 22050, depth=1).run([rq(bad, pos_big), rq(small22, pos_small)]))
            ref = list(RequestFront(fresh, 22050, depth=1).run([rq(small22, pos_small)]))
            assert torch.equal(res[1].labels, ref[0].labels)
            for a, b in zip(res[1].pcm, ref[0].pcm):
                assert a.shape == b.shape and np.array_equal(a, b), (arch, voc, "RequestFront")
    finally:
        used.ctx.close()
        fresh.ctx.close()


# ------------------------------------------------------------------------------------------------------------ coverage
EXEMPT = ()                                            # (family, reason) pairs a test-sized run cannot reach: at most 3, and none is needed


def test_zz_every_scratch_family_was_launched_under_poison():
    """(last in the file) the union of the families launched above is a superset of poison.SCRATCH_FAMILIES."""
    assert len(EXEMPT) <= 3
    missing = set(P.SCRATCH_FAMILIES) - FAMILIES - {f for f, _ in EXEMPT}
    print(f"   families launched under poison: {len(FAMILIES & set(P.SCRATCH_FAMILIES))} of {len(P.SCRATCH_FAMILIES)} with scratch, "
          f"{len(FAMILIES & set(P.NO_SCRATCH_FAMILIES))} without; the file took {time.time() - T0:.1f} s")
    assert not missing, f"scratch families this file never launched: {sorted(missing)}"
