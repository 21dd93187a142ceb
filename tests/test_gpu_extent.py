"""a pass writes its outputs and the requested bytes of its regions, nothing else.

The engines are built with SI_WS_REDZONE=65536: the carve leaves 64 KiB in front of the first region and behind every region of the
caller-owned workspace, and si_debug_ws_regions names what the pass asked for.  In front of every call the whole workspace is filled
with one of the two fills of tests/extent.py; the call runs inside guarded_allocs(), where every torch.empty of native.py lies between
two 64 KiB bands of the same fill.  Afterwards every byte of the workspace outside the requested bytes of the regions, every band
and every input hold the bits they held.  The routes are those of tests/routes.py: the smallest shapes that reach
each kernel, whose last tile is partial almost everywhere.  All assertions are exact."""
import ctypes as C
import time

import pytest
import torch

from tests import cases
from tests import extent as X
from tests import poison as P
from tests.harness import build_engine, scoped_env, tapped_run
from tests.routes import (MEL_N22, VOC_CONFIGS, VOC_RAGGED, VOC_TM, _base, _enc_engine, _encoder_entries, _i32, _large, _mel_engine, _mel_entries,
                          _ragged_mel, _tiny, _uniform_mel, _voc_engine, _voc_id)

pytestmark = pytest.mark.gpu

R = 65536
ZONE = {"SI_WS_REDZONE": str(R)}
FAMILIES = set()                                       # poison.family_of(name) of every launch profiled in this file
T0 = time.time()
LIBRARY_OWNED = {"kmeans_assign"} | {f for f in P.SCRATCH_FAMILIES if f.startswith("detect_")}   # ctx->km_cnorm, ctx->det_scratch: no pointer to read


def _up(v, a=256):
    return (v + a - 1) // a * a


def _note(prof):
    for n in prof:
        fam = P.family_of(n)
        assert fam is not None, f"launch {n!r} is in neither family list of tests/poison.py"
        FAMILIES.add(fam)
    return set(prof)


def _laid_out(regions, zone):
    """The regions lie as the header states: the first behind one zone, each next one 256-aligned behind its predecessor's bytes and zone."""
    assert regions and regions[0][1] == zone, regions[:1]
    for (_, o, n), (name, o2, _) in zip(regions, regions[1:]):
        assert o2 == _up(o + n) + zone, (name, o2, o, n)
    assert len({r[0] for r in regions}) == len(regions) <= 32


def _guard(eng, which, run, inputs=(), attr="_ws", zone=R):
    """run() profiled once (its families; the workspace reaches its size), then once per fill on the filled workspace inside
    guarded_allocs(): the workspace outside the regions, the bands and the inputs are untouched -> (the last result, the launch names).
    The profiled run is banded as well (a workspace it grows too), so that no run of a pass in this file has an output or a workspace
    that ends where the test's memory ends."""
    ctx = eng.ctx
    with X.guarded_allocs(X.FILLS[0]) as first:
        _, _, prof = tapped_run(ctx, {}, run, profile=True)
    first.check()
    watched = dict(inputs) if isinstance(inputs, dict) else {i: t for i, t in enumerate(inputs)}
    watched["weights"] = eng.weights_tensor()
    for fill in X.FILLS:
        ws = getattr(ctx, attr)
        ws.fill_(fill)
        snap = X.unchanged(watched)
        with X.guarded_allocs(fill) as rec:
            out = run()
            torch.cuda.synchronize()
        assert getattr(ctx, attr) is ws and rec.allocs, "the workspace was regrown, or the call allocated no output"
        regions = ctx.ws_regions(which)
        _laid_out(regions, zone)
        X.check_workspace(ws, regions, fill)
        rec.check()
        snap.check()
    return out, _note(prof)


# ------------------------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_tiny_encoder_every_entry_point(math):
    """The tiny architecture: B = 3, N = 8000 (24 frames, 72 rows) through the six entry points, and B = 1, N = 400 (one frame)."""
    from speech_inpainting_amd import synth
    harch = _tiny()
    eng = _enc_engine(harch, math, ZONE)
    entries, wave, _, (ms, ml, _) = _encoder_entries(eng, harch, 3, 8000, 11)
    for name, run in entries.items():
        _, prof = _guard(eng, "encoder", run, {"wave": wave, "mask_start": ms, "mask_len": ml})
        assert any(n.startswith("tapgemm_") for n in prof), (name, sorted(prof))
    one = synth.synth_wave(1, 400, 12).cuda()
    out, _ = _guard(eng, "encoder", lambda: eng.encode(one), {"wave": one})
    assert out.shape[:2] == (1, 1)
    names = [r[0] for r in eng.ctx.ws_regions("encoder")]
    assert names[:2] == ["stats", "partials"] and ("lnf16" in names) == (math == "bf16"), names


BASE_ENVS = [{}] + [{"SI_ENC_GEMMCU": str(f)} for f in (10, 11, 12, 13, 14, 15, 0)] + [{"SI_ENC_LNFUSE": "0"}, {"SI_ENC_OPREADY": "0"}, {"SI_ATT_BF16": "0"},
                                                                                     {"SI_ENC_FFNPAD": "0"}, {"SI_ENC_FFNPAD": "128"}]


@pytest.mark.parametrize("env", BASE_ENVS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_base_encoder_bf16_routes(env):
    """HuBERT-base's widths in bf16, one layer, B = 3, N = 24000: 74 frames, 222 rows uniform and 116 packed -- the last row tile of
    every GEMM is partial.  Every entry point on the default route; the uniform and the ragged one under each switch."""
    harch = _base()
    eng = _enc_engine(harch, "bf16", dict(env, **ZONE))
    entries, wave, _, (ms, ml, _) = _encoder_entries(eng, harch, 3, 24000, 12, only=None if not env else ("forward", "varlen"))
    for name, run in entries.items():
        _, prof = _guard(eng, "encoder", run, {"wave": wave, "mask_start": ms, "mask_len": ml})
        flag = int(env.get("SI_ENC_GEMMCU", "1"))
        if flag >= 10:
            assert any(n.startswith("gemmcu_bf16_") for n in prof), (name, sorted(prof))
        if flag == 0:
            assert any(n.startswith("lingemm_") for n in prof) and not any(n.startswith("gemmcu") for n in prof), (name, sorted(prof))
        regions = {r[0]: r[2] for r in eng.ctx.ws_regions("encoder")}
        rows = regions["h"] // (4 * harch.hidden_size)
        assert rows == (222 if name != "varlen" and name != "spans_ragged" else 116), (name, rows)
        assert ("ln_stats" in regions) == (env.get("SI_ENC_LNFUSE") != "0" and env.get("SI_ENC_OPREADY") != "0"), (name, sorted(regions))
        if env.get("SI_ENC_OPREADY") != "0":
            pad = int(env.get("SI_ENC_FFNPAD", "64"))
            assert regions["ffn16"] == rows * (harch.intermediate_size + pad) * 2, (name, regions["ffn16"])


def test_large_encoder_widths():
    """HuBERT-large's widths (one layer), bf16, B = 2, N = 16000: the LayerNorm behind every conv, posconv's 64-channel groups."""
    harch = _large()
    eng = _enc_engine(harch, "bf16", ZONE)
    entries, wave, _, (ms, ml, _) = _encoder_entries(eng, harch, 2, 16000, 13, only=("forward", "padded", "varlen", "extract"))
    for name, run in entries.items():
        _, prof = _guard(eng, "encoder", run, {"wave": wave, "mask_start": ms, "mask_len": ml})
        assert any(n.startswith("posconv_bf16_c64") for n in prof) and "conv0_apply" in prof, (name, sorted(prof))


def test_tiled_attention_and_packed_rows_that_end_the_buffer():
    """T = 300 > 256 frames, B = 2, uniform and padded: the tiled attention kernel.  And the ragged frame list of
    test_gpu_encoder_ops.py: packed rows whose last clip ends q | k | v and the attention output."""
    from speech_inpainting_amd import synth
    harch = _base()
    eng = _enc_engine(harch, "bf16", ZONE)
    N = 320 * 299 + 400
    assert harch.num_frames(N) == 300
    wave = synth.synth_wave(2, N, 14).cuda()
    _guard(eng, "encoder", lambda: eng.encode(wave), {"wave": wave})
    valid = _i32([N, 320 * 256 + 400])
    _guard(eng, "encoder", lambda: eng.encode(wave, valid_len=valid), {"wave": wave, "valid_len": valid})
    frames = [256, 33, 1, 129, 200, 32]
    lens = [320 * (f - 1) + 400 for f in frames]
    ragged = synth.synth_wave(len(lens), max(lens), 90).cuda()
    _, prof = _guard(eng, "encoder", lambda: eng.encode_ragged(ragged, lens), {"wave": ragged})
    assert "attention_bf16" in prof and {"pack_rows", "unpack_rows"} <= prof, sorted(prof)
    assert dict((r[0], r[2]) for r in eng.ctx.ws_regions("encoder"))["att"] == sum(frames) * harch.hidden_size * 4


# ------------------------------------------------------------------------------------------------------------ generator
EXTENT_VOC = VOC_CONFIGS + [("v1", "fp16", {"SI_VOC_UPSGEMM": "0"})]


@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("cfg", EXTENT_VOC, ids=_voc_id)
def test_generator_uniform_and_ragged(cfg, chunk):
    """si_hifigan_forward at Tm = 1, 57, 130 and si_hifigan_forward_varlen at mel_len = [57, 1, 30], B = 3, with and without the stretch.
    vocoder_chunk = 2: the buffers hold two clips and the second chunk, one clip, runs in them."""
    arch, math, env = cfg
    eng, varch = _voc_engine(arch, math, dict(env, **ZONE), chunk)
    seen = set()
    for stretch in (True, False):
        for Tm in VOC_TM:
            mel = _uniform_mel(varch, Tm)
            seen |= _guard(eng, "vocoder", lambda: eng.vocode(mel, stretch), {"mel": mel})[1]
        mel = _ragged_mel(varch)
        seen |= _guard(eng, "vocoder", lambda: eng.vocode_ragged(mel, VOC_RAGGED, stretch), {"mel": mel})[1]
        names = [r[0] for r in eng.ctx.ws_regions("vocoder")]
        assert names == ["lengths", "ext"] + [f"buf{i}" for i in range(6)] + [f"h16_{i}" for i in range(6)], names
    if (arch, math) == ("v1", "fp16") and not env:
        for fam in ("respair_f16_c256", "respair_f16_c128", "respair_f16_c64", "reschain_f16_c32", "upsample_f16_c", "gemmcu_f16_", "conv_post"):
            assert any(n.startswith(fam) for n in seen), (fam, sorted(seen))
    if env.get("SI_VOC_UPSGEMM") == "0":
        assert not any(n.startswith("gemmcu") for n in seen), sorted(seen)


# ------------------------------------------------------------------------------------------------------------ mel front-end
@pytest.mark.parametrize("N22", MEL_N22)
def test_mel_frontend_every_entry_point(N22):
    """si_mel_frontend, _varlen and _spans, B = 3; the ragged batch [N22, 400, 9999] holds a one-frame clip and one that fills its row."""
    eng = _mel_engine(ZONE)
    uniform, ragged, wave, _ = _mel_entries(eng, N22)
    for run in uniform:
        _guard(eng, "mel", run, {"wave": wave}, attr="_ws_mel")
        assert [r[0] for r in eng.ctx.ws_regions("mel")] == ["peak", "frames", "spec"]
    for name, run in ragged.items():
        _guard(eng, "mel", lambda: run(wave), {"wave": wave}, attr="_ws_mel")
        assert [r[0] for r in eng.ctx.ws_regions("mel")] == ["peak", "frames", "spec", "lengths"], name


# ------------------------------------------------------------------------------------------------------------ F0 encoder
@pytest.mark.parametrize("case", [("default", 877, "1"), ("default", 878, "1"), ("default", 877, "0"), ("width=12", 17, "1")],
                         ids=lambda c: f"{c[0]}-T{c[1]}-fused{c[2]}")
def test_f0_encoder_both_routes(case):
    """si_f0_encoder_forward through the C ABI on a workspace of the test's own between two bands.  T = 877 is the last length of the
    single launch, which keeps the track in LDS: the workspace is untouched everywhere.  T = 878, SI_F0_FUSED=0 and width = 12 run
    layer by layer in three slots of B * c * T1 floats + 256 bytes: the 256 bytes behind each slot's floats and the bands are untouched."""
    from speech_inpainting_amd import native, synth
    from speech_inpainting_amd.engine import pack_f0_encoder
    from speech_inpainting_amd.native import _ptr
    name, T, fused = case
    desc = native.F0EncDesc(**({"width": 12} if name == "width=12" else {}))
    ctx = _mel_engine(ZONE).ctx
    w = pack_f0_encoder(synth.synth_f0_vqvae_state(desc, 20, seed=5), desc).cuda()
    B = 2
    f0 = (torch.randn(B, desc.in_width, T, generator=torch.Generator().manual_seed(T)).abs() * 2.0).cuda()
    d = desc.as_struct()
    k, pad = desc.down_kernel()
    floats = B * max(desc.width, desc.n_state) * ((T + 2 * pad - k) // desc.stride_t + 1)
    need = int(ctx.lib.si_f0_encoder_workspace_bytes(C.byref(d), B, T))
    assert need == 3 * (floats * 4 + 256)
    single = name == "default" and T <= 877 and fused == "1"
    slots = [] if single else [(f"slot{i}", R + i * (floats * 4 + 256), floats * 4) for i in range(3)]
    Tp = int(ctx.lib.si_f0_encoder_frames(C.byref(d), T))
    outs = []
    with scoped_env({"SI_F0_FUSED": fused}):
        with X.guarded_allocs(X.FILLS[0]) as first:                  # native's call: its per-call workspace and its output between bands
            _, _, prof = tapped_run(ctx, {}, lambda: ctx.f0_encoder(desc, w, f0), profile=True)
        first.check()
        assert _note(prof) == ({"f0enc_fused"} if single else {"f0enc_conv1d"}), prof
        for fill in X.FILLS:
            raw = torch.full((R + need + R,), fill, dtype=torch.uint8, device=ctx.device)
            snap = X.unchanged({"f0": f0, "weights": w})
            with X.guarded_allocs(fill) as rec:
                out = torch.empty(B, Tp, desc.out_width, dtype=torch.float32, device=ctx.device)
                ctx._check(ctx.lib.si_f0_encoder_forward(ctx._h, C.byref(d), _ptr(w), _ptr(f0), B, T, _ptr(out), C.c_void_p(raw.data_ptr() + R), need,
                                                         ctx._stream()), "si_f0_encoder_forward")
                torch.cuda.synchronize()
            X.check_workspace(raw, slots, fill)
            rec.check()
            snap.check()
            outs.append(out.cpu())
    assert torch.equal(P.bits(outs[0]), P.bits(outs[1])) and bool(torch.isfinite(outs[0]).all())


# ------------------------------------------------------------------------------------------------------------ outputs only
def _banded(run, inputs):
    """run() inside guarded_allocs() under both fills: the bands and the inputs keep their bits."""
    for fill in X.FILLS:
        snap = X.unchanged(inputs)
        with X.guarded_allocs(fill) as rec:
            run()
            torch.cuda.synchronize()
        assert rec.allocs
        rec.check()
        snap.check()


def test_label_and_metric_kernels_write_their_outputs_only():
    """si_codebook_splice in both forms, si_kmeans_assign (MFMA and plain), si_codebook_metrics, si_mel_metrics and si_sisdr, each at
    the smallest shape of tests/label_ref.py, their outputs between bands.  The splice also writes the mel, a tensor of the test's:
    it lies between bands too."""
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from tests import label_ref as L
    K, D = L.SPLICE_KS[0], 80
    case = L.codebook_case(K, D)
    F = len(case["v"])
    eng = build_engine(HubertArch.tiny(codebook_dim=D), VocoderArch.tiny(), K, state=(None, None, torch.from_numpy(case["cb"])), key=f"test_gpu_extent:{K}x{D}")
    ctx = eng.ctx
    feats = torch.from_numpy(case["v"]).reshape(1, F, D).cuda()
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    clip, frame = torch.zeros(F, dtype=torch.int32, device="cuda"), torch.arange(F, dtype=torch.int32, device="cuda")
    target = torch.from_numpy(case["target"]).reshape(1, F).cuda()
    for form in ("clip", "spans"):
        for fill in X.FILLS:
            snap = X.unchanged({"feats": feats, "pos": pos, "clip": clip, "frame": frame})
            with X.guarded_allocs(fill) as rec:
                mel = torch.empty(1, D, F + 2, dtype=torch.float32, device="cuda")
                mel.fill_(1000.0)
                lab = ctx.codebook_splice(feats, pos, F, mel) if form == "clip" else ctx.codebook_splice_spans(feats, clip, frame, mel)
                torch.cuda.synchronize()
            assert len(rec.allocs) == 2 and bool((mel[:, :, F:] == 1000.0).all()) and int(lab.min()) >= 0 and int(lab.max()) < K
            rec.check()
            snap.check()
    _banded(lambda: ctx.codebook_metrics(feats, pos, F, target), {"feats": feats, "pos": pos, "target": target})
    shape = min(L.KMEANS_SHAPES)
    km = L.kmeans_case(*shape)
    x, cent = torch.from_numpy(km["x"]).cuda(), torch.from_numpy(km["cent"]).cuda()
    for env in ({}, {"SI_KMEANS_MFMA": "0"}):
        with scoped_env(env):
            _banded(lambda: ctx.kmeans_assign(x, cent, with_distance=True), {"x": x, "cent": cent})
    Dm, Ln = min(L.MEL_SHAPES, key=lambda s: s[0] * s[1])
    a, b = cases._mel(3, Ln, 7, Dm).cuda(), cases._mel(3, Ln, 8, Dm).cuda()
    _banded(lambda: ctx.mel_metrics(a, b), {"a": a, "b": b})
    n = min(L.SISDR_NS)
    est, ref = torch.randn(3, n, generator=torch.Generator().manual_seed(1)).cuda(), torch.randn(3, n, generator=torch.Generator().manual_seed(2)).cuda()
    _banded(lambda: ctx.sisdr(est, ref), {"est": est, "ref": ref})


# ------------------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("voc", ["bf16", "fp16"])
def test_one_ragged_step_writes_inside_its_allocations(voc):
    """predict_ragged_batch on the tiny pair (bf16 encoder): every allocation of the step is banded, both workspaces are checked against
    the regions of the pass that ran last in them, and the weight blob and the inputs have the same bits afterwards."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.predict import pad_stack
    eng = build_engine(HubertArch.tiny(), VocoderArch.tiny(), 50, "bf16", voc, env=ZONE, key=("test_gpu_extent", "step", voc))
    w16 = [synth.synth_wave(1, int(round(s * 16000)), 800 + i)[0].numpy() for i, s in enumerate([1.1, 0.6])]
    w22 = [synth.synth_wave(1, -(-len(w) * 441 // 320), 1300 + i, sr=22050)[0].numpy() for i, w in enumerate(w16)]
    (wave16, len16), (wave22, len22) = pad_stack(w16), pad_stack(w22)
    wave16, wave22, pos = wave16.cuda(), wave22.cuda(), _i32([12, 8])
    mel_len = [eng.ctx.mel_frames(n) for n in len22]

    def step():
        mel = eng.mel_ragged(wave22, len22)
        return eng.predict_ragged_batch(wave16, len16, mel, mel_len, pos, 5)

    want = step()
    torch.cuda.synchronize()
    for fill in X.FILLS:
        eng.ctx._ws.fill_(fill)
        eng.ctx._ws_mel.fill_(fill)
        ws, ws_mel = eng.ctx._ws, eng.ctx._ws_mel
        snap = X.unchanged({"wave16": wave16, "wave22": wave22, "pos": pos, "weights": eng.weights_tensor()})
        with X.guarded_allocs(fill) as rec:
            got = step()
            torch.cuda.synchronize()
        assert eng.ctx._ws is ws and eng.ctx._ws_mel is ws_mel and len(rec.allocs) >= 4
        rec.check()
        snap.check()
        X.check_workspace(ws_mel, eng.ctx.ws_regions("mel"), fill)
        # the encoder and the generator share one workspace: what lies outside BOTH carves is untouched
        X.check_workspace(ws, eng.ctx.ws_regions("encoder") + eng.ctx.ws_regions("vocoder"), fill)
        for k in ("feats", "labels", "mel", "wave"):
            assert torch.equal(P.bits(got[k]), P.bits(want[k])), (voc, k)


# ------------------------------------------------------------------------------------------------------------ the carve itself
def _ws_bytes(ctx, B, N=0, Tm=0):
    need = C.c_size_t(0)
    ctx._check(ctx.lib.si_workspace_bytes(ctx._h, B, N, Tm, C.byref(need)), "si_workspace_bytes")
    return int(need.value)


def _mel_ws_bytes(ctx, B, N22):
    need = C.c_size_t(0)
    ctx._check(ctx.lib.si_mel_workspace_bytes(ctx._h, B, N22, C.byref(need)), "si_mel_workspace_bytes")
    return int(need.value)


@pytest.mark.parametrize("value,zone", [("0", 0), ("255", 0), ("1000", 768), ("65536", 65536), ("1048576", 1 << 20), ("5000000", 1 << 20), ("-4096", 0)])
def test_the_switch_is_rounded_down_to_256_and_capped_at_1_mib(value, zone):
    """SI_WS_REDZONE as si_create reads it, seen through the sizes it adds: 5 zones to the mel front-end's estimate, 18 and 15 to the others'."""
    from speech_inpainting_amd.arch import VocoderArch
    from speech_inpainting_amd.native import NativeContext, make_desc
    sizes = []
    for env in ({}, {"SI_WS_REDZONE": value}):
        with scoped_env(env):
            ctx = NativeContext(make_desc(_tiny(), VocoderArch.tiny(), 50), torch.device("cuda:0"))
        try:
            sizes.append((_mel_ws_bytes(ctx, 3, 22063), _ws_bytes(ctx, 3, N=8000), _ws_bytes(ctx, 3, Tm=57)))
        finally:
            ctx.close()
    assert [a - b for a, b in zip(sizes[1], sizes[0])] == [5 * zone, 18 * zone, 15 * zone], (value, sizes)


def test_regions_are_laid_out_as_stated_and_the_zones_change_no_value():
    """With R: offset[0] = R and offset[i + 1] = align_up(offset[i] + bytes[i], 256) + R (_guard holds every route to that).  An engine at
    R = 0: the same names and bytes at consecutive 256-aligned offsets, and outputs bit-identical to the R engine's.  For each pass
    ws_bytes(R) - ws_bytes(0) = R k with one k over all shapes."""
    from speech_inpainting_amd import synth
    harch = _tiny()
    runs = []
    for env in (ZONE, {}):
        enc, (voc, varch), mel = _enc_engine(harch, "bf16", env), _voc_engine("v1", "fp16", env), _mel_engine(env)
        wave, lens = synth.synth_wave(3, 8000, 11).cuda(), [8000, 400, 4445]
        w22, m = synth.synth_wave(3, 22063, 21, sr=22050).cuda(), _ragged_mel(varch)
        passes = {("encoder", "uniform"): (enc, lambda: enc.encode(wave)), ("encoder", "ragged"): (enc, lambda: enc.encode_ragged(wave, lens)),
                  ("vocoder", "uniform"): (voc, lambda: voc.vocode(m)), ("vocoder", "ragged"): (voc, lambda: voc.vocode_ragged(m, VOC_RAGGED)),
                  ("mel", "uniform"): (mel, lambda: mel.mel(w22)), ("mel", "ragged"): (mel, lambda: mel.mel_ragged(w22, [22063, 400, 9999]))}
        got = {}
        for key, (eng, run) in passes.items():
            out = run()
            torch.cuda.synchronize()
            regions = eng.ctx.ws_regions(key[0])
            _laid_out(regions, R if env else 0)
            got[key] = (out.cpu(), regions)
        sizes = {"encoder": [_ws_bytes(enc.ctx, B, N=N) for B in (1, 3, 32) for N in (400, 8000, 48000)],
                 "vocoder": [_ws_bytes(voc.ctx, B, Tm=Tm) for B in (1, 3, 32) for Tm in (1, 57, 500)],
                 "mel": [_mel_ws_bytes(mel.ctx, B, N) for B in (1, 3, 32) for N in (400, 22063, 66150)]}
        runs.append((got, sizes))
    (zoned, big), (plain, small) = runs
    for key in zoned:
        assert torch.equal(P.bits(zoned[key][0]), P.bits(plain[key][0])), (key, "the zones changed a value")
        assert [(n, b) for n, _, b in zoned[key][1]] == [(n, b) for n, _, b in plain[key][1]], key
    for which in big:
        ks = {(a - b) // R for a, b in zip(big[which], small[which])}
        assert all((a - b) % R == 0 for a, b in zip(big[which], small[which])) and len(ks) == 1, (which, ks)
        most = max(len(regions) for (p, _), (_, regions) in zoned.items() if p == which)
        print(f"   {which}: ws_bytes(R) - ws_bytes(0) = {ks.pop()} R; the routes here carve at most {most} regions")


def test_the_estimate_covers_the_carve():
    """The tiny pair at R = 65536 over B = 1, 2, 5, 32 and lengths from one frame to 3 s, uniform, padded and ragged: no call is refused
    with "exceeded its own estimate" (any refusal raises).  The largest part of an estimate that its carve left unused is printed."""
    from speech_inpainting_amd import synth
    enc, (voc, varch), mel = _enc_engine(_tiny(), "bf16", ZONE), _voc_engine("v1", "fp16", ZONE), _mel_engine(ZONE)
    spare = {"encoder": 0, "vocoder": 0, "vocoder, unstretched": 0, "mel": 0}   # (si_workspace_bytes sizes the generator for the stretch)

    def ran(eng, which, need, key=None):
        r = eng.ctx.ws_regions(which)
        used = _up(r[-1][1] + r[-1][2]) + R
        assert used <= need, (which, used, need)
        spare[key or which] = max(spare[key or which], need - used)

    for B in (1, 2, 5, 32):
        for N in (400, 401, 8000, 48000):
            wave = synth.synth_wave(B, N, B + N).cuda()
            lens = ([N, 400, max(400, (N * 5 // 9) | 1)] * B)[:B]
            for run in (lambda: enc.encode(wave), lambda: enc.encode(wave, valid_len=_i32(lens)), lambda: enc.encode_ragged(wave, lens)):
                run()
                ran(enc, "encoder", _ws_bytes(enc.ctx, B, N=N))
        for Tm in (1, 2, 57, 500):
            if B * Tm > 5 * 500:
                continue                                            # (B = 32 at 500 frames: 16 clips' worth of the V1 generator says nothing new)
            m = cases._mel(B, Tm, B + Tm, varch.num_mels).cuda()
            lens = ([Tm, 1, (Tm * 5 // 9) | 1] * B)[:B]
            for stretch in (True, False):
                for run in (lambda: voc.vocode(m, stretch), lambda: voc.vocode_ragged(m, lens, stretch)):
                    run()
                    ran(voc, "vocoder", _ws_bytes(voc.ctx, B, Tm=Tm), "vocoder" if stretch else "vocoder, unstretched")
        for N22 in (400, 401, 22063, 66150):
            w = synth.synth_wave(B, N22, B + N22, sr=22050).cuda()
            lens = ([N22, 400, max(400, (N22 * 5 // 9) | 1)] * B)[:B]
            for run in (lambda: mel.mel(w), lambda: mel.mel_ragged(w, lens)):
                run()
                ran(mel, "mel", _mel_ws_bytes(mel.ctx, B, N22))
    torch.cuda.synchronize()
    print(f"   largest unused remainder of an estimate, bytes: {spare}")


def test_the_checker_bites_on_the_real_workspace():
    """The premise of every test above: after a real pass one byte written with torch into a zone, into the slack behind a region's
    requested bytes, behind the last region's zone and into a band fails its check, which names the place."""
    from speech_inpainting_amd import synth
    eng = _enc_engine(_tiny(), "bf16", ZONE)
    ctx = eng.ctx
    wave = synth.synth_wave(3, 8000, 11).cuda()
    eng.encode(wave)
    for fill in X.FILLS:
        stray = X.FILLS[0] if fill != X.FILLS[0] else X.FILLS[1]
        ws = ctx._ws
        ws.fill_(fill)
        with X.guarded_allocs(fill) as rec:
            eng.encode(wave)
            torch.cuda.synchronize()
        regions = ctx.ws_regions("encoder")
        X.check_workspace(ws, regions, fill)
        rec.check()
        written = int((ws != fill).sum())
        assert 0 < written <= sum(r[2] for r in regions) < ws.numel()
        by = {r[0]: r for r in regions}
        slack = next(r for r in regions if r[2] % 256)               # a region whose bytes end inside a 256-byte line
        last = regions[-1]
        places = {"zone": (by["h"][1] - 1, f"behind the requested {by['lnf'][2]} bytes of region 'lnf'"),
                  "front": (R - 1, "in front of the first region"),
                  "slack": (slack[1] + slack[2], f"0 bytes behind the requested {slack[2]} bytes of region {slack[0]!r}"),
                  "rest": (ws.numel() - 1, f"behind the requested {last[2]} bytes of region {last[0]!r}")}
        assert ws.numel() - 1 >= _up(last[1] + last[2]) + R - 1
        for what, (at, words) in places.items():
            ws[at] = stray
            with pytest.raises(AssertionError, match=f"workspace byte {at} holds {stray:#04x}.*{words}"):
                X.check_workspace(ws, regions, fill)
            ws[at] = fill
            X.check_workspace(ws, regions, fill)
        raw, nbytes = rec.allocs[-1][0], rec.allocs[-1][1]
        for at, words in ((R - 1, "byte 1 in front of the tensor"), (R + nbytes, "byte 0 behind the tensor's end")):
            raw[at] = stray
            with pytest.raises(AssertionError, match=words):
                rec.check()
            raw[at] = fill
        rec.check()


# ------------------------------------------------------------------------------------------------------------ coverage
def test_zz_every_scratch_family_with_a_pointer_ran_between_zones():
    """(last in the file) the families launched above hold every entry of poison.SCRATCH_FAMILIES except the library-owned ones:
    ctx->km_cnorm and ctx->det_scratch have no pointer a test can read."""
    missing = set(P.SCRATCH_FAMILIES) - LIBRARY_OWNED - FAMILIES
    print(f"   families launched between zones: {len(FAMILIES & set(P.SCRATCH_FAMILIES))} of {len(P.SCRATCH_FAMILIES) - len(LIBRARY_OWNED)} with "
          f"caller-owned scratch; the file took {time.time() - T0:.1f} s")
    assert not missing, f"scratch families this file never launched: {sorted(missing)}"
