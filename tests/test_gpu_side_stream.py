"""every pass enqueues on the caller's stream, and does not wait for it.

Each case runs through tests/side_stream.py's behind_a_delay: once on the default stream (the baseline), then on a side stream
(one under whose pending work stream 0 is seen to run) behind a torch.cuda._sleep of 100 ms, where the real inputs arrive and the workspaces are poisoned only BEHIND that delay -- a launch,
a memset or a copy that went to another stream works on the decoy inputs or on old scratch, and its result is poisoned afterwards.
The outputs must be the baseline's bits, and the call must have come back to the host while the delay was still running.  A second
delayed run of each case is profiled (si_profile_stop waits by design, so that run is not held to the no-wait half): the last test
holds the families launched there against poison.SCRATCH_FAMILIES and NO_SCRATCH_FAMILIES, and the entry points each case called
against side_stream.COVERED.  The shapes are those of tests/routes.py, the smallest that reach each route."""
import time

import numpy as np
import pytest
import torch

from tests import cases
from tests import poison as P
from tests import side_stream as S
from tests.harness import build_engine, scoped_env
from tests.routes import (VOC_CONFIGS, VOC_RAGGED, _base, _enc_engine, _encoder_entries, _i32, _large, _mel_engine, _mel_entries, _ragged_mel, _tiny,
                          _uniform_mel, _voc_engine, _voc_id)
from tests.test_gpu_scratch import BASE_ENVS

pytestmark = pytest.mark.gpu

T0 = time.time()
FAMILIES = set()                                       # poison.family_of(name) of every launch profiled behind a delay
CALLS = {}                                             # case label -> the entry points of side_stream.COVERED it called behind a delay
ROUTES = set()                                         # side_stream.SHARED_FAMILY_ROUTES entries that ran behind a delay
SIGHT = {}                                             # seeded mistake -> behind_a_delay raised on bits
N_FILE = 2 * 2048 + 77                                 # two chunk seams of every file kernel


# ------------------------------------------------------------------------------------------------------------ the harness sees
def _chain(x, mistake=None):
    """Three torch ops -- a = 2 x + 1; b = a * flip(a); out = zeros(n + 8) with out[:n] = b * b -- with one seeded mistake."""
    def run():
        if mistake == "sync":
            torch.cuda.current_stream().synchronize()
        a = x * 2.0 + 1.0
        if mistake == "middle":
            with torch.cuda.stream(torch.cuda.default_stream()):
                b = a * torch.flip(a, (0,))
        else:
            b = a * torch.flip(a, (0,))
        out = torch.empty(x.numel() + 8, dtype=torch.float32, device=x.device)
        if mistake == "zero":
            with torch.cuda.stream(torch.cuda.default_stream()):
                out.zero_()
        else:
            out.zero_()
        out[:x.numel()] = b * b
        return out
    return run


def _chain_input():
    return (torch.arange(4101, dtype=torch.float32) % 7 - 3.0).cuda() * 0.125


def _raises_on_bits(mistake):
    if mistake not in SIGHT:
        x = _chain_input()
        try:
            S.behind_a_delay(_chain(x, mistake), [x], no_wait=False, label=f"self-test {mistake}")
            SIGHT[mistake] = False
        except AssertionError as e:
            SIGHT[mistake] = "behind a delay on a side stream changes" in str(e)
    return SIGHT[mistake]


def _sight():
    """Every test below: skipped, not passed, unless the two seeded stream mistakes are seen."""
    if not (_raises_on_bits("middle") and _raises_on_bits("zero")):
        pytest.skip("the probe is blind: a seeded launch on the default stream was not seen (torch's side streams wait for stream 0 here?)")


def test_00a_a_middle_op_on_the_default_stream_is_seen():
    assert _raises_on_bits("middle"), "the probe is blind: the middle op of three ran on the default stream and the bits did not change"


def test_00b_an_output_zeroed_on_the_default_stream_is_seen():
    assert _raises_on_bits("zero"), "the probe is blind: the output was zeroed on the default stream and the bits did not change"


def test_00c_a_pass_that_synchronises_its_stream_is_seen():
    x = _chain_input()
    with pytest.raises(AssertionError, match="waited for the caller's stream"):
        S.behind_a_delay(_chain(x, "sync"), [x], label="self-test sync")


def test_00d_the_correct_chain_passes_and_returns_the_baseline():
    x = _chain_input()
    base = S.behind_a_delay(_chain(x), [x], label="self-test correct")["out"]
    a = x.cpu() * 2.0 + 1.0
    b = a * torch.flip(a, (0,))
    want = torch.cat([b * b, torch.zeros(8)])
    assert base.shape == want.shape and torch.allclose(base, want, rtol=1e-6, atol=0.0) and not bool(base[-8:].any())
    assert torch.equal(x.cpu(), _chain_input().cpu()), "the inputs were not put back"
    assert S.LOG[-1][3] and 50.0 <= S.LOG[-1][2] <= S.DELAY_CAP_MS, S.LOG[-1]


# ------------------------------------------------------------------------------------------------------------ one case
def _case(label, run, inputs, ctx, no_wait=True, routes=(), **kw):
    """run() behind a delay, then once more behind a delay with the launches profiled -> the baseline."""
    _sight()
    with S.calls_recorded(ctx.lib) as seen:
        base = S.behind_a_delay(run, inputs, ctx, no_wait=no_wait, label=label, **kw)
    CALLS[label] = set(seen)
    ctx.profile_start(4000)
    try:
        S.behind_a_delay(run, inputs, ctx, no_wait=False, baseline=base, label=label + " (profiled)", **kw)
    finally:
        prof = ctx.profile_stop()
    for e in prof:
        fam = P.family_of(e["name"])
        assert fam is not None, f"launch {e['name']!r} is in neither family list of tests/poison.py"
        FAMILIES.add(fam)
    assert prof, (label, "nothing was launched")
    ROUTES.update(routes)
    return base


# ------------------------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_tiny_encoder_every_entry_point(math):
    harch = _tiny()
    eng = _enc_engine(harch, math)
    entries, wave, _, _ = _encoder_entries(eng, harch, 3, 8000, 11)
    for name, run in entries.items():
        _case(f"encoder tiny {math} {name}", run, [wave], eng.ctx)


@pytest.mark.parametrize("env", BASE_ENVS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_base_encoder_bf16_routes(env):
    """Every entry point on the default route, one case each; under a switch the uniform and the ragged pass in one case."""
    harch = _base()
    eng = _enc_engine(harch, "bf16", env)
    entries, wave, _, _ = _encoder_entries(eng, harch, 3, 24000, 12, only=None if not env else ("forward", "varlen"))
    if not env:
        for name, run in entries.items():
            _case(f"encoder base bf16 {name}", run, [wave], eng.ctx)
    else:
        tag = ",".join(f"{k}={v}" for k, v in env.items())
        _case(f"encoder base bf16 {tag}", lambda: {k: f() for k, f in entries.items()}, [wave], eng.ctx)


def test_large_encoder_and_tiled_attention():
    """HuBERT-large's widths (posconv's 64-channel groups); and T = 257 frames on the base widths: the tiled attention kernel."""
    from speech_inpainting_amd import synth
    harch = _large()
    eng = _enc_engine(harch, "bf16")
    entries, wave, _, _ = _encoder_entries(eng, harch, 2, 16000, 13, only=("forward", "padded", "varlen", "extract"))
    _case("encoder large bf16", lambda: {k: f() for k, f in entries.items()}, [wave], eng.ctx)
    harch = _base()
    eng = _enc_engine(harch, "bf16")
    N = 320 * 256 + 400
    assert harch.num_frames(N) == 257
    long = synth.synth_wave(2, N, 14).cuda()
    _case("encoder base bf16 T=257", lambda: eng.encode(long), [long], eng.ctx)


# ------------------------------------------------------------------------------------------------------------ generator
SIDE_VOC = VOC_CONFIGS + [("v1", "fp16", {"SI_VOC_UPSGEMM": "0"})]


@pytest.mark.parametrize("cfg", SIDE_VOC, ids=_voc_id)
def test_generator_uniform_and_ragged_chunked(cfg):
    """vocoder_chunk = 2 on B = 3: two chunks per pass, the second in the buffers the first left.  V1's four stages are the widths
    C = 256 / 128 / 64 / 32; the default route holds reschain and the gemmcu upsampler, SI_VOC_UPSGEMM=0 upsample.hip."""
    arch, math, env = cfg
    eng, varch = _voc_engine(arch, math, env, 2)
    mel = _uniform_mel(varch, 57)
    _case(f"generator {_voc_id(cfg)} uniform", lambda: eng.vocode(mel, True), [mel], eng.ctx)
    rag = _ragged_mel(varch)
    _case(f"generator {_voc_id(cfg)} ragged", lambda: {"stretch": eng.vocode_ragged(rag, VOC_RAGGED, True), "plain": eng.vocode_ragged(rag, VOC_RAGGED, False)},
          [rag], eng.ctx)


# ------------------------------------------------------------------------------------------------------------ mel front-end, F0 encoder
def test_mel_frontend_all_three_forms():
    eng = _mel_engine()
    uniform, ragged, wave, _ = _mel_entries(eng, 22064)
    for i, run in enumerate(uniform):
        _case(f"mel uniform {i}", run, [wave], eng.ctx)
    for name, run in ragged.items():
        _case(f"mel ragged {name}", lambda: run(wave), [wave], eng.ctx)


@pytest.mark.parametrize("T", [877, 878])
def test_f0_encoder_both_routes(T):
    from speech_inpainting_amd import native, synth
    from speech_inpainting_amd.engine import pack_f0_encoder
    desc = native.F0EncDesc()
    ctx = _mel_engine().ctx
    w = pack_f0_encoder(synth.synth_f0_vqvae_state(desc, 20, seed=5), desc).cuda()
    f0 = (torch.randn(2, desc.in_width, T, generator=torch.Generator().manual_seed(T)).abs() * 2.0).cuda()
    _case(f"f0 encoder T={T}", lambda: ctx.f0_encoder(desc, w, f0), [f0], ctx)
    assert ("f0enc_fused" if T <= 877 else "f0enc_conv1d") in FAMILIES


# ------------------------------------------------------------------------------------------------------------ small operations
def _randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _randint(hi, *shape, seed):
    return torch.randint(0, hi, shape, generator=torch.Generator().manual_seed(seed)).cuda()


def test_codebook_calls_in_grid_and_table_form():
    ctx = _mel_engine().ctx
    feats, melf = _randn(3, 24, 80, seed=33), cases._mel(3, 30, 34).cuda()
    pos, cnt, lm = _i32([3, 0, 10]), _i32([5, 0, 2]), 5
    target = _randint(50, 3, lm, seed=35)

    def grid():
        m1, m2, m3 = melf.clone(), melf.clone(), melf.clone()
        out = {"labels": ctx.codebook_splice(feats, pos, lm, m1), "labels_varlen": ctx.codebook_splice_varlen(feats, pos, cnt, lm, m2)}
        ctx.codebook_splice_labels(target, pos, m3)
        out.update(m1=m1, m2=m2, m3=m3)
        out.update({f"metrics{i}": t for i, t in enumerate(ctx.codebook_metrics(feats, pos, lm, target))})
        return out
    _case("codebook grid", grid, [feats, melf], ctx)
    clip, frame, tflat = _i32([0, 0, 1, 2, 2]), _i32([3, 4, 0, 10, 11]), _randint(50, 5, seed=36)

    def table():
        m1, m2 = melf.clone(), melf.clone()
        out = {"labels": ctx.codebook_splice_spans(feats, clip, frame, m1), "m1": m1, "m2": m2}
        ctx.codebook_splice_labels_spans(tflat, clip, frame, m2)
        out.update({f"metrics{i}": t for i, t in enumerate(ctx.codebook_metrics_spans(feats, clip, frame, tflat))})
        return out
    _case("codebook table", table, [feats, melf], ctx)


def test_unit_calls_kmeans_and_metrics():
    ctx = _mel_engine().ctx
    clean, masked = _randint(11, 3, 300, seed=1), _randint(11, 3, 300, seed=2)
    first, last = _i32([3, 0, 100]), _i32([8, 0, 300])
    code, f0c = _randint(11, 3, 257, seed=3), _randint(7, 3, 257, seed=4)
    emb_c, emb_p, spk = _randn(11, 8, seed=5), _randn(7, 8, seed=6), _randn(3, 8, seed=7)
    _case("units", lambda: {"code": ctx.code_splice(clean, masked, first, last), "front": ctx.unit_frontend(code, emb_c, f0c, emb_p, spk)},
          [clean, masked, emb_c, emb_p, spk], ctx)
    x, cent = _randn(300, 768, seed=8), _randn(50, 768, seed=9)
    _case("kmeans mfma", lambda: ctx.kmeans_assign(x, cent, with_distance=True), [x, cent], ctx, owned_scratch=True)
    with scoped_env({"SI_KMEANS_MFMA": "0"}):
        _case("kmeans scalar", lambda: ctx.kmeans_assign(x, cent, with_distance=True), [x, cent], ctx, owned_scratch=True)
    a, b = cases._mel(3, 30, 7).cuda(), cases._mel(3, 30, 8).cuda()
    est, ref = _randn(3, 4101, seed=10), _randn(3, 4101, seed=11)
    _case("metrics", lambda: {"mel": ctx.mel_metrics(a, b), "sisdr": ctx.sisdr(est, ref)}, [a, b, est, ref], ctx)


def test_resamplers_pcm16_and_extend_mel():
    from speech_inpainting_amd import audio, synth
    eng = _mel_engine()
    ctx = eng.ctx
    x = synth.synth_wave(3, 9000, 31, sr=22050).cuda()
    n_len = _i32([9000, 1, 4321])
    eng.resample(x, 22050, 16000)                                                   # the time registers reach their length here
    eng.resample(x, 22050, 16000, kind="poly")                                      # and the tap table is designed and uploaded
    f = eng._sinc_tables(22050, 16000)
    n_out = audio.resampled_len(9000, 22050, 16000)
    _case("resamplers", lambda: {"poly": eng.resample(x, 22050, 16000, kind="poly"), "sinc": ctx.resample_sinc(x, f, n_out, n_len)}, [x], ctx)
    wav, mel = _randn(3, 4101, seed=12, scale=0.3), cases._mel(3, 57, 13).cuda()
    _case("pcm16 and extend_mel", lambda: {"pcm": ctx.pcm16(wav), "ext": ctx.extend_mel(mel)}, [wav, mel], ctx)


def test_patch_mode_and_long_recordings():
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import native, synth
    eng = _mel_engine()
    ctx, dev = eng.ctx, eng.device
    B, N, fade = 3, 9000, 110
    lens, wl = [9000, 1, 4321], [8000, 1, 4200]
    wave, gen = synth.synth_wave(B, N, 31, sr=22050).cuda(), synth.synth_wave(B, N, 32, sr=22050).cuda()
    len_dev = _i32(lens)
    tab = native.SpanTable([[(1000, 300)], [], [(4000, 321)]], dev)
    patch = native.PatchTable([(b, 0, min(wl[b], N)) for b in range(B)], [0, 2], [min(n, w) for n, w in zip(lens, wl)], fade, dev)
    ext = ctx.extend_mel(cases._mel(3, 57, 14).cuda())
    wins = [(0, 0, 10), (2, 50, ext.shape[2]), (1, 5, 6)]
    host = ctx.window_words(wins)
    words = (host, torch.from_numpy(host).cuda())
    torch.cuda.synchronize()

    def patch_mode():
        f32, pcm = ctx.patch_compose(wave, tab, patch, gen, None, sample_len=lens, f32=True, pcm=True)
        return {"peak": ctx.wave_peak(wave, tab, len_dev), "peak_plain": ctx.wave_peak(wave, None, len_dev), "windows": ctx.gather_windows(ext, wins, tab=words),
                "patched": f32, "pcm": pcm}
    _case("patch mode", patch_mode, [wave, gen, ext], ctx)

    src = wave[0].clone()
    src[77] = 0.99
    s, l = 5000, 700
    ws = s - fade - 3
    region = native.RegionTable([(s, l, 0, N)], [(0, ws, N - ws)], G.region_chunks(G.file_regions([(s, l)], [N], fade)), 1, fade, dev)
    row, gain = gen[1, :N - ws + 5].reshape(1, -1).contiguous(), torch.tensor([0.8]).cuda()
    starts = [0, 4000, N - 2049]
    torch.cuda.synchronize()

    def long_recordings():
        out = src.clone()
        ctx.patch_regions(src, region, row, gain, out)
        return {"clips": ctx.cut_clips(src, starts, 2049), "valid": ctx.cut_clips_valid(src, starts, 2049, 0.5), "patched": out}
    _case("long recordings", long_recordings, [src, row], ctx)


# ------------------------------------------------------------------------------------------------------------ file kernels
def _files(seed, nan=False):
    """{(sample type, channels): the file on the device}: N_FILE sample times of a tone under a little noise with quiet and held runs on and
    across the 8-sample, 512-sample and chunk seams, one quiet stretch longer than the level window, and three clicks, as fp32, int16 and
    packed 24-bit, mono (channels 0) and three channels interleaved."""
    from tests import s24_ref
    out = {}
    for ch in (0, 3):
        rng = np.random.default_rng(seed + ch)
        k = np.arange(N_FILE)[:, None]
        x = 0.5 * np.sin(2.0 * np.pi * k / 57.0 + np.arange(max(ch, 1))[None, :]) + rng.uniform(-0.01, 0.01, (N_FILE, max(ch, 1)))
        for s in (0, 7, 511, 2047, 2048, 4095, N_FILE - 5):
            x[s:s + 6] = 0.0
        x[1000:1100] = 0.0
        for s in (20, 2040, 4090, N_FILE - 12):
            x[s:s + 9] = x[s]
        for s in (300, 2500, 4100):
            x[s] = 0.95 * np.sign(x[s] + 1e-9) * -1.0
        x = x if ch else x[:, 0]
        f32 = x.astype(np.float32)
        if nan:
            f32 = f32.copy()
            f32.reshape(N_FILE, -1)[[100, 2047, 2048, 4096]] = np.nan
            f32.reshape(N_FILE, -1)[[101, N_FILE - 1]] = np.inf
        out["fp32", ch] = torch.from_numpy(np.ascontiguousarray(f32)).cuda()
        out["int16", ch] = torch.from_numpy(np.ascontiguousarray((x * 32767).astype(np.int16))).cuda()
        out["s24", ch] = torch.from_numpy(np.ascontiguousarray(s24_ref.pack((x * 8388607).astype(np.int64)))).cuda()
    return out


UNIT = {"fp32": 1.0, "int16": 32768.0, "s24": 8388608.0}   # full scale in the file's own steps


def _channels(ch, joint):
    return [None] if not ch else [0, ch - 1] + ([-1] if joint else [])


DETECTORS = {
    "quiet": (True, lambda ctx, x, u, c, T: ctx.quiet_runs(x, 1e-4 * u, 2, 64, channel=c)),
    "dead": (True, lambda ctx, x, u, c, T: ctx.dead_runs(x, threshold=1e-4 * u, rel_threshold=0.01, held_tol=0.0, min_len=2, max_runs=64, channel=c, threshold_out=T)),
    "level": (False, lambda ctx, x, u, c, T: ctx.level_runs(x, half=8, threshold=1e-4 * u, rel_threshold=0.01, min_len=2, max_runs=64, channel=c, threshold_out=T)),
    "burst": (False, lambda ctx, x, u, c, T: ctx.burst_runs(x, half=8, threshold=0.3 * u, rel_threshold=0.01, min_len=2, max_runs=64, channel=c, threshold_out=T)),
    "invalid": (True, lambda ctx, x, u, c, T: ctx.invalid_runs(x, ceiling=0.9 * u, min_len=1, max_runs=64, channel=c)),
    "impulse": (False, lambda ctx, x, u, c, T: ctx.impulse_runs(x, order=8, half=64, rel_threshold=0.01, min_len=1, max_runs=64, channel=c, threshold_out=T)),
}


@pytest.mark.parametrize("det", list(DETECTORS))
def test_detector_routes(det):
    """One case per detector route: fp32, int16 and packed 24-bit, mono and three channels (the first, the last and, where the route
    has one, the joint form).  The scratch is the library's own: it holds the decoy's results when the delayed run starts."""
    ctx = _mel_engine().ctx
    files = _files(40, nan=det == "invalid")
    joint, call = DETECTORS[det]

    def run():
        out = {}
        for (kind, ch), x in files.items():
            for c in _channels(ch, joint):
                T = torch.empty(1, dtype=torch.float32, device=x.device)
                runs, n = call(ctx, x, UNIT[kind], c, T)
                out.update({f"{kind} {ch} {c} runs": runs, f"{kind} {ch} {c} n": n})
                if det not in ("quiet", "invalid"):
                    out[f"{kind} {ch} {c} T"] = T
        return out
    base = _case(f"detector {det}", run, list(files.values()), ctx, owned_scratch=True,
                 routes={"quiet": ("quiet", "quiet_ch"), "invalid": ("invalid", "invalid_ch"), "dead": ("dead", "dead_ch")}.get(det, (det,)))
    found = sum(int(v[0]) for k, v in base.items() if k.endswith(" n"))
    print(f"   detector {det}: {found} runs over {len(base)} outputs")
    assert found > 0, (det, "no run was found in a file that holds some")


def test_residual_mend_and_patch_rate():
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import native
    from tests import feed_ref as F
    eng = _mel_engine()
    ctx, dev = eng.ctx, eng.device
    files = _files(41)

    def residual():
        return {f"{kind} {ch} {c}": ctx.impulse_residual(x, order=8, channel=c) for (kind, ch), x in files.items() for c in _channels(ch, False)}
    _case("impulse residual", residual, list(files.values()), ctx, routes=("impulse residual",))
    rows = torch.tensor([[100, 5], [2046, 6], [4000, 3]], dtype=torch.int32).cuda()

    def mend():
        out = {}
        for (kind, ch), x in files.items():
            for c in _channels(ch, False):
                y = x.clone()
                out[f"{kind} {ch} {c} status"] = ctx.mend_runs(y, rows, channel=c)
                out[f"{kind} {ch} {c}"] = y
        return out
    _case("mend runs", mend, list(files.values()), ctx, routes=("mend_runs",))
    sr = 48000
    fade_f, filt = G.file_fade(5.0, sr), eng._rate_filter(sr)
    P22, Q22 = G.rate_ratio(sr)
    N22 = F.n22(N_FILE, sr)
    s, l = N_FILE - 700, 700
    ws = (s - fade_f) * P22 // Q22 - filt["reach"] - 2
    wl = N22 - ws
    assert ws > 0 and s < 4096 < s + l
    gen = _randn(1, wl + 5, seed=3, scale=0.3)
    table = native.RateTable([(s, l, 0, N_FILE)], [(0, ws, wl, N22)], G.region_chunks(G.file_regions([(s, l)], [N_FILE], fade_f)), 1, fade_f, dev)
    torch.cuda.synchronize()

    def patch():
        out = {}
        for (kind, ch), x in files.items():
            for c in _channels(ch, False)[-1:]:
                y = x.clone()
                ctx.patch_rate(x, sr, table, gen, filt, y, None, channel=c)
                out[f"{kind} {ch} {c}"] = y
        return out
    base = _case(f"patch rate {sr}", patch, list(files.values()) + [gen], ctx, routes=("patch_rate",))
    assert not torch.equal(base["int16 0 None"][s:], files["int16", 0].cpu()[s:]), "the span was not written"


@pytest.mark.parametrize("sr", [48000, 16000])
def test_cut_rate_and_cut_pair(sr):
    """si_cut_rate, _ch and _valid, then si_cut_pair, _ch and _valid, from every sample type: two clips, the first of the recording and one
    that ends with its 22.05 kHz axis (the pair: frames 0 and 1)."""
    from tests import feed_ref as F
    eng = _mel_engine()
    ctx = eng.ctx
    files = _files(42, nan=True)
    f22, f16 = eng._feed_filter(sr), eng._feed_filter16(sr)
    N22 = F.n22(N_FILE, sr)
    starts = [0, N22 - 441]
    torch.cuda.synchronize()

    def rate():
        out = {}
        for (kind, ch), x in files.items():
            c = ch - 1 if ch else None
            out[f"{kind} {ch}"] = ctx.cut_rate(x, sr, starts, 441, f22, channel=c)
            out[f"{kind} {ch} valid"] = ctx.cut_rate_valid(x, sr, starts, 441, f22, 0.9 * UNIT[kind], channel=c)
        return out
    _case(f"cut rate {sr}", rate, list(files.values()), ctx, routes=("cut_rate", "cut_rate_ch"))

    def pair():
        out = {}
        for (kind, ch), x in files.items():
            c = ch - 1 if ch else None
            out[f"{kind} {ch} 22"], out[f"{kind} {ch} 16"] = ctx.cut_pair(x, sr, [0, 1], 441, 320, f22, f16, channel=c)
            out[f"{kind} {ch} valid 22"], out[f"{kind} {ch} valid 16"] = ctx.cut_pair_valid(x, sr, [0, 1], 441, 320, f22, f16, 0.9 * UNIT[kind], channel=c)
        return out
    _case(f"cut pair {sr}", pair, list(files.values()), ctx, routes=("cut_pair", "cut_pair_ch"))


# ------------------------------------------------------------------------------------------------------------ engine routes
def _step_engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.tiny(), 50, "bf16", "fp16", key=("test_gpu_side_stream", "step"))


def test_one_inpaint_step_uniform_and_ragged():
    """Python's own torch ops follow the current stream; these routes copy counts and tables between host and device by design, so they are
    held to the bits alone."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.predict import pad_stack
    eng = _step_engine()
    wave16, wave22, pos = synth.synth_wave(2, 17600, 800).cuda(), synth.synth_wave(2, 24255, 1300, sr=22050).cuda(), _i32([12, 8])
    _case("inpaint uniform", lambda: eng.predict_batch(wave16, eng.mel(wave22), pos, 5), [wave16, wave22], eng.ctx, no_wait=False)
    w16 = [synth.synth_wave(1, int(round(s * 16000)), 800 + i)[0].numpy() for i, s in enumerate([1.1, 0.6])]
    w22 = [synth.synth_wave(1, -(-len(w) * 441 // 320), 1300 + i, sr=22050)[0].numpy() for i, w in enumerate(w16)]
    (r16, len16), (r22, len22) = pad_stack(w16), pad_stack(w22)
    r16, r22 = r16.cuda(), r22.cuda()
    mel_len = [eng.ctx.mel_frames(n) for n in len22]
    _case("inpaint ragged", lambda: eng.predict_ragged_batch(r16, len16, eng.mel_ragged(r22, len22), mel_len, pos, 5), [r16, r22], eng.ctx, no_wait=False)


def test_ida_inpaint_batch_with_its_side_stream():
    """engine.ida_inpaint_batch runs the F0 encoder on the engine's own side stream under the HuBERT pass: both hang off the caller's."""
    from speech_inpainting_amd.arch import HubertArch
    from speech_inpainting_amd.engine import CodeGenerator, F0Quantizer, InpaintingEngine
    from tests.test_gpu_ida import _ida_setup
    harch, K = HubertArch.tiny(), 50
    varch, hsd, gsd, f0sd, emb_c, emb_p, spk, wave, f0 = _ida_setup(harch, 2, 9600, 77, K)
    eng = InpaintingEngine(harch, varch, K, "cuda:0", "fp32", "fp32").load_state(hsd, gsd)
    try:
        gen = CodeGenerator(eng, emb_c, emb_p, f0_quantizer=F0Quantizer(eng, f0sd))
        cent = _randn(K, harch.hidden_size, seed=5)
        wave, f0, spk = wave.cuda(), f0.cuda().contiguous(), spk.cuda()
        _case("ida inpaint", lambda: eng.ida_inpaint_batch(wave, 3200, 1600, cent, gen, f0, spk, output_layer=1), [wave, f0], eng.ctx, no_wait=False,
              owned_scratch=True)
    finally:
        eng.ctx.close()


def test_file_routes_and_the_request_front():
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.stream import Request, RequestFront
    eng = _step_engine()
    sr = 48000
    x = (synth.synth_wave(1, sr // 2, 900, sr=sr)[0] * 20000).to(torch.int16)
    x[10 * 960:13 * 960] = 0
    x = x.cuda()
    _case("patch_file", lambda: eng.patch_file(x, sr, gaps=[(10, 3)]), [x], eng.ctx, no_wait=False)
    _case("conceal_file contexts", lambda: eng.conceal_file(x, sr, feed="contexts"), [x], eng.ctx, no_wait=False, owned_scratch=True)
    clips = lambda lens, seed: [synth.synth_wave(1, int(n), seed + i, sr=22050)[0].numpy() for i, n in enumerate(lens)]
    reqs = [Request(clips([22050, 26460], 1560), [8, 11], 5, tag=0), Request(clips([24255, 19845], 1570), gaps=[[(5, 5)], [(2, 3), (30, 4)]], tag=1)]

    def front():
        out = {}
        for r in RequestFront(eng, 22050, depth=2).run(reqs):
            out[f"labels {r.tag}"] = torch.as_tensor(r.labels)
            out.update({f"pcm {r.tag} {j}": torch.from_numpy(np.ascontiguousarray(p)) for j, p in enumerate(r.pcm)})
        return out
    _case("request front", front, [], eng.ctx, no_wait=False)


# ------------------------------------------------------------------------------------------------------------ the waits the header names
def _fresh_ctx():
    from speech_inpainting_amd.arch import VocoderArch
    from speech_inpainting_amd.native import NativeContext, make_desc
    return NativeContext(make_desc(_tiny(), VocoderArch.tiny(), 50), torch.device("cuda:0"))


def test_a_ragged_pass_waits_only_when_it_reuses_a_pinned_slot_that_is_still_behind_the_delay():
    """The length tables of the ragged passes rotate through VL_SLOTS pinned slots.  Behind ONE delay the first VL_SLOTS ragged calls
    return under it; the next one finds its slot's copy still queued behind the delay and waits for it."""
    _sight()
    eng = _mel_engine()
    _, _, wave, lens = _mel_entries(eng, 22064)
    base = eng.mel_ragged(wave, lens).cpu()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    e = torch.cuda.Event()
    outs, under = [], []
    with torch.cuda.stream(side):
        torch.cuda._sleep(S.cycles_for(S.DELAY_MS))
        e.record()
        for _ in range(S.VL_SLOTS + 1):
            outs.append(eng.mel_ragged(wave, lens))
            under.append(not e.query())
    side.synchronize()
    print(f"   ragged calls behind one delay returned under it: {under}")
    assert all(under[:S.VL_SLOTS]), under
    assert not under[S.VL_SLOTS], "the call that reuses the first slot did not wait for the copy queued in it"
    for o in outs:
        assert torch.equal(P.bits(o.cpu()), P.bits(base))


def test_library_owned_scratch_waits_when_it_grows_and_not_on_the_next_call():
    """After a small detector call a larger one, whose bitmap no longer fits ctx->det_scratch, behind a delay: it synchronises the stream
    before it frees the old block, and its result is still the right one; a second call of the larger size returns under the delay."""
    _sight()
    n_big = 5000 * 2048 + 77                                                        # a bitmap of more than the scratch's first 1 MiB
    small = _files(43)["fp32", 0]
    big = torch.rand(n_big, generator=torch.Generator().manual_seed(44)).cuda() - 0.5
    big[::99991] = 0.0
    call = lambda c, x: c.quiet_runs(x, 1e-6, 1, 256)
    fresh, used = _fresh_ctx(), _fresh_ctx()
    try:
        with P.poisoned_allocs():
            want = {k: v.cpu() for k, v in S.as_dict(call(fresh, big)).items()}
        call(used, small)
        torch.cuda.synchronize()
        assert 0 < int(want["out1"][0]) <= 256
        S.behind_a_delay(lambda: call(used, big), [big], used, no_wait=False, baseline=want, label="detector growth, first call")
        assert not S.LOG[-1][3], "the call that replaced ctx->det_scratch did not wait for the stream"
        S.behind_a_delay(lambda: call(used, big), [big], used, no_wait=True, baseline=want, owned_scratch=True, label="detector growth, second call")
    finally:
        fresh.close()
        used.close()


# ------------------------------------------------------------------------------------------------------------ the ledger
def test_zz_every_family_and_every_entry_point_ran_behind_a_delay():
    """(last in the file) the families profiled behind a delay hold poison.SCRATCH_FAMILIES and NO_SCRATCH_FAMILIES; every route that
    shares a family name with another was marked by its own case; every entry point of side_stream.COVERED was called behind a delay by
    the case the table names."""
    print(f"   {'case':<44} {'host ms':>8} {'delay ms':>9}  under the delay")
    for label, enqueue, slept, under in S.LOG:
        print(f"   {label:<44} {enqueue:8.2f} {slept:9.1f}  {under}")
    timed = [r for r in S.LOG if not r[0].endswith("(profiled)")]
    print(f"   {len(S.LOG)} delayed runs; the longest host enqueue of a no-wait case took {max([r[1] for r in timed if r[3]] or [0.0]):.2f} ms; "
          f"the file took {time.time() - T0:.1f} s")
    _sight()
    missing = (set(P.SCRATCH_FAMILIES) | set(P.NO_SCRATCH_FAMILIES)) - FAMILIES
    assert not missing, f"families never launched behind a delay: {sorted(missing)}"
    routes = {r for rs in S.SHARED_FAMILY_ROUTES.values() for r in rs}
    assert routes <= ROUTES, f"routes that share a family name and never ran behind a delay: {sorted(routes - ROUTES)}"
    wrong = {e: c for e, c in S.COVERED.items() if e not in CALLS.get(c, ())}
    assert not wrong, f"entry points the named case did not call behind a delay: {wrong}"
