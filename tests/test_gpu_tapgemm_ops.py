"""The tap-GEMM (tapgemm.hip) on fp32 activations -- its exact-fp32 path (v_mfma_f32_32x32x2_f32, lane-half K split), its bf16x3 path
(two LDS planes, the w_lo weight plane, three MFMAs per product) and its bf16 path that converts fp32 inputs while staging
(SI_VOC_OPREADY=0) -- launch by launch against a float64 reference of the same operation (vocoder_ref.tapgemm_ref, encoder_ref.linear_ref) on the
operands the kernel itself read, captured through the taps of the fp32 residual stream ("pre", "ups<i>", "stage<i>.rb<j>.t<n>",
"stage<i>.rb<j>.p<n>", include/si_hip.h) and the encoder's fp32 per-op taps.

Vocoder side: the one-stage architectures of test_gpu_vocoder_ops.py put one stage of C = 32 / 64 / 128 / 256 channels (si_pick_bn: 32-, 64- and
128-column tiles) at exactly Tm rows; Tm = 127, 128, 129 (the M > 128 switch from the 128-row to the 256-row tile of launch_math's narrow
branch), 255, 256, 257 (the M > 256 switch to 256x128w8) and 513 (three tiles).  `_config` restates launch_math for fp32 inputs; every
run asserts that the profile holds exactly the configurations `_config` names for its launches, and the coverage test that the cases
together reach all six tile shapes in each of the three arithmetics.  Every assertion is |got - ref| <= E over ALL rows and channels of
clip 0, E derived in the references' docstrings; clip 1 (the same clip, other workgroups) must equal clip 0 bit for bit.  The line printed
per check gives max err / E over the rows within the taps' reach of a tile seam or clip edge and over the rest.

Encoder side: InpaintingEngine(..., "fp32", ...) with one layer, base and large widths, M = B T = 127, 129, 255, 256, 257 rows: every Linear
(the feature projection behind its LayerNorm, QKV, out-proj, FFN1 + GELU, FFN2: ntaps = 1 keeps them on 128 x 128 tiles) and strided conv
against linear_ref(round_w=False, fp32_products=True); the grouped positional conv (16 groups, 128 taps, 48 / 64 channels per group: BK = 16 for
48; N = 48 in Npad = 64) from "projected" to "encoder_in"; the head's LayerNorm + Linear(-> 80), two 64-column tiles of a weight padded to
Npad = 128 whose second tile masks 48 columns, from "last_hidden" to what encode returns; uniform and ragged with a single-frame clip.

(conv_pre's packed K is the input width rounded up to 32 -- 96 channels for 80 mels, BK = 32 -- so in this file BK = 16 is reached by the base
positional conv only; tests/test_gpu_unitvoc_ops.py runs a 16-channel stage, an ungrouped conv at BK = 16, through the same helpers.)

What the bounds can see.  They are worst-case bounds of K fp32 additions, linear in K, while the error of a correct kernel grows like
sqrt(K): measured on MI355X (RECORD; max err / E over rows within the taps' reach of a tile seam or clip edge | the rest) the kernels sit
at 0.002 - 0.035 of E for K = 96 ... 2816, and below 5e-4 for the positional conv (K = 6144 / 8192, where E is 1 - 6 % of the output).  A wrong
row, tap, dilation, slope order, alpha, a dropped bf16x3 cross term or a masked column written lands outside E (tests/test_vocoder_ref.py,
tests/test_encoder_ref.py emulate each on the CPU, the positional conv's dropped halo row at the real widths); a mistake of a few ulp does not.
"""
import dataclasses
import os

import pytest
import torch

from tests import encoder_ref as E
from tests import vocoder_ref as V
from tests.test_gpu_vocoder_ops import _arch, _mel, _state

pytestmark = pytest.mark.gpu

torch.set_num_threads(16)
MODES = {"fp32": ("fp32", "f32", {}), "bf16x3": ("bf16x3", "bf16x3", {}), "bf16": ("bf16", "bf16", {"SI_VOC_OPREADY": "0"})}
TILES = ("128x32", "256x32", "128x64", "256x64", "128x128", "256x128w8")
ROWS = (127, 128, 129, 255, 256, 257, 513)
SUMMARY = {}                                          # kernel configuration -> [max err / E near seams and edges, elsewhere, checks]
# max err / E per configuration as measured on MI355X by test_zz_summary_of_ratios (records, not limits): (seam + edge rows, the rest).
# The encoder's Linear layers and strided convs are in the 128x128 / 128x64 fp32 lines (last tile | the rest); "groups": the positional conv.
RECORD = {
    "tapgemm_f32_128x32": (0.020, 0.028), "tapgemm_f32_256x32": (0.026, 0.035), "tapgemm_f32_128x64": (0.011, 0.015),
    "tapgemm_f32_256x64": (0.015, 0.015), "tapgemm_f32_128x128": (0.012, 0.017), "tapgemm_f32_256x128w8": (0.006, 0.010),
    "tapgemm_f32_128x64 groups BK=16": (0.0005, 0.0005), "tapgemm_f32_256x64 groups BK=16": (0.0005, 0.0005),       # (an upper limit: the run printed 0.000)
    "tapgemm_f32_128x64 groups BK=32": (0.0005, 0.0005), "tapgemm_f32_256x64 groups BK=32": (0.0005, 0.0005),
    "tapgemm_bf16x3_128x32": (0.004, 0.005), "tapgemm_bf16x3_256x32": (0.005, 0.007), "tapgemm_bf16x3_128x64": (0.003, 0.003),
    "tapgemm_bf16x3_256x64": (0.004, 0.005), "tapgemm_bf16x3_128x128": (0.003, 0.003), "tapgemm_bf16x3_256x128w8": (0.002, 0.002),
    "tapgemm_bf16_128x32": (0.009, 0.010), "tapgemm_bf16_256x32": (0.014, 0.015), "tapgemm_bf16_128x64": (0.005, 0.006),
    "tapgemm_bf16_256x64": (0.014, 0.008), "tapgemm_bf16_128x128": (0.005, 0.007), "tapgemm_bf16_256x128w8": (0.003, 0.004),
}


def _config(math, N, M, ntaps, dil, Cin, stride=1):
    """launch_math (tapgemm.hip) for fp32 inputs (x16 == nullptr) -> (profile name, BM).  MaxA<256, 512> = 6 and MaxA<256> = 12 float4 per
    thread: both caps are 3072 float4, i.e. 384 rows of 32 channels.  N = 16 (a 32-column tile, Npad = 32) and Cin = 16 (BK = 16: a quarter of
    the float4 per row, so the 256-row tile's halo always fits) need no case of their own: tests/test_gpu_unitvoc_ops.py asserts these names there."""
    bk = 32 if Cin % 32 == 0 else 16
    bn = 128 if N >= 128 else 64 if N > 32 else 32
    rows256 = 255 * stride + (ntaps - 1) * abs(dil) + 1
    cap = (3 if ntaps == 1 else 6) * 512
    if bn == 128:
        tall = bk == 32 and M > 256 and rows256 * (bk // 4) <= cap
        return (f"tapgemm_{math}_256x128w8", 256) if tall else (f"tapgemm_{math}_128x128", 128)
    tall = rows256 * (bk // 4) <= cap and M > 128
    return (f"tapgemm_{math}_256x{bn}", 256) if tall else (f"tapgemm_{math}_128x{bn}", 128)


def _mel_ld(num_mels):
    return -(-num_mels // 32) * 32


_ENGINES = {}
_FOLDED = {}


def _engine(varch, mode, opready=False):
    """An engine per (architecture, arithmetic), kept for the file: the knobs are read when the context is created."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch
    from speech_inpainting_amd.engine import InpaintingEngine
    key = (repr(varch), mode, opready)
    if key not in _ENGINES:
        voc, _, env = MODES[mode]
        env = {} if opready else env
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            eng = InpaintingEngine(HubertArch.tiny(), varch, 20, "cuda:0", "fp32", voc)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        _ENGINES[key] = eng.load_state(synth.synth_hubert_state(HubertArch.tiny()), _state(varch), synth.synth_codebook(20))
    return _ENGINES[key]


def _w(varch, name):
    """The packer's fp32 folded weight of a module (vocoder_ref.fold, unrounded)."""
    key = (repr(varch), name)
    if key not in _FOLDED:
        _FOLDED[key] = V.fold(_state(varch), name, round16=False).float()
    return _FOLDED[key]


def _shapes(varch, B, Tm, t_suffix=""):
    """{tap name: (B, rows, channels)} of every tap of the fp32 residual stream at Tm frames (stretch off)."""
    C, L = varch.upsample_initial_channel, Tm
    out = {"pre": (B, L, C)}
    for i, u in enumerate(varch.upsample_rates):
        C, L = C // 2, L * u
        out[f"ups{i}"] = out[f"stage{i}"] = (B, L, C)
        for j, dil in enumerate(varch.resblock_dilation_sizes):
            for n in range(len(dil)):
                out[f"stage{i}.rb{j}.p{n}"] = (B, L, C)
                out[f"stage{i}.rb{j}.t{n}{t_suffix}"] = (B, L, C)
    return out


def _run(eng, varch, mel, lens=None, tapped=True, t_suffix=""):
    """One generator pass -> (taps {name: (B, rows, C) cpu}, wave cpu, {kernel: launches})."""
    B, _, Tm = mel.shape
    shapes = _shapes(varch, B, Tm, t_suffix)
    eng.ctx.clear_captures()
    caps = eng.ctx.capture(list(shapes), capacity={k: s[0] * s[1] * s[2] for k, s in shapes.items()}) if tapped else {}
    eng.ctx.profile_start(4000)
    wave = eng.vocode_ragged(mel.cuda(), lens, stretch=False) if lens is not None else eng.vocode(mel.cuda(), stretch=False)
    prof = {e["name"]: e["launches"] for e in eng.ctx.profile_stop()}
    torch.cuda.synchronize()
    taps = {}
    for k, t in caps.items():
        assert eng.ctx.lib.si_debug_size(eng.ctx._h, k.encode()) == t.numel(), (k, "was not produced")
        taps[k] = t.cpu().view(shapes[k])
    eng.ctx.clear_captures()
    return taps, wave.cpu(), prof


def _note(kernel, near, rest):
    s = SUMMARY.setdefault(kernel, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], near), max(s[1], rest), s[2] + 1


def _one(tag, kernel, clip, got, r, stored, halo):
    L = r.ref.shape[0]
    c = V.check_f32(got.reshape(r.ref.shape), r.ref, r.E)
    line, near, rest = V.report(tag, kernel, clip, c, L, stored, halo)
    print("   " + line)
    assert c["finite"] and c["bad"] == 0, line
    if r.exact is not None and r.exact is not r.ref:           # bf16x3: also within the derived distance of the exact fp32 product
        cx = V.check_f32(got.reshape(r.ref.shape), r.exact, r.E_exact)
        linex, _, _ = V.report(tag + " vs the fp32 product", kernel, clip, cx, L, stored, halo)
        assert cx["bad"] == 0, linex
    _note(kernel, near, rest)


def _verify(varch, mode, mel, lens, taps, prof, tag, clips=None, wave=None):
    """Every tap of every clip against its reference from the tapped input; -> the configurations the launches must have taken.
    wave: the samples, to check conv_post_kernel (fp32 rows, the slope in fp32) against conv_post_ref(mfma=False) on the last stage's tap."""
    math = MODES[mode][1]
    sd = _state(varch)
    B, _, Tm = mel.shape
    nk = len(varch.resblock_kernel_sizes)
    a_last = V.alpha32(nk)
    want = set()
    Lmax = Tm
    for b in (range(B) if clips is None else clips):
        L = int(lens[b]) if lens is not None else Tm
        C0 = varch.upsample_initial_channel
        nm = varch.num_mels
        kern, bm = _config(math, C0, Lmax, 7, 1, _mel_ld(nm))              # (conv_pre's packed K: the input width rounded up to 32, api.hip's mel_ld)
        want.add(kern)
        r = V.tapgemm_ref(mel[b, :, :L].t(), _w(varch, "conv_pre"), sd["conv_pre.bias"], math, V.conv_geom(1), 7 * nm)
        x = taps["pre"][b, :L]
        _one(f"{tag} conv_pre {nm}->{C0}", kern, b, x, r, bm, 6)
        C, Lm = C0, Lmax
        for i, (u, k) in enumerate(zip(varch.upsample_rates, varch.upsample_kernel_sizes)):
            w = _w(varch, f"ups.{i}")
            ntaps, pad = -(-k // u), (k - u) // 2
            Lo, Lmo, Cin, C = L * u, Lm * u, C, C // 2
            kern, bm = _config(math, u * C, (pad + Lmo - 1) // u + 1, ntaps, -1, Cin)
            want.add(kern)
            r = V.tapgemm_ref(x, w, sd[f"ups.{i}.bias"], math, V.tconv_geom(u), ntaps * Cin, slope=V.SLOPE32)
            U = taps[f"ups{i}"][b, :Lo]
            _one(f"{tag} ups{i} {Cin}->{C} u={u} k={k}", kern, b, U, r, bm * u, k)
            L, Lm = Lo, Lmo
            kern, bm = _config(math, C, Lm, 3, 1, C)               # (k and the dilation never change the tile here: 255 + 10 * 5 + 1 <= 384 rows)
            want.add(kern)
            xs_prev = None
            for j, (rk, dils) in enumerate(zip(varch.resblock_kernel_sizes, varch.resblock_dilation_sizes)):
                assert _config(math, C, Lm, rk, max(dils), C)[0] == kern
                p = f"resblocks.{i * nk + j}."
                xin = U
                for n, d in enumerate(dils):
                    last = n == len(dils) - 1
                    t = taps[f"stage{i}.rb{j}.t{n}"][b, :L]
                    r = V.tapgemm_ref(xin, _w(varch, f"{p}convs1.{n}"), sd[f"{p}convs1.{n}.bias"], math, V.conv_geom(d), rk * C, slope=V.SLOPE32)
                    _one(f"{tag} stage{i}.rb{j}.t{n} k={rk} d={d}", kern, b, t, r, bm, (rk - 1) * d)
                    prev = xs_prev if (last and j > 0) else None
                    r = V.tapgemm_ref(t, _w(varch, f"{p}convs2.{n}"), sd[f"{p}convs2.{n}.bias"], math, V.conv_geom(1), rk * C, slope=V.SLOPE32,
                                      res=xin, alpha=a_last if last else 1.0, prev=prev)
                    out = taps[f"stage{i}.rb{j}.p{n}"][b, :L]
                    _one(f"{tag} stage{i}.rb{j}.p{n} k={rk}" + (" alpha" if last else "") + (" acc" if prev is not None else ""), kern, b, out, r, bm, rk - 1)
                    xin = out
                xs_prev = xin
            assert torch.equal(taps[f"stage{i}"][b, :L], xs_prev), f"{tag} stage{i} is not the last resblock's running sum"
            x = xs_prev
        if wave is not None:
            ref, Eb = V.conv_post_ref(x, _w(varch, "conv_post"), sd["conv_post.bias"], mfma=False)
            c = V.check_f32(wave[b, :L], ref, Eb)
            line, near, rest = V.report(f"{tag} conv_post C={C}", "conv_post", b, c, L, 256, 3)
            print("   " + line)
            assert "conv_post" in prof and c["finite"] and c["bad"] == 0, line
            assert not bool(wave[b, L:].any()), f"{tag}: samples past clip {b}'s end are not silence"
            _note(f"conv_post_kernel C={C}", near, rest)
    got = {n for n in prof if n.startswith("tapgemm_")}
    assert got == want, f"{tag}: the launches took {sorted(got)}, launch_math restated gives {sorted(want)}"
    return want


def _uniform(varch, mode, L, seed, tag, post=False):
    one = _mel(1, L, seed, varch.num_mels)
    mel = torch.cat([one, one]).contiguous()
    taps, wave, prof = _run(_engine(varch, mode), varch, mel)
    cfgs = _verify(varch, mode, mel, None, taps, prof, f"{tag} L={L}", clips=[0], wave=wave if post else None)
    for k, t in taps.items():
        assert torch.equal(t[0], t[1]), f"{tag} L={L}: {k} differs between two copies of one clip"
    assert torch.equal(wave[0], wave[1])
    return cfgs, taps, wave


def _reached(mode, C, L, num_mels=80):
    """The configurations of one (C, L) case, from `_config` alone (no GPU): conv_pre, the u = 1, k = 3 upsampler(s), the pairs."""
    math = MODES[mode][1]
    out = {_config(math, 2 * C, L, 7, 1, _mel_ld(num_mels))[0], _config(math, C, L + 1, 3, -1, 2 * C)[0], _config(math, C, L, 3, 1, C)[0]}
    if C == 256:
        out |= {_config(math, 128, L + 1, 3, -1, 256)[0], _config(math, 128, L, 3, 1, 128)[0]}
    return out


@pytest.mark.parametrize("L", ROWS)
@pytest.mark.parametrize("C", [32, 64, 128, 256])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_tapgemm_launch_of_a_stage_at_the_tile_seams(mode, C, L):
    """conv_pre, the upsampler (a transposed conv: dil = -1, M = L + 1 GEMM rows, ooff < 0) and the nine pairs (k = 3, 7, 11 x dilation 1, 3, 5;
    residual, alpha = 1 / 3, accumulate) of one stage of C channels at L rows, two copies of one clip."""
    varch = _arch(C)
    cfgs, _, _ = _uniform(varch, mode, L, 1000 + C + L, f"{mode} C={C}")
    assert cfgs == _reached(mode, C, L), (sorted(cfgs), sorted(_reached(mode, C, L)))


def test_coverage_of_every_reachable_configuration():
    """The cases above, through launch_math as `_config` restates it (each case asserts that its launches took exactly those names): all six
    tile shapes in each arithmetic.  The 8-wave 128x128 and 256x64 tiles and the 64-deep K chunk take operand-ready inputs only."""
    ran = set()
    for mode in MODES:
        for C in (32, 64, 128, 256):
            for L in ROWS:
                ran |= _reached(mode, C, L)
    want = {f"tapgemm_{MODES[m][1]}_{t}" for m in MODES for t in TILES}
    print(sorted(ran))
    assert want == ran, (sorted(want - ran), sorted(ran - want))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("u,k,C", [(2, 4, 64), (8, 16, 32)])
def test_upsampler_phases(mode, u, k, C):
    """The transposed conv with u = 2, k = 4 and u = 8, k = 16 (two taps, N = u Cout phases, ooff = -(k - u) / 2 Cout): Lin = 127, 128, 129 put
    the M = Lin + 1 GEMM rows at the tall switch; the stage behind it runs at u Lin rows."""
    varch = _arch(C, u=u, k=k, resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1, 3, 5),))
    for L in (127, 128, 129):
        _uniform(varch, mode, L, 2000 + u + L, f"{mode} u={u}")


@pytest.mark.parametrize("mode", list(MODES))
def test_ragged_batch_equals_each_clip_alone(mode):
    """vocode_ragged: lengths on both sides of the 128- and 256-row switches and one single row; every tap of every clip against its
    reference, and every clip's taps and samples equal to the same clip run alone, bit for bit."""
    varch = _arch(64)
    lens = [257, 1, 129, 128, 256]
    mel = _mel(len(lens), max(lens), 3000)
    eng = _engine(varch, mode)
    taps, wave, prof = _run(eng, varch, mel, lens)
    _verify(varch, mode, mel, lens, taps, prof, f"{mode} ragged")
    for b, L in enumerate(lens):
        one = mel[b:b + 1, :, :L].contiguous()
        t1, w1, _ = _run(eng, varch, one)
        for k in t1:
            assert torch.equal(t1[k][0], taps[k][b, :t1[k].shape[1]]), f"{mode} ragged clip {b} (L = {L}): {k} differs from the clip alone"
        assert torch.equal(w1[0], wave[b, :w1.shape[1]]) and not bool(wave[b, w1.shape[1]:].any())


@pytest.mark.parametrize("C", [32, 64, 128])
def test_operand_ready_bf16_is_bit_identical_at_the_seams(C):
    """api.hip: the operand-ready bf16 form (the default; 16-bit copies written by the producers, the 8-wave tiles) computes what the
    fp32-input form (SI_VOC_OPREADY=0) computes.  Every fp32 tap and the waveform, at the rows around both switches."""
    varch = _arch(C)
    for L in (127, 129, 256, 257):
        one = _mel(1, L, 4000 + L)
        mel = torch.cat([one, one]).contiguous()
        taps, wave, _ = _run(_engine(varch, "bf16"), varch, mel)
        t_op, w_op, prof = _run(_engine(varch, "bf16", opready=True), varch, mel, t_suffix=".bf16")
        if C == 64 and L > 128:
            assert "tapgemm_bf16_256x64w8" in prof, sorted(prof)
        for k in taps:
            if ".t" in k:                                      # the intermediate exists only as bf16(leaky_relu(t, 0.1)) there
                want = V.lrelu32(taps[k], V.SLOPE32).to(torch.bfloat16)
                assert torch.equal(t_op[k + ".bf16"], want), f"C={C} L={L}: {k}.bf16 is not the staged operand of the fp32-input form"
            else:
                assert torch.equal(t_op[k], taps[k]), f"C={C} L={L}: {k} differs between the operand-ready and the fp32-input form"
        assert torch.equal(w_op, wave)


def test_full_v1_in_bf16x3_and_taps_are_inert():
    """The V1 generator (512 channels down to 32, u = 8, 8, 2, 2), every tap of every stage once in bf16x3; and in each of the three modes the
    waveform, the kernel names and the launch counts with every tap registered are those of a run without."""
    from speech_inpainting_amd.arch import VocoderArch
    varch = VocoderArch.v1()
    mel = _mel(2, 9, 5000)
    for mode in MODES:
        eng = _engine(varch, mode)
        _, plain, prof0 = _run(eng, varch, mel, tapped=False)
        taps, wave, prof = _run(eng, varch, mel)
        assert torch.equal(wave, plain), f"{mode}: registering the taps changed the waveform"
        assert prof == prof0, (prof, prof0)
        if mode == "bf16x3":
            _verify(varch, mode, mel, None, taps, prof, "V1 bf16x3")          # (its launches, too, must take the tiles `_config` names)


# ------------------------------------------------------------------------------------------------------------ encoder side
def _harch(name):
    from speech_inpainting_amd.arch import HubertArch
    return HubertArch(num_hidden_layers=1) if name == "base" else dataclasses.replace(HubertArch.large(), num_hidden_layers=1)


def _enc_state(harch):
    from tests.test_gpu_encoder_ops import _state as enc_state
    return enc_state(harch)


def _enc_engine(name):
    """fp32 encoder, one layer, real widths."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import VocoderArch
    from speech_inpainting_amd.engine import InpaintingEngine
    if ("enc", name) not in _ENGINES:
        harch = _harch(name)
        eng = InpaintingEngine(harch, VocoderArch.tiny(), 50, "cuda:0", "fp32", "fp32")
        _ENGINES[("enc", name)] = eng.load_state(_enc_state(harch), synth.synth_generator_state(VocoderArch.tiny()), synth.synth_codebook(50))
    return _ENGINES[("enc", name)]


def _enc_run(eng, harch, wave, lens=None):
    """One fp32 encoder forward with every tap registered -> (taps, transformer rows, {kernel: launches}, what encode returned)."""
    B, N = wave.shape
    R = sum(harch.num_frames(n) for n in lens) if lens is not None else B * harch.num_frames(N)
    cap = {k: v for k, v in E.tap_capacities(harch, B, N, R).items() if not k.endswith(".bf16")}
    for nm in ("projected", "encoder_in", "last_hidden"):
        cap[nm] = R * harch.hidden_size
    cap["features"] = R * harch.conv_dim[-1]
    eng.ctx.clear_captures()
    caps = eng.ctx.capture(list(cap), capacity=cap)
    eng.ctx.profile_start(4000)
    out = eng.encode_ragged(wave, lens, normalize=False) if lens is not None else eng.encode(wave, normalize=False)
    prof = {e["name"]: e["launches"] for e in eng.ctx.profile_stop()}
    torch.cuda.synchronize()
    produced = {k: eng.ctx.lib.si_debug_size(eng.ctx._h, k.encode()) for k in cap}
    got = {k: v.cpu() for k, v in caps.items() if produced[k] > 0 and produced[k] == cap[k]}
    eng.ctx.clear_captures()
    return got, R, prof, out.cpu()


def _enc_one(tag, kernel, got, ref, bound, stored=128):
    r = E.check_f32(got.reshape(ref.shape), ref, bound)
    M = ref.shape[0]
    ratio = ((got.reshape(ref.shape).double() - ref).abs() / bound.clamp_min(1e-300)).reshape(M, -1).amax(1)
    last0 = (M - 1) // stored * stored                       # rows of the last (partial) tile | the rest
    near = float(ratio[last0:].max())
    rest = float(ratio[:last0].max()) if last0 else 0.0
    print(f"   {E.fmt(tag, r)} [{kernel}] last tile {near:.3f}, rest {rest:.3f}")
    assert r["bad"] == 0, E.fmt(tag, r)
    _note(kernel, near, rest)


def _check_layer32(got, harch, R, tag):
    """The four Linear layers of layer 0 on the exact-fp32 tap-GEMM, each on its captured fp32 operand."""
    sd = _enc_state(harch)
    H, I = harch.hidden_size, harch.intermediate_size
    p = "base_model.encoder.layers.0."
    pre = harch.do_stable_layer_norm
    kw = dict(round_w=False, fp32_products=True)
    kern = _config("f32", H, R, 1, 1, H)[0]
    assert kern == "tapgemm_f32_128x128"                      # (a Linear's two half-sets of prefetch registers rule the 256-row tiles out)
    hin = got["layer0.h"].view(R, H)
    a_qkv = got["layer0.ln1"].view(R, H) if pre else hin
    wqkv = torch.cat([sd[p + f"attention.{n}_proj.weight"] for n in "qkv"])
    bqkv = torch.cat([sd[p + f"attention.{n}_proj.bias"] for n in "qkv"])
    _enc_one(f"{tag} QKV", kern, got["layer0.qkv"].view(R, 3 * H), *E.linear_ref(a_qkv, wqkv, bqkv, **kw))
    _enc_one(f"{tag} out-proj + residual", kern, got["layer0.att_res"].view(R, H),
             *E.linear_ref(got["layer0.att"].view(R, H), sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"], res=hin, **kw))
    a_ffn = got["layer0.ln2" if pre else "layer0.ln1"].view(R, H)
    res2 = got["layer0.att_res" if pre else "layer0.ln1"].view(R, H)
    ffn = got["layer0.ffn"].view(R, I)
    _enc_one(f"{tag} FFN1 + GELU", kern, ffn, *E.linear_ref(a_ffn, sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"], act="gelu", **kw))
    _enc_one(f"{tag} FFN2 + residual", kern, got["layer0.ffn_res"].view(R, H),
             *E.linear_ref(ffn, sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"], res=res2, **kw))
    return {kern}


def _check_convs32(got, harch, B, N, tag, clip_lens=None):
    """Strided convs 1 .. n - 1 (stride 2: the 256-row tile's halo does not fit, 128 x 128 tiles) of every clip on their captured fp32 inputs."""
    from tests.test_gpu_encoder_ops import _sel_rows
    sd = _enc_state(harch)
    Ls = harch.feat_lengths(N)
    layer = harch.feat_extract_norm == "layer"
    pre = "base_model.feature_extractor.conv_layers."
    want = set()
    for i in range(1, len(harch.conv_dim)):
        Cin, C, k, s = harch.conv_dim[i - 1], harch.conv_dim[i], harch.conv_kernel[i], harch.conv_stride[i]
        kern = _config("f32", C, Ls[i + 1], k, 1, Cin, stride=s)[0]
        want.add(kern)
        xin = got[f"conv{i - 1}.ln" if layer else f"conv{i - 1}"].view(B, Ls[i], Cin)
        y = got[f"conv{i}"].view(B, Ls[i + 1], C)
        w = E.conv_weight(sd[pre + f"{i}.conv.weight"])
        bias = sd[pre + f"{i}.conv.bias"] if harch.conv_bias else None
        for b in range(B):
            Lb = harch.feat_lengths(clip_lens[b])[i + 1] if clip_lens is not None else Ls[i + 1]
            rows = _sel_rows(Lb, seed=b)
            ref, bound = E.linear_ref(E.conv_rows(xin[b].double(), k, s, rows), w, bias, act=None if layer else "gelu", round_w=False, fp32_products=True)
            r = E.check_f32(y[b][rows], ref, bound)
            print("   " + E.fmt(f"{tag} conv{i} clip {b} (L = {Lb}, last tile {Lb % 128} rows) [{kern}]", r))
            assert r["bad"] == 0, E.fmt(f"{tag} conv{i} clip {b}", r)
            _note(kern, r["worst"], 0.0)
    return want


def _check_posconv32(got, harch, clips, Tmax, tag):
    """h2 = h + gelu(pos_conv(h) + b) on the tap-GEMM (16 groups, 128 taps, pad 64, the even kernel's last output row dropped) from
    "projected" to "encoder_in": directly in the pre-LN flavour; through the encoder's LayerNorm, whose passage of the conv's bound
    encoder_ref.layernorm_of_bounded derives, in the post-LN one.  clips: [(first packed row, T)]."""
    sd = _enc_state(harch)
    H, G, k = harch.hidden_size, harch.num_conv_pos_embedding_groups, harch.num_conv_pos_embeddings
    cg = H // G
    w = E.pos_conv_weight(sd)
    bias = sd["base_model.encoder.pos_conv_embed.conv.bias"]
    kern, bm = _config("f32", cg, Tmax, k, 1, cg)
    R = got["projected"].numel() // H
    proj, enc_in = got["projected"].view(R, H), got["encoder_in"].view(R, H)

    contract = E.pos_conv_geom(k, G)
    for r0, T in clips:
        h = proj[r0:r0 + T]
        r = V.tapgemm_ref(h, w, bias, "f32", contract, k * cg, act="gelu", res=h)
        ref, bound = r.ref, r.E
        if not harch.do_stable_layer_norm:
            ref, bound = E.layernorm_of_bounded(ref, bound, sd["base_model.encoder.layer_norm.weight"], sd["base_model.encoder.layer_norm.bias"], harch.layer_norm_eps)
        c = V.check_f32(enc_in[r0:r0 + T], ref, bound)
        line, near, rest = V.report(f"{tag} positional conv ({G} groups of {cg}, BK = {32 if cg % 32 == 0 else 16}) T={T}", kern, r0, c, T, bm, k // 2)
        print("   " + line)
        assert c["finite"] and c["bad"] == 0, line
        _note(kern + f" groups BK={32 if cg % 32 == 0 else 16}", near, rest)
    return {kern}


def _check_projection32(got, harch, R, tag):
    """feature_projection: [LayerNorm +] Linear(512 -> H) from "features" to "projected"."""
    sd = _enc_state(harch)
    p = "base_model.feature_projection."
    CF, H = harch.conv_dim[-1], harch.hidden_size
    ln = harch.feat_proj_layer_norm
    kern = _config("f32", H, R, 1, 1, CF)[0]
    ref, bound = E.ln_linear_ref(got["features"].view(R, CF), sd[p + "layer_norm.weight"] if ln else None, sd[p + "layer_norm.bias"] if ln else None,
                            harch.layer_norm_eps, sd[p + "projection.weight"], sd[p + "projection.bias"])
    _enc_one(f"{tag} feature projection", kern, got["projected"].view(R, H), ref, bound)
    return {kern}


def _check_head32(got, harch, feats, clips, tag):
    """final_layers: LayerNorm(eps 1e-5) + Linear(H -> 80) in fp32, from "last_hidden" to what encode returns.  N = 80 runs on two 64-column
    tiles of a weight padded to Npad = 128 rows: the second tile's last 48 columns are masked.  clips: [(first packed row, T, clip index in feats)]."""
    sd = _enc_state(harch)
    H = harch.hidden_size
    R = got["last_hidden"].numel() // H
    kern = _config("f32", 80, R, 1, 1, H)[0]
    assert kern == "tapgemm_f32_128x64"
    ref, bound = E.ln_linear_ref(got["last_hidden"].view(R, H), sd["final_layers.0.weight"], sd["final_layers.0.bias"], 1e-5,
                            sd["final_layers.1.weight"], sd["final_layers.1.bias"])
    assert feats.shape[-1] == 80
    for r0, T, b_ in clips:
        _enc_one(f"{tag} head clip {b_} T={T}", kern, feats[b_, :T], ref[r0:r0 + T], bound[r0:r0 + T])
        assert not bool(feats[b_, T:].any()), f"{tag}: frames past clip {b_}'s own are not zero"
    return {kern}


ENC_CASES = [(1, 127), (2, 128), (1, 129), (1, 255), (1, 257)]


@pytest.mark.parametrize("B,T", ENC_CASES)
@pytest.mark.parametrize("arch", ["base", "large"])
def test_fp32_encoder_tapgemm_launches(arch, B, T):
    """M = B T = 127, 256, 129, 255, 257 transformer rows (last tiles of 127, 128, 1, 127 and 1 rows; T = 127 / 128 | 129 on both sides of the
    positional conv's 256-row switch); the sample count puts strided convs at last tiles of 1 and 127 rows where it can."""
    from tests.test_gpu_encoder_ops import _pick_wave
    harch = _harch(arch)
    eng = _enc_engine(arch)
    wave = _pick_wave(harch, B, T, 128)
    got, R, prof, feats = _enc_run(eng, harch, wave)
    assert R == B * T
    want = _check_layer32(got, harch, R, f"{arch} M={R}")
    want |= _check_convs32(got, harch, B, wave.shape[1], f"{arch} M={R}")
    want |= _check_projection32(got, harch, R, f"{arch} M={R}")
    want |= _check_posconv32(got, harch, [(b * T, T) for b in range(B)], T, f"{arch} M={R}")
    want |= _check_head32(got, harch, feats, [(b * T, T, b) for b in range(B)], f"{arch} M={R}")
    names = {n for n in prof if n.startswith("tapgemm_")}
    assert names == want, (sorted(names), sorted(want))


def test_fp32_encoder_coverage():
    """From `_config` alone: the encoder cases reach the Linear instantiations (128 x 128, and 128 x 64 with masked columns), the strided
    128 x 128 conv, and the grouped positional conv on both heights at BK = 16 (48 channels per group) and BK = 32 (64)."""
    for cg in (48, 64):
        hs = {_config("f32", cg, T, 128, 1, cg)[0] for _, T in ENC_CASES}
        assert hs == {"tapgemm_f32_128x64", "tapgemm_f32_256x64"}, hs
    assert _config("f32", 512, 400, 3, 1, 512, stride=2)[0] == "tapgemm_f32_128x128"


@pytest.mark.parametrize("arch", ["base", "large"])
def test_fp32_encoder_ragged_with_a_single_frame_clip(arch):
    """encode_ragged: packed transformer rows, per-clip conv segments, the positional conv's zero padding at each clip's own ends; one clip
    is a single frame.  Every op as above, per clip."""
    from speech_inpainting_amd import synth
    harch = _harch(arch)
    eng = _enc_engine(arch)
    frames = [130, 1, 97]
    lens = [320 * (T - 1) + 400 + d for T, d in zip(frames, (17, 5, 300))]
    wave = synth.synth_wave(len(lens), max(lens), 29).cuda()
    got, R, prof, feats = _enc_run(eng, harch, wave, lens=lens)
    assert R == sum(frames)
    offs = [sum(frames[:b]) for b in range(len(frames))]
    _check_layer32(got, harch, R, f"ragged {arch}")
    _check_convs32(got, harch, len(lens), max(lens), f"ragged {arch}", clip_lens=lens)
    _check_projection32(got, harch, R, f"ragged {arch}")
    _check_posconv32(got, harch, list(zip(offs, frames)), max(frames), f"ragged {arch}")
    _check_head32(got, harch, feats, [(o, T, b) for b, (o, T) in enumerate(zip(offs, frames))], f"ragged {arch}")


def test_zz_summary_of_ratios():
    """(last in the file) the largest err / E per kernel configuration over every check above: near seams and clip edges | elsewhere."""
    for k in sorted(SUMMARY):
        s = SUMMARY[k]
        print(f"   SUMMARY {k}: max err/E seam+edge rows {s[0]:.4f}, interior {s[1]:.4f} over {s[2]} checks")
        assert s[0] <= 1.0 and s[1] <= 1.0
