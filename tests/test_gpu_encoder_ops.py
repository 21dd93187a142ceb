"""Each kernel of the bf16 encoder against a float64 reference of its own operation (tests/encoder_ref.py), on the operands
the kernel itself read, captured through the encoder's per-op taps: the GEMMs (gemmcu.hip's six instantiations, lingemm.hip's
three tile heights, the tap-GEMM's bf16 path) at M = BM - 1, BM, BM + 1 and on ragged per-clip segments; the attention kernels
at the 32-key tile edges, across the whole-K/V / tiled switch (T = 256 / 257), on padded and ragged batches; LayerNorm at
C = 512, 768, 1024 (its bf16 operand bit-equal to rne of its fp32 rows); conv0 + GroupNorm + GELU.  Real layer widths, one
layer.  Every bound is an error bound derived in encoder_ref.py, not a tolerance fitted to these runs.

The feature projection (`_check_projection`, in every run that checks a layer's GEMMs): its LayerNorm(512), stored as the GEMM's
bf16 operand only ("features.ln.bf16"), and Linear(512 -> H), the encoder's only GEMM with K = 512, on that operand.

The positional conv (`test_posconv_*`): posconv.hip and the SI_ENC_POSCONV=0 fallback (the grouped bf16 tap-GEMM, N = 48 in
Npad = 64), Cg = 48 and 64, at the "pos_conv" tap against vocoder_ref.tapgemm_ref's "bf16" bound on the captured "projected" rows, every
row and channel, at the smallest shapes that reach each seam of posconv.hip's tiling: two clips per workgroup (Tmax <= 256) | 512-row
blocks of two 256-row halves, each staged with a 128-row halo; an odd batch, a half or a block holding one row, clips shorter than
the 64-row padding, the clamped rows outside a clip, padded frames zeroed.  What that bound can see: it is the worst case of
K = 6144 / 8192 fp32 additions, linear in K, while a correct kernel's error grows like sqrt(K) and sits far below it (the records
below).  A wrong row, tap, halo or clip lands outside it (tests/test_encoder_ref.py fails it with four seeded mistakes on a CPU
emulation: a halo off by one at the half seam, a dropped tap, a neighbouring clip in the padding, the even kernel's extra row kept);
a mistake of a few ulp does not.  The bit-identity assertions (each ragged clip equal to the clip alone) see those.

Measured on MI355X (records, not limits): max err / E over the rows within 64 of a 256-row seam or a clip edge | over the rest
    posconv_bf16_c48        below 5e-4 | below 5e-4 (23 clips; the run printed 0.000)
    posconv_bf16_c64        below 5e-4 | below 5e-4 (23 clips)
    tapgemm_bf16_256x64     below 5e-4 | below 5e-4 (46 clips) (the fallback, both widths)
the projection GEMM, max err / E over the rows of the last (partial) row tile | the rest
    gemmcu_bf16_320x256, 256x256, 160x128, 224x128, 128x128, 208x256 (M = BM - 1, BM, BM + 1 each)     0.002 over all rows
    lingemm_bf16_64x128 (M = 3984, 3700, 300 and the ragged base / large batches, M = 432)              0.002
    tapgemm_bf16_128x128w8 (SI_ENC_LINGEMM=0, M = 300) 0.002;  tapgemm_bf16_128x128 (fp32 features, no LayerNorm, M = 257) 0.002
and the share of "features.ln.bf16" outputs != rne(float64 LayerNorm): at most 0.0059 % over 24 runs (the "ln" guard: 0.064 %)."""
import dataclasses

import pytest
import torch

from tests import encoder_ref as E
from tests.cases import _pick_wave, _sel_rows
from tests.cases import _enc_state as _state
from tests.encoder_checks import (GEMMCU_BM, GEMMCU_BN, PC_HALF, _check, _check_attention, _check_convs, _check_layernorms, _check_layers,
                                  _check_projection, _engine, _run)
from tests.encoder_checks import _check_posconv as _check_posconv_arch
from tests.encoder_checks import _pc_both as _pc_both_arch

pytestmark = pytest.mark.gpu


def _base():
    from speech_inpainting_amd.arch import HubertArch
    return HubertArch(num_hidden_layers=1)


def _large():
    from speech_inpainting_amd.arch import HubertArch
    return dataclasses.replace(HubertArch.large(), num_hidden_layers=1)


GEMM_CASES = [(c, d) for c in range(10, 16) for d in (-1, 0, 1)]


@pytest.mark.parametrize("flag,dm", GEMM_CASES)
def test_gemmcu_instantiation_against_float64(flag, dm):
    """SI_ENC_GEMMCU = 10 + c: instantiation c takes every encoder GEMM it covers (all of the base model's: N % 256 == 0); one clip
    of T = BM + dm frames puts the transformer GEMMs at M = BM - 1, BM, BM + 1, the clip length puts strided convs at last tiles
    of 1 / BM - 1 rows where it can.  Every GEMM and conv output of the run against its float64 reference."""
    harch = _base()
    bm = GEMMCU_BM[flag]
    eng = _engine(harch, {"SI_ENC_GEMMCU": str(flag)})
    wave = _pick_wave(harch, 1, bm + dm, bm)
    got, R, names = _run(eng, harch, wave, profile=True)
    assert f"gemmcu_bf16_{bm}x{GEMMCU_BN[flag]}" in names, names
    assert not any(n.startswith("lingemm_bf16_") for n in names), names
    Ls = harch.feat_lengths(wave.shape[1])
    print(f"\nSI_ENC_GEMMCU={flag} ({bm} rows): M = {R} (M mod BM = {R % bm}); conv segments {Ls[2:]} mod BM {[L % bm for L in Ls[2:]]}")
    _check_layers(got, harch, R, f"gemmcu {bm}")
    _check_projection(got, harch, R, f"gemmcu {bm}", names, {"SI_ENC_GEMMCU": str(flag)})
    _check_convs(got, harch, 1, wave.shape[1], f"gemmcu {bm}")


def test_gemmcu_coverage_of_tile_remainders():
    """The runs above, from feat_lengths: every instantiation at M mod BM = 1, BM - 1 and 0."""
    want = {(c, r) for c, bm in GEMMCU_BM.items() for r in (1, bm - 1, 0)}
    # (computed, not recorded: this test must not depend on the others having run first)
    ran = set()
    harch = _base()
    for c, dm in GEMM_CASES:
        bm = GEMMCU_BM[c]
        ran.add((c, harch.num_frames(320 * (bm + dm - 1) + 400) % bm))
    for c, bm in GEMMCU_BM.items():
        print(f"gemmcu {bm} x {GEMMCU_BN[c]}: transformer M mod BM {sorted(r for cc, r in ran if cc == c)}")
    assert want <= ran, want - ran


@pytest.mark.parametrize("B,T,env", [(16, 249, {"SI_ENC_GEMMCU": "0"}), (10, 370, {"SI_ENC_GEMMCU": "0"}), (3, 100, {"SI_ENC_GEMMCU": "0"}),
                                     (2, 150, {"SI_ENC_LINGEMM": "0"})])
def test_lingemm_and_tapgemm_against_float64(B, T, env):
    """SI_ENC_GEMMCU=0: lingemm.hip alone, its rule picking 128-, 96- or 64-row tiles by the tile count (M = 3984 / 3700 reach
    the shorter ones); SI_ENC_LINGEMM=0: the generic tap-GEMM's bf16 path.  Rows checked: the first, the last 336, random ones."""
    harch = _base()
    eng = _engine(harch, env)
    wave = _pick_wave(harch, B, T, 128)
    got, R, names = _run(eng, harch, wave, profile=True)
    lg = sorted(n for n in names if n.startswith("lingemm_bf16_"))
    print(f"\n{env} B={B} T={T} M={R}: {lg}")
    assert not any(n.startswith("gemmcu_bf16") for n in names), names
    assert bool(lg) != ("SI_ENC_LINGEMM" in env), names
    _check_layers(got, harch, R, "lingemm" if lg else "tapgemm", rows=_sel_rows(R))
    _check_projection(got, harch, R, "lingemm" if lg else "tapgemm", names, env, rows=_sel_rows(R))
    _check_convs(got, harch, B, wave.shape[1], "lingemm" if lg else "tapgemm")


def test_lingemm_reaches_every_tile_height():
    """The shapes of the test above, through the launcher's rule: together they run all three lingemm instantiations."""
    harch = _base()
    heights = set()
    for B, T in ((16, 249), (10, 370), (3, 100)):
        wave = _pick_wave(harch, B, T, 128)
        _, _, names = _run(_engine(harch, {"SI_ENC_GEMMCU": "0"}), harch, wave, profile=True)
        heights |= {n for n in names if n.startswith("lingemm_bf16_")}
    print(heights)
    assert {"lingemm_bf16_64x128", "lingemm_bf16_96x128", "lingemm_bf16_128x128"} <= heights, heights


@pytest.mark.parametrize("arch", ["base", "large"])
def test_ragged_batch_gemms_against_float64(arch):
    """encode_ragged: the strided convs run as per-clip segments of each clip's own length (seg_m tiles), the transformer on packed
    rows; every conv row checked per clip, the layer GEMMs on the packed rows."""
    harch = _base() if arch == "base" else _large()
    eng = _engine(harch)
    lens = [320 * (T - 1) + 400 + d for T, d in ((199, 17), (33, 0), (1, 5), (129, 300), (70, 77))]
    from speech_inpainting_amd import synth
    wave = synth.synth_wave(len(lens), max(lens), 23).cuda()
    got, R, names = _run(eng, harch, wave, lens=lens, profile=True)
    print(f"\nragged {arch}: clips {[harch.num_frames(n) for n in lens]} frames, packed M = {R}; {sorted(n for n in names if 'gemm' in n)}")
    _check_layers(got, harch, R, f"ragged {arch}")
    _check_projection(got, harch, R, f"ragged {arch}", names)
    _check_convs(got, harch, len(lens), max(lens), f"ragged {arch}", clip_lens=lens)


def test_projection_without_layernorm_against_float64():
    """feat_proj_layer_norm=False: the projection reads the fp32 features themselves, so it runs on the tap-GEMM's bf16 path, whose
    staging rounds them (M = 257: two 128-row tiles and a last tile of one row)."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch
    harch = HubertArch(feat_proj_layer_norm=False, num_hidden_layers=1)
    eng = _engine(harch)
    T = 257
    got, R, names = _run(eng, harch, synth.synth_wave(1, 320 * (T - 1) + 400, 11).cuda(), profile=True)
    assert R == T
    _check_projection(got, harch, R, "no LayerNorm", names)
    _check_layers(got, harch, R, "no LayerNorm")


# ------------------------------------------------------------------------------------------------------------ attention


@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 199, 255, 256, 257, 384, 385, 499])
def test_bf16in_attention_against_float64(T):
    """attention_bf16in_whole_kernel (T <= 256: the clip's whole K / V in LDS) and attention_bf16in_kernel (T > 256, key tiles
    of 32 streamed), on the bf16 q | k | v the QKV GEMM stored: at the edges of the 32-key tiles and of the 128-query blocks."""
    from speech_inpainting_amd import synth
    harch = _base()
    eng = _engine(harch)
    wave = synth.synth_wave(2, 320 * (T - 1) + 400, 40 + T).cuda()
    got, R, names = _run(eng, harch, wave, profile=True)
    assert "attention_bf16" in names, names
    print(f"\nT={T}: {'whole-K/V' if T <= 256 else 'tiled'} kernel")
    _check_attention(got, harch, [(0, T, T), (T, T, T)], "bf16in", "bf16")


@pytest.mark.parametrize("env,kind,name", [({"SI_ATT_BF16": "0"}, "bf16", "attention_f32"), ({"SI_ENC_OPREADY": "0"}, "f32", "attention_f32")])
@pytest.mark.parametrize("T", [33, 257])
def test_fp32_attention_kernel_against_float64(env, kind, name, T):
    """attention_kernel (fp32 MFMA on the fp32 q | k | v): with a bf16 output (SI_ATT_BF16=0) and an fp32 one (SI_ENC_OPREADY=0).
    P is not rounded before P V here.  (attention_bf16_kernel -- fp32 q | k | v staged as bf16 -- is not reachable from the
    encoder: every path that would select it takes the bf16-input kernel.)"""
    from speech_inpainting_amd import synth
    harch = _base()
    eng = _engine(harch, env)
    wave = synth.synth_wave(2, 320 * (T - 1) + 400, 60 + T).cuda()
    got, R, names = _run(eng, harch, wave, profile=True)
    assert name in names and "attention_bf16" not in names, names
    _check_attention(got, harch, [(0, T, T), (T, T, T)], f"attention_kernel {env}", kind, p_bf16=False)


@pytest.mark.parametrize("T", [64, 300])
def test_padded_batch_attention_against_float64(T):
    """encode(valid_len=...): clips whose valid frame counts land at 1, 32, 33 and T - 1; the keys past them are excluded for
    EVERY query row, and every row (padded ones included) is compared."""
    from speech_inpainting_amd import synth
    harch = _base()
    eng = _engine(harch)
    frames = [1, 32, 33, T - 1]
    N = 320 * (T - 1) + 400
    valid = torch.tensor([320 * (f - 1) + 400 for f in frames], dtype=torch.int32, device="cuda")
    wave = synth.synth_wave(len(frames), N, 80 + T).cuda()
    got, R, _ = _run(eng, harch, wave, valid_len=valid)
    assert [harch.num_frames(int(v)) for v in valid] == frames
    _check_attention(got, harch, [(b * T, T, f) for b, f in enumerate(frames)], "padded", "bf16")


@pytest.mark.parametrize("frames", [[256, 33, 1, 129, 200, 32], [385, 32, 257, 100, 128]])
def test_ragged_batch_attention_against_float64(frames):
    """encode_ragged: packed rows, clips across the 32-key and 128-query tiles; the longest clip <= 256 frames (whole-K/V kernel)
    and > 256 (tiled kernel)."""
    from speech_inpainting_amd import synth
    harch = _base()
    eng = _engine(harch)
    lens = [320 * (f - 1) + 400 for f in frames]
    wave = synth.synth_wave(len(lens), max(lens), 90).cuda()
    got, R, _ = _run(eng, harch, wave, lens=lens)
    offs = [sum(frames[:b]) for b in range(len(frames))]
    _check_attention(got, harch, [(o, f, f) for o, f in zip(offs, frames)], "ragged", "bf16")


def test_ragged_batch_attention_of_the_large_encoder_against_float64():
    """The first frame list above on the large encoder: 16 heads (H = 1024; every other attention case here has 12)."""
    from speech_inpainting_amd import synth
    harch = _large()
    assert harch.num_attention_heads == 16
    frames = [256, 33, 1, 129, 200, 32]
    lens = [320 * (f - 1) + 400 for f in frames]
    wave = synth.synth_wave(len(lens), max(lens), 90).cuda()
    got, R, _ = _run(_engine(harch), harch, wave, lens=lens)
    offs = [sum(frames[:b]) for b in range(len(frames))]
    _check_attention(got, harch, [(o, f, f) for o, f in zip(offs, frames)], "ragged large", "bf16")


# ------------------------------------------------------------------------------------------------------- positional conv
PC_UNIFORM = [(3, 256), (2, 257), (1, 513)]
PC_RAGGED = [[256, 1, 255, 16, 17, 64, 65], [513, 1, 257, 512, 256, 511]]
PC_PADDED = (300, [1, 32, 33, 299])


def _pc_arch(cg):
    return _base() if cg == 48 else _large()


def _pc_engine(cg, kernel):
    """One engine per (width, kernel), kept for the session: SI_ENC_POSCONV is read when the context is created."""
    from tests.encoder_checks import PC_KERNELS
    return _engine(_pc_arch(cg), PC_KERNELS[kernel], key=("posconv", cg, kernel))


def _pc_both(cg, wave, lens=None, valid_len=None):
    return _pc_both_arch(_pc_arch(cg), wave, lens=lens, valid_len=valid_len, key=("posconv", cg))


def _check_posconv(runs, cg, clips, tag, valid=None):
    return _check_posconv_arch(runs, _pc_arch(cg), clips, tag, valid=valid)


@pytest.mark.parametrize("cg", [48, 64])
@pytest.mark.parametrize("B,T", PC_UNIFORM)
def test_posconv_uniform_batches_against_float64(B, T, cg):
    """(3, 256): two clips per workgroup with an odd batch -- the last workgroup's second half has no clip; (2, 257): 512-row
    blocks, the second half holding one row; (1, 513): two blocks per clip, the second holding one row.  Cg = 48: base (post-LN,
    where only the "pos_conv" tap shows the conv's output), 64: large (pre-LN)."""
    from speech_inpainting_amd import synth
    wave = synth.synth_wave(B, 320 * (T - 1) + 400, 120 + T).cuda()
    runs = _pc_both(cg, wave)
    print(f"\nCg={cg} B={B} T={T}: {[n for _, n in runs.values()]}")
    _check_posconv(runs, cg, [(b * T, T) for b in range(B)], f"uniform B={B}")


@pytest.mark.parametrize("cg", [48, 64])
@pytest.mark.parametrize("frames", PC_RAGGED)
def test_posconv_ragged_batches_against_float64(frames, cg):
    """encode_ragged, packed rows.  Tmax = 256: two clips per workgroup -- seven clips (the last workgroup has an empty half), clips
    of different lengths sharing a workgroup, a single-frame clip, a clip shorter than the 64-row padding, T = 64 | 65 where the
    first and last taps first reach a real row.  Tmax = 513: a two-block grid in which clips shorter than one half sit.  Every clip
    against float64, and bit-identical to the same clip run alone (256 and 255 run alone two per workgroup, but share the second
    batch's block grid): a clip's result does not depend on which other clip shares its workgroup."""
    from speech_inpainting_amd import synth
    harch = _pc_arch(cg)
    H = harch.hidden_size
    lens = [320 * (f - 1) + 400 for f in frames]
    wave = synth.synth_wave(len(lens), max(lens), 130 + len(frames)).cuda()
    runs = _pc_both(cg, wave, lens=lens)
    offs = [sum(frames[:b]) for b in range(len(frames))]
    print(f"\nCg={cg} ragged {frames}: {[n for _, n in runs.values()]}")
    _check_posconv(runs, cg, list(zip(offs, frames)), f"ragged Tmax={max(frames)}")
    R = sum(frames)
    for b, f in enumerate(frames):
        alone = wave[b:b + 1, :lens[b]].contiguous()
        for kernel, (got, name) in runs.items():
            one, R1, _ = _run(_pc_engine(cg, kernel), harch, alone, lens=[lens[b]])
            assert R1 == f
            assert torch.equal(one["pos_conv"].view(f, H), got["pos_conv"].view(R, H)[offs[b]:offs[b] + f]), \
                f"{name}: clip {b} ({f} frames) in the batch differs from the clip alone"


@pytest.mark.parametrize("cg", [48, 64])
def test_posconv_padded_batch_against_float64(cg):
    """encode(valid_len=...), T = 300, valid frames 1, 32, 33, 299: the conv reads "projected" with every frame >= the clip's valid
    count zeroed -- which also holds frame_lengths_kernel and zero_padded_rows_kernel to their definitions -- and is defined on
    all T rows."""
    from speech_inpainting_amd import synth
    harch = _pc_arch(cg)
    T, frames = PC_PADDED
    valid = torch.tensor([320 * (f - 1) + 400 for f in frames], dtype=torch.int32, device="cuda")
    assert [harch.num_frames(int(v)) for v in valid] == frames
    wave = synth.synth_wave(len(frames), 320 * (T - 1) + 400, 140).cuda()
    runs = _pc_both(cg, wave, valid_len=valid)
    print(f"\nCg={cg} padded T={T} valid {frames}: {[n for _, n in runs.values()]}")
    _check_posconv(runs, cg, [(b * T, T) for b in range(len(frames))], "padded", valid=frames)


def test_posconv_coverage_of_seams():
    """The cases above through the launcher's rule alone (pair mode when Tmax <= 256, else ceil(Tmax / 512) blocks of two 256-row
    halves per clip; 16-row MFMA tiles): together they reach pair mode, block mode with one and with two blocks per clip, a half
    without a clip or without a row of its clip, and last row tiles of 1, 15 and 16 rows.  Runs nothing on the GPU."""
    batches = [[T] * B for B, T in PC_UNIFORM] + PC_RAGGED + [[PC_PADDED[0]] * len(PC_PADDED[1])]
    reached, last_tiles = set(), set()
    for frames in batches:
        Tmax, B = max(frames), len(frames)
        pair = Tmax <= PC_HALF
        blocks = -(-Tmax // (2 * PC_HALF))
        reached.add("pair" if pair else f"blocks{blocks}")
        halves = []                                                    # (clip or None, first row) of every half of every workgroup
        if pair:
            halves = [(c if c < B else None, 0) for c in range(2 * ((B + 1) // 2))]
        else:
            halves = [(c, (2 * j + h) * PC_HALF) for c in range(B) for j in range(blocks) for h in range(2)]
        for c, r0 in halves:
            if c is None or r0 >= frames[c]:
                reached.add("empty half")
            else:
                last_tiles.add((min(frames[c] - r0, PC_HALF) - 1) % 16 + 1)
        for T in frames:
            if T < 64:
                reached.add("clip shorter than the padding")
        if pair and len(set(frames)) > 1:
            reached.add("clips of different lengths in a workgroup")
    print(sorted(reached), "last row tiles:", sorted(last_tiles))
    assert {"pair", "blocks1", "blocks2", "empty half", "clip shorter than the padding", "clips of different lengths in a workgroup"} <= reached, reached
    assert {1, 15, 16} <= last_tiles, last_tiles
    assert any(len(f) % 2 for f in batches if max(f) <= PC_HALF)      # pair mode with an odd batch: a half without a clip


# ------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("arch", ["base", "post1024", "large"])
def test_layernorm_against_float64(arch):
    """layernorm_kernel: C = 768 (base, post-LN) and 1024 (post-LN at H = 1024: fp32 rows + the bf16 operand, bit-equal to rne of
    the rows -- the claim the operand-ready copy rests on; pre-LN large: the bf16 operand only) and C = 512 (the layer flavour's
    LayerNorm + GELU behind every conv: bf16 only, the last one fp32)."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch
    harch = {"base": _base(), "large": _large(),
             "post1024": HubertArch(num_hidden_layers=1, hidden_size=1024, num_attention_heads=16, intermediate_size=4096)}[arch]
    eng = _engine(harch)
    B, T = 2, 140
    N = 320 * (T - 1) + 400
    got, R, _ = _run(eng, harch, synth.synth_wave(B, N, 5).cuda())
    _check_layernorms(got, harch, B, N, R, arch)


# ------------------------------------------------------------------------------------------------------------ conv0
@pytest.mark.parametrize("B,N", [(2, 16000), (1, 64000 + 37)])
def test_conv0_groupnorm_against_float64(B, N):
    """conv0 (k = 10, stride 5, fp32) + GroupNorm over each channel's frames + GELU, written as the bf16 operand of conv1, against
    the oracle's float64 form (un-normalised input: the samples are the operands)."""
    from speech_inpainting_amd import synth
    harch = _base()
    eng = _engine(harch)
    wave = synth.synth_wave(B, N, 3).cuda()
    got, R, _ = _run(eng, harch, wave)
    sd = _state(harch)
    pre = "base_model.feature_extractor.conv_layers.0."
    L1, C = harch.feat_lengths(N)[1], harch.conv_dim[0]
    y = got["conv0.bf16"].view(B, L1, C)
    for b in range(B):
        x = E.conv_rows(wave[b].cpu().double()[:, None], 10, 5, torch.arange(L1))
        ref, bound = E.conv0_groupnorm_ref(x, sd[pre + "conv.weight"][:, 0, :], sd[pre + "layer_norm.weight"], sd[pre + "layer_norm.bias"])
        _check(f"conv0 + GroupNorm + GELU clip {b} (L = {L1})", "bf16", y[b], ref, bound, "conv0")


def test_taps_change_no_value():
    """Registering every per-op tap (which also turns the LayerNorm-residual fusion off) leaves the encoder output EQUAL to the
    run without captures."""
    from speech_inpainting_amd import synth
    harch = _base()
    eng = _engine(harch)
    wave = synth.synth_wave(3, 30000, 99).cuda()
    plain = eng.encode(wave).cpu()
    cap = E.tap_capacities(harch, 3, 30000, 3 * harch.num_frames(30000))
    eng.ctx.capture(list(cap), capacity=cap)
    tapped = eng.encode(wave).cpu()
    eng.ctx.clear_captures()
    assert torch.equal(plain, tapped)
    assert torch.equal(eng.encode(wave).cpu(), plain)
