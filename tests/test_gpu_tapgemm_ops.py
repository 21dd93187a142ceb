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

import pytest
import torch

from tests import encoder_ref as E
from tests import tapgemm_checks as TG
from tests import vocoder_ref as V
from tests.cases import _arch, _config, _enc_state, _mel, _pick_wave, _sel_rows
from tests.harness import RatioSummary, build_engine, tapped_run
from tests.tapgemm_checks import MODES, _engine, _reached, _run

pytestmark = pytest.mark.gpu

SUMMARY = RatioSummary()                              # this file's max err / E per kernel configuration
TILES = ("128x32", "256x32", "128x64", "256x64", "128x128", "256x128w8")
ROWS = (127, 128, 129, 255, 256, 257, 513)
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


def _verify(*args, summary=SUMMARY, **kw):
    return TG._verify(*args, summary=summary, **kw)


def _uniform(*args, summary=SUMMARY, **kw):
    return TG._uniform(*args, summary=summary, **kw)


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


def _enc_engine(name):
    """fp32 encoder, one layer, real widths; one per width, kept for the session."""
    from speech_inpainting_amd.arch import VocoderArch
    harch = _harch(name)
    return build_engine(harch, VocoderArch.tiny(), 50, "fp32", "fp32", state=(_enc_state(harch), None, None), key=("tapgemm-enc", name))


def _enc_run(eng, harch, wave, lens=None):
    """One fp32 encoder forward with every tap registered -> (taps, transformer rows, {kernel: launches}, what encode returned)."""
    B, N = wave.shape
    R = sum(harch.num_frames(n) for n in lens) if lens is not None else B * harch.num_frames(N)
    cap = {k: v for k, v in E.tap_capacities(harch, B, N, R).items() if not k.endswith(".bf16")}
    for nm in ("projected", "encoder_in", "last_hidden"):
        cap[nm] = R * harch.hidden_size
    cap["features"] = R * harch.conv_dim[-1]
    got, out, prof = tapped_run(eng.ctx, cap, lambda: eng.encode_ragged(wave, lens, normalize=False) if lens is not None
                                else eng.encode(wave, normalize=False))
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
    SUMMARY.note(kernel, near, rest)


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
            SUMMARY.note(kern, r["worst"], 0.0)
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
        SUMMARY.note(kern + f" groups BK={32 if cg % 32 == 0 else 16}", near, rest)
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
    SUMMARY.report()
