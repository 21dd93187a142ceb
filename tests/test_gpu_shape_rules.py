"""Every launcher's shape rule on both sides: the cases of tests/shape_rules.py -- per term of each rule one architecture at the last shape
the rule accepts and one a single step past it -- through the kernels, each op against the float64 reference of its own operation on the
operands the kernel read (tests/vocoder_ref.py, tests/encoder_ref.py; the bounds are the derived ones of those modules, nothing here is
fitted), and the profiled kernel families against `shape_rules.reaches(case)`.  And the descriptors that used to load and fail in
the first forward: refused when the engine is created from the descriptor, before any launch.

Generator (fp16 stream): one-stage architectures, one ragged batch of at most 32 clips whose lengths are `_pair_lengths` of the case's
own (k, d) (the chain's: its own stored rows), the uniform seam set for the first case of each group.  Encoder (bf16): one layer,
B = 2 clips of T = 140 frames (two 128-row tiles) and the ragged batch [140, 33, 129] for the first case of each group.

The share of bf16 outputs off rne(float64) per op: test_gpu_encoder_ops.py's MISMATCH_LIMIT was measured at K = 512 .. 4096 and is
asserted here only for a GEMM whose K is one of those widths (512, 768, 1024, 3072, 4096) and for LayerNorms of C = 512, 768, 1024.  For
the others the share is recorded (test_zz_encoder_summary prints it per width on every run) and held to twice the largest share measured
on MI355X at these widths: SMALL_K_LIMIT / SMALL_C_LIMIT below, with the measured figures."""
import pytest
import torch

from tests import encoder_checks as EC
from tests import encoder_ref as E
from tests import shape_rules as S
from tests.cases import R1, _config, _interleave, _mel, _pair_lengths
from tests.harness import RatioSummary
from tests.vocoder_checks import _engine, _ragged, _run, _uniform, _verify

pytestmark = pytest.mark.gpu

SUMMARY = RatioSummary(digits=3)


# ------------------------------------------------------------------------------------------------------------ generator
def _lengths(case):
    """The clip lengths of a case: those the case names, else the seam set of its own (k, d): the pair kernels' for a width they have
    a tile for, the 128- and 256-row seams of the tap-GEMM otherwise; the chain's own stored rows where the chain covers the block."""
    if case.lens is not None:
        return set(case.lens)
    C = S._padded(case.C)
    dils = sorted({d for ds in case.dils for d in ds})
    if C in R1:
        out = set(_pair_lengths(C, case.ks, dils))
    else:
        out = {1, 2, 127, 128, 129, 257} | {(k - 1) * d for k in case.ks for d in dils}
    for k, ds in zip(case.ks, case.dils):
        if "SI_VOC_CHAIN" not in case.env and S.holds("reschain", dict(C=C, k=k, dils=ds)):
            st = S.RC_R - (k - 1) * (sum(ds) + 3)
            out |= {S.RC_R, S.RC_R + 1, st - 1, st, st + 1, 2 * st + 1}
    return {v for v in out if v >= 1}


def _families(case, prof, tag):
    got, want = S.profiled_generator(prof), S.reaches(case)
    assert got == want, f"{tag}: the launches were {got}, the rules give {want} (profile: {sorted(prof)})"


def _group(name):
    return [c for c in S.GEN_CASES if c.group == name]


def _ids(cases):
    return [c.name for c in cases]


def _run_case(case, seed, ops=("rb", "post"), uniform=False):
    varch = S.gen_arch(case)
    eng = _engine(varch, case.env)
    prof = _ragged(eng, varch, _lengths(case), seed, case.name, SUMMARY, ops=ops)
    _families(case, prof, case.name)
    if uniform:
        C, k = S._padded(case.C), case.ks[0]
        st = R1.get(C, 128) - (k - 1)
        for L in sorted({1, 2, k - 1, st - 1, st, st + 1, 2 * st + 1} - {0}):
            p = _uniform(eng, varch, L, seed + 1, case.name, SUMMARY, ops=ops)
            _families(case, p, f"{case.name} uniform L={L}")
    return prof


@pytest.mark.parametrize("case", _group("pairs inside"), ids=_ids(_group("pairs inside")))
def test_pairs_inside_the_rule(case):
    """respair.hip / respair_wide.hip at (k, d) nobody has run: k = 5 x (2, 4, 6), k = 9 x (1, 2, 6), k = 3 x (1, 12, 25) -- (k - 1) d = 50, the
    halo's last row -- at all four widths.  Every launch a respair launch."""
    prof = _run_case(case, 3000 + case.C + case.ks[0], uniform=case is _group("pairs inside")[0])
    assert not any(n.startswith("reschain") for n in prof)


@pytest.mark.parametrize("case", _group("pairs past"), ids=_ids(_group("pairs past")))
def test_pairs_one_step_past_the_rule(case):
    """(k - 1) d = 52 and 60, k = 13, k = 1, a width with no instantiation: both convs of every pair on the tap-GEMM, no respair launch."""
    prof = _run_case(case, 3100 + case.C + case.ks[0], uniform=case is _group("pairs past")[0])
    assert not any(n.startswith(("respair", "reschain")) for n in prof), sorted(prof)


@pytest.mark.parametrize("case", _group("block of both") + _group("stage of both"), ids=_ids(_group("block of both") + _group("stage of both")))
def test_fused_and_unfused_pairs_hand_the_stream_to_each_other(case):
    """A block whose pairs lie on both sides of the halo rule -- (1, 25, 26) and (26, 1, 25): fused -> two-launch and two-launch -> fused through
    h16[4 + (n & 1)] -- and a stage whose middle block (k = 13) falls back: the MRF accumulate and the 1 / 3 scale cross it."""
    _run_case(case, 3200 + case.C, uniform=case is _group("block of both")[0])


@pytest.mark.parametrize("case", _group("chain"), ids=_ids(_group("chain")))
def test_chain_inside_its_rule(case):
    """reschain.hip at the limit of each term: k = 3 x (25, 25, 25), where the pair kernels cover every pair too and the bits must be equal;
    k = 7 x (10, 10, 9): 2 H = 192 = RC_R / 4, 576 stored rows; k = 11 x (1, 6, 6) and k = 3 x (32, 25, 25): the chain covers what the pair
    kernels refuse, so its x_2 comes from a SI_VOC_CHAIN=0 run through the tap-GEMM and the float64 bound alone holds it."""
    varch = S.gen_arch(case)
    lens = _interleave(_lengths(case))
    assert len(lens) <= 32
    mel = _mel(len(lens), max(lens), 3300 + case.ks[0] + sum(case.dils[0]))
    pairs = _run(_engine(varch, S.NOCHAIN), varch, mel, lens)
    pairs_case = case._replace(env=S.NOCHAIN)
    _families(pairs_case, pairs[2], case.name + " pairs")
    equal = all(S.holds("respair", dict(C=32, k=case.ks[0], d=d)) for d in case.dils[0])
    assert equal == (case.note == "equal")
    _verify(varch, mel, lens, *pairs, case.name + " pairs", SUMMARY, ops=("rb",))
    taps, wave, prof = _run(_engine(varch), varch, mel, lens)
    _families(case, prof, case.name)
    assert "stage0.rb0.p0.f16" not in taps and "stage0.rb0.p2.f16" in taps
    _verify(varch, mel, lens, taps, wave, prof, case.name, SUMMARY, ops=("rb", "post"), x2_from=pairs[0], chain_equal=equal)
    if equal:
        assert torch.equal(wave, pairs[1])
    if case is _group("chain")[0]:                         # the uniform seam set: one clip twice, around the chain's own stored rows
        st = S.RC_R - (case.ks[0] - 1) * (sum(case.dils[0]) + 3)
        for L in (1, 2, st - 1, st, st + 1, 2 * st + 1):
            one = _mel(1, L, 3390 + L)
            mel2 = torch.cat([one, one]).contiguous()
            p2 = _run(_engine(varch, S.NOCHAIN), varch, mel2)
            t2, w2, prof2 = _run(_engine(varch), varch, mel2)
            _families(case, prof2, f"{case.name} uniform L={L}")
            _verify(varch, mel2, None, t2, w2, prof2, f"{case.name} uniform L={L}", SUMMARY, ops=("rb", "post"), clips=[0], x2_from=p2[0], chain_equal=equal)
            for k, t in t2.items():
                assert torch.equal(t[0], t[1]), f"{case.name} uniform L={L}: {k} differs between two copies of one clip"
            assert torch.equal(w2[0], w2[1]) and torch.equal(w2, p2[1])


@pytest.mark.parametrize("case", _group("chain refused"), ids=_ids(_group("chain refused")))
def test_chain_refused_by_one_term(case):
    """One term of si_launch_reschain's rule broken at a time (2 H = 198, (k - 1) / 2 d = 35 and 33, k = 13, k = 1, C = 64, num_dil = 2 and 4):
    no reschain launch, the pairs one by one on whatever their own rule gives."""
    prof = _run_case(case, 3400 + case.C + case.ks[0] + len(case.dils[0]), uniform=case is _group("chain refused")[0])
    assert not any(n.startswith("reschain") for n in prof), sorted(prof)


@pytest.mark.parametrize("case", _group("upsamplers"), ids=_ids(_group("upsamplers")))
def test_upsamplers_on_both_sides_of_their_rules(case):
    """upsample.hip (u = 2, k = 4, Cin 64 / 128), gemmcu's TC kernel (two taps, N % 256 == 0, Cin % 64 == 0; N = 256 and 768: one and three
    column tiles) and, one term past each, the tap-GEMM: one tap (k = u), three taps, k no multiple of u, N = 128 / 384, Cin = 32 / 96 / 256.
    Lin = 1, 2, 255, 256, 257."""
    _run_case(case, 3500 + case.C + case.u + case.ku, ops=("pre", "ups"), uniform=False)
    if case is _group("upsamplers")[0]:
        varch = S.gen_arch(case)
        for L in S.UPS_LIN:
            _uniform(_engine(varch, case.env), varch, L, 3599, case.name, SUMMARY, ops=("ups",))


def test_a_mel_width_the_packer_pads_runs():
    """num_mels = 1 and 81 (conv_pre's rows padded to 32 and 96 channels, zero weights behind the real ones): conv_pre against its reference."""
    from tests.cases import _arch
    for nm in (1, 81):
        varch = _arch(32, num_mels=nm, resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1,),))
        _ragged(_engine(varch), varch, {1, 2, 127, 128, 129}, 3600 + nm, f"num_mels={nm}", SUMMARY, ops=("pre",))


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", [c for c in _group("pairs past") if c.C == 64], ids=_ids([c for c in _group("pairs past") if c.C == 64]))
def test_the_fallback_shapes_in_fp32_and_bf16x3(case, mode):
    """The blocks no fused kernel takes ((k - 1) d = 52 and 60, k = 13, k = 1) through the tap-GEMM's other arithmetics, every launch against
    tapgemm_ref: M = 129 and 257, on both sides of the 128- and 256-row tiles."""
    from tests import tapgemm_checks as TG
    varch = S.gen_arch(case)
    for M in (129, 257):
        TG._uniform(varch, mode, M, 3650 + case.ks[0] + M, f"{mode} {case.name}", SUMMARY)


# -------------------------------------------------------------------------------------- the tap-GEMM's tile switch, moved by the halo
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("C", [128, 64])
def test_tapgemm_tile_switch_by_halo(mode, C):
    """launch_math takes the 256-row tile while (255 + (ntaps - 1) |dil| + 1) 8 float4 fit 3072: at k = 11, d = 12 (376 rows) it does, at
    d = 13 (386) it does not.  M = 257 and 300; the family names from cases._config, every launch against tapgemm_ref."""
    from tests import tapgemm_checks as TG
    from tests.cases import _arch
    math = TG.MODES[mode][1]
    seen = set()
    for d in (12, 13):
        varch = _arch(C, resblock_kernel_sizes=(11,), resblock_dilation_sizes=((d,),))
        for M in (257, 300):
            cfgs, _, _ = TG._uniform(varch, mode, M, 3700 + C + d + M, f"{mode} C={C} k=11 d={d}", SUMMARY)
            seen.add((d, _config(math, C, M, 11, d, C)))
            assert _config(math, C, M, 11, d, C)[0] in cfgs
    assert {bm for d_, (_, bm) in seen if d_ == 12} == {256} and {bm for d_, (_, bm) in seen if d_ == 13} == {128}, seen


# ------------------------------------------------------------------------------------------------------------ encoder
ENC_T, ENC_RAGGED = 140, [140, 33, 129]                # two 128-row tiles; a ragged batch of 302 packed rows
MEASURED_K = (512, 768, 1024, 3072, 4096)              # the widths test_gpu_encoder_ops.py's MISMATCH_LIMIT was measured at
MEASURED_C = (512, 768, 1024)
# Share of bf16 outputs != rne(float64 reference) at the widths of this file: twice the largest share measured on MI355X over this
# file's runs (the convention of test_gpu_encoder_ops.py), per K of the GEMM / per C of the LayerNorm.  Measured: see the docstring of
# test_zz_encoder_summary, which prints the table again on every run.
# Measured (GEMM K: share, checks): 64: 0.0223 %, 20 | 96: 0.2392 %, 64 (the tiny conv stack's k = 3 convs) | 128: 0.0181 %, 8 | 192: 0.0790 %, 6 |
# 256: 0.0089 %, 4 | 384: 0.0190 %, 6 | 2048: 0.0213 %, 2;  (LayerNorm C: share, checks): 16: 0.0143 %, 2 | 32: 0.0500 %, 16 | 128: 0.0028 %, 3 |
# 1040: 0.0113 %, 2 | 64: none of 17920 outputs in its one check, so its limit is two outputs of that tensor.
SMALL_K_LIMIT = {64: 2 * 0.000223, 96: 2 * 0.002392, 128: 2 * 0.000181, 192: 2 * 0.000790, 256: 2 * 0.000089, 384: 2 * 0.000190, 2048: 2 * 0.000213}
SMALL_C_LIMIT = {16: 2 * 0.000143, 32: 2 * 0.000500, 64: 2 / 17920, 128: 2 * 0.000028, 1040: 2 * 0.000113}
ENC_NOTES = []                                         # (case, op, K or C, kind, share, err / E)


def _samples(harch, T):
    """The smallest sample count that gives T frames."""
    hop = 1
    for s in harch.conv_stride:
        hop *= s
    n = hop * (T - 1)
    while harch.num_frames(n) < T:
        n += 1
    assert harch.num_frames(n) == T
    return n


def _wave(harch, B, T, seed):
    from speech_inpainting_amd import synth
    return synth.synth_wave(B, _samples(harch, T), seed).cuda()


def _op_width(tag, harch):
    """(kind of limit, K of the GEMM or C of the LayerNorm) of a check by its tag."""
    H, I, CF = harch.hidden_size, harch.intermediate_size, harch.conv_dim[-1]
    if "keys=" in tag:
        return "attention", H
    if "GroupNorm" in tag:
        return "conv0", harch.conv_dim[0]
    if "LayerNorm" in tag or " ln1 " in tag or " ln2 " in tag:
        import re
        return "ln", int(re.search(r"C = (\d+)", tag).group(1))
    if "FFN2" in tag:
        return "gemm", I
    if "projection (K" in tag:
        return "gemm", CF
    for i in range(1, len(harch.conv_dim)):
        if f" conv{i} " in tag:
            return "gemm", harch.conv_kernel[i] * harch.conv_dim[i - 1]
    return "gemm", H


def _checked(case, harch, body):
    """Run `body(**ck)` (calls of encoder_checks, which take their limits and their notes as arguments): conv0 (K = 10 at every width) and the
    attention (head_dim 64 at every width) are held to MISMATCH_LIMIT by `_check` itself; the GEMM and LayerNorm shares are noted and then
    held to the limit of their own width: MISMATCH_LIMIT at a measured width, SMALL_K_LIMIT / SMALL_C_LIMIT otherwise."""
    notes = []
    body(limits=dict(EC.MISMATCH_LIMIT, gemm=None, ln=None), notes=notes)
    mine = [(tag, kind, key, share, worst) + _op_width(tag, harch) for tag, kind, key, share, worst in notes]
    ENC_NOTES.extend((case.name, tag, what, width, kind, share, worst) for tag, kind, key, share, worst, what, width in mine)
    for tag, kind, key, share, worst, what, width in mine:
        if kind != "bf16" or key not in ("gemm", "ln"):
            continue
        if width in (MEASURED_K if what == "gemm" else MEASURED_C):
            limit = EC.MISMATCH_LIMIT[key]
        else:
            limit = (SMALL_K_LIMIT if what == "gemm" else SMALL_C_LIMIT).get(width)
        assert limit is not None, f"{case.name} {tag}: no recorded share for {what} width {width} (measured {share:.5f})"
        assert share <= limit, f"{case.name} {tag}: {100 * share:.4f} % of the outputs are off rne(float64), the limit at width {width} is {100 * limit:.4f} %"


def _gemm_families(case, harch, names, R, env=None):
    """The profiled names against reaches(case): each GEMM on the family the rules give (the instantiation by _linear_kernel's rule)."""
    want = S.reaches(case, captures=True, env=env)
    shapes = S.enc_gemms(harch)
    for op, fam in want.items():
        if op in shapes:
            kern = EC._linear_kernel(R, shapes[op]["N"], shapes[op]["K"], env, x16=(op != "projection" or harch.feat_proj_layer_norm))
            assert kern.startswith(tuple(fam.split("|"))), (case.name, op, kern, fam)
            assert kern in names, (case.name, op, kern, sorted(names))
        elif op == "pos_conv":
            assert any(n.startswith(fam) for n in names), (case.name, op, fam, sorted(names))
            assert fam.startswith("posconv") or not any(n.startswith("posconv_") for n in names), sorted(names)
    ded = any(f != "tapgemm_bf16" for op, f in want.items() if op in shapes)
    assert ded == any(n.startswith(("gemmcu_bf16_", "lingemm_bf16_")) for n in names), (case.name, sorted(names))


def _check_run(case, harch, got, R, names, B, N, tag, clip_lens=None, env=None):
    def body(**ck):
        EC._check_layers(got, harch, R, tag, **ck)
        EC._check_projection(got, harch, R, tag, names, env, **ck)
        EC._check_convs(got, harch, B, N, tag, clip_lens=clip_lens, **ck)
        if clip_lens is None:
            EC._check_layernorms(got, harch, B, N, R, tag, **ck)
            EC._check_attention(got, harch, [(b * (R // B), R // B, R // B) for b in range(B)], tag, "bf16", **ck)
    _checked(case, harch, body)
    _gemm_families(case, harch, names, R, env)


@pytest.mark.parametrize("case", S.ENC_CASES, ids=_ids(S.ENC_CASES))
def test_encoder_widths_on_both_sides_of_the_gemm_rules(case):
    """One layer at H = 64 .. 2048 (K of one k-step, N % 128 != 0, three 128-column tiles, an FFN width lingemm refuses on either side, the
    widest LayerNorm row), seven conv widths, two convs, the layer flavour at 16 and 1040 channels: every GEMM, conv, LayerNorm and the
    attention against float64 under the derived bounds, on the kernel family the rules give."""
    harch = S.enc_arch(case)
    eng = EC._engine(harch)
    wave = _wave(harch, 2, ENC_T, 4000 + harch.hidden_size)
    got, R, names = EC._run(eng, harch, wave, profile=True)
    assert R == 2 * ENC_T
    _check_run(case, harch, got, R, names, 2, wave.shape[1], case.name)
    if case.name in ("E6", "E6b"):                         # the group flavour's conv0 at 64 channels
        sd = EC._state(harch)
        pre = "base_model.feature_extractor.conv_layers.0."
        L1, C = harch.feat_lengths(wave.shape[1])[1], harch.conv_dim[0]
        for b in range(2):
            x = E.conv_rows(wave[b].cpu().double()[:, None], 10, 5, torch.arange(L1))
            ref, bound = E.conv0_groupnorm_ref(x, sd[pre + "conv.weight"][:, 0, :], sd[pre + "layer_norm.weight"], sd[pre + "layer_norm.bias"])
            # (K = 10 at every width: MISMATCH_LIMIT["conv0"] applies; measured at C = 64: 0.0312 % of 574400 outputs, the limit is 0.103 %)
            _checked(case, harch, lambda **ck: EC._check(f"{case.name} conv0 + GroupNorm + GELU clip {b} (C = {C})", "bf16", got["conv0.bf16"].view(2, L1, C)[b],
                                                         ref, bound, "conv0", **ck))
    if case is S.ENC_CASES[0] or case.name in ("E3", "E6"):
        from speech_inpainting_amd import synth
        lens = [_samples(harch, f) for f in ENC_RAGGED]
        w = synth.synth_wave(len(lens), max(lens), 4100).cuda()
        got, R, names = EC._run(eng, harch, w, lens=lens, profile=True)
        assert R == sum(ENC_RAGGED)
        _check_run(case, harch, got, R, names, len(lens), max(lens), case.name + " ragged", clip_lens=lens)
        offs = [sum(ENC_RAGGED[:b]) for b in range(len(ENC_RAGGED))]
        _checked(case, harch, lambda **ck: EC._check_attention(got, harch, [(o, f, f) for o, f in zip(offs, ENC_RAGGED)], case.name + " ragged", "bf16", **ck))


GEMM_TAPS = ("layer0.qkv.bf16", "layer0.att_res", "layer0.ffn.bf16", "layer0.ffn_res", "projected")


@pytest.mark.parametrize("case", S.ENC_CASES, ids=_ids(S.ENC_CASES))
def test_every_gemm_is_bit_equal_across_the_gemmcu_knob(case):
    """DESIGN's knob table: the default, SI_ENC_GEMMCU=2 (every shape an instantiation covers) and each 10 + c whose BN divides N give the
    same bits in every GEMM output -- each instantiation sums the k-steps in the same order."""
    harch = S.enc_arch(case)
    wave = _wave(harch, 2, ENC_T, 4200 + harch.hidden_size)
    base, R, names0 = EC._run(EC._engine(harch), harch, wave, profile=True)
    ran = set()
    for knob in ("2",) + tuple(str(10 + c) for c in range(6)):
        got, _, names = EC._run(EC._engine(harch, {"SI_ENC_GEMMCU": knob}), harch, wave, profile=True)
        ran |= {n for n in names if n.startswith("gemmcu_bf16_")}
        for t in GEMM_TAPS:
            assert torch.equal(got[t], base[t]), f"{case.name}: {t} differs between the default and SI_ENC_GEMMCU={knob} ({sorted(n for n in names if 'gemm' in n)})"
    want = S.reaches(case, captures=True)
    if any(f != "tapgemm_bf16" for op, f in want.items() if op in S.enc_gemms(harch)):
        assert ran, (case.name, "no gemmcu instantiation ran under any knob")
        print(f"   {case.name}: {sorted(ran)}")


@pytest.mark.parametrize("name", ["E3", "E4b", "E2", "E4a"])
def test_layernorm_residual_fusion_keeps_the_bits(name):
    """ln_fuse (H % 128 == 0, I % 64 == 0, no capture).  E3, E4b: the final output with SI_ENC_LNFUSE 1 and 0 is equal, and the fused route
    ran: the same LayerNorm launches write fewer profiled bytes (no fp32 rows that only a residual would read).  One step past each modulus
    (E2: H = 192; E4a: I = 272) the same two runs: equal output, and the LayerNorms write the same bytes -- the switch changes nothing."""
    case = S.ENC[name]
    harch = S.enc_arch(case)
    fused = S.reaches(case, captures=False)["ln_residual"] == "fused"
    assert fused == (name in ("E3", "E4b")) and S.reaches(case, captures=True)["ln_residual"] == "written"
    wave = _wave(harch, 2, ENC_T, 4300)
    outs, profs = {}, {}
    for knob in ("1", "0"):
        eng = EC._engine(harch, {"SI_ENC_LNFUSE": knob})
        eng.ctx.profile_start(4000)
        try:
            outs[knob] = eng.encode(wave, normalize=False).cpu()
        finally:
            profs[knob] = {e["name"]: e for e in eng.ctx.profile_stop()}
    assert torch.equal(outs["1"], outs["0"]), f"{name}: SI_ENC_LNFUSE changes the output"
    ln1, ln0 = profs["1"]["layernorm"], profs["0"]["layernorm"]
    assert ln1["launches"] == ln0["launches"], (name, ln1, ln0)
    assert (ln1["bytes"] < ln0["bytes"]) if fused else (ln1["bytes"] == ln0["bytes"]), (name, ln1, ln0)
    if not fused:
        assert {n: e["launches"] for n, e in profs["1"].items()} == {n: e["launches"] for n, e in profs["0"].items()}


@pytest.mark.parametrize("case", S.PC_CASES, ids=_ids(S.PC_CASES))
def test_positional_conv_on_both_sides_of_its_rule(case):
    """posconv.hip at (Cg 48, k 64), (48, 8), (64, 2), (64, 128) and the tap-GEMM one term past: (ntaps Cg) % 128 != 0 (k = 4 at 48, k = 127),
    ntaps = 129 and 130, Cg = 32 and 80.  Both routes against one float64 reference per clip; where the rule refuses the shape the default
    engine takes the fallback by itself with the bits of SI_ENC_POSCONV=0."""
    harch = S.enc_arch(case)
    covered = S.reaches(case)["pos_conv"].startswith("posconv")
    assert covered == (case.group == "posconv")
    wave = _wave(harch, 2, ENC_T, 4400 + harch.num_conv_pos_embeddings)
    runs = EC._pc_both(harch, wave, covered=covered)
    worst = EC._check_posconv(runs, harch, [(0, ENC_T), (ENC_T, ENC_T)], case.name)
    ENC_NOTES.append((case.name, "pos_conv " + "/".join(n for _, n in runs.values()), "gemm", harch.num_conv_pos_embeddings * harch.hidden_size // harch.num_conv_pos_embedding_groups,
                      "f32", None, worst))
    if case is S.PC_CASES[0] or case.name == "P64k127":
        from speech_inpainting_amd import synth
        lens = [_samples(harch, f) for f in ENC_RAGGED]
        w = synth.synth_wave(len(lens), max(lens), 4500).cuda()
        runs = EC._pc_both(harch, w, lens=lens, covered=covered)
        offs = [sum(ENC_RAGGED[:b]) for b in range(len(ENC_RAGGED))]
        EC._check_posconv(runs, harch, list(zip(offs, ENC_RAGGED)), case.name + " ragged")


@pytest.mark.parametrize("case", S.ENC_CASES + [S.ENC["P64k127"], S.ENC["P64k129"], S.ENC["P80"]],
                         ids=_ids(S.ENC_CASES + [S.ENC["P64k127"], S.ENC["P64k129"], S.ENC["P80"]]))
def test_fp32_stage_taps_match_the_oracle(case):
    """fp32 mode: "features", "projected", "encoder_in" and "last_hidden" against oracle.ref_cpu.custom_model_forward at
    test_stage_taps_match_oracle's criterion, rms <= 2e-5 max(rms ref, 1)."""
    from oracle import ref_cpu as R
    from speech_inpainting_amd.arch import VocoderArch
    from tests.common import rms
    from tests.harness import build_engine, tapped_run
    harch = S.enc_arch(case)
    sd = EC._state(harch)
    eng = build_engine(harch, VocoderArch.tiny(), 50, "fp32", "fp32", state=(sd, None, None))
    wave = _wave(harch, 2, ENC_T, 4600 + harch.hidden_size)
    want = {}
    R.custom_model_forward(sd, harch, wave.cpu(), taps=want)
    names = ("features", "projected", "encoder_in", "last_hidden")
    n = 2 * ENC_T
    cap = {"features": n * harch.conv_dim[-1], "projected": n * harch.hidden_size, "encoder_in": n * harch.hidden_size, "last_hidden": n * harch.hidden_size}
    got, _, _ = tapped_run(eng.ctx, cap, lambda: eng.encode(wave, normalize=False), require_all=True, profile=False)
    for nm in names:
        ref = want[nm].reshape(-1)
        assert got[nm].numel() == ref.numel(), nm
        r = rms(got[nm], ref)
        print(f"   {case.name} {nm}: rms err {r:.3e} (rms ref {rms(ref, torch.zeros_like(ref)):.3e})")
        assert r <= 2e-5 * max(rms(ref, torch.zeros_like(ref)), 1.0), (case.name, nm, r)


# ------------------------------------------------------------------------------------------------------------ refusals at load
def test_every_architecture_of_this_file_loads_and_runs_one_step():
    """Each generator and encoder architecture above as one half of an engine: load_state and one step, no SI_EINVAL -- a vocode for the
    generators, a predict for the encoders (an encode for E6b, whose two-conv stack predict's frame arithmetic does not fit)."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch, mel_frames
    from tests.harness import build_engine
    archs = {repr(S.gen_arch(c)): S.gen_arch(c) for c in S.GEN_CASES}
    for varch in archs.values():
        eng = build_engine(HubertArch.tiny(), varch, 20, "fp32", "fp16")
        out = eng.vocode(_mel(1, 9, 5, varch.num_mels).cuda())
        assert bool(torch.isfinite(out).all())
    N, lm = 8000, 5
    for case in S.ENC_CASES + S.PC_CASES:
        harch = S.enc_arch(case)
        if len(harch.conv_dim) != 7:                                    # E6b: predict's frame arithmetic is the seven-conv stack's, so its step is an encode
            eng = build_engine(harch, VocoderArch.tiny(), 100, "bf16", "fp16")
            assert bool(torch.isfinite(eng.encode(_wave(harch, 2, 25, 9))).all()), case.name
            continue
        eng = build_engine(harch, VocoderArch.tiny(), 100, "bf16", "fp16")
        Tm = mel_frames(N * 22050 // 16000)
        out = eng.predict_batch(synth.synth_wave(2, N).cuda(), synth.synth_mel(2, Tm).cuda(), torch.tensor([3, 11], dtype=torch.int32).cuda(), lm)
        assert bool(torch.isfinite(out["wave"]).all()), case.name


REFUSED = [
    ("hidden_size", dict(hidden_size=2112, num_attention_heads=33), {}),
    ("conv_dim[0]", dict(conv_dim=(48,) + (32,) * 6), {}),
    ("conv_dim[0]", dict(conv_dim=(2048,) + (32,) * 6), {}),
    ("conv_kernel[0]", dict(conv_kernel=(8, 3, 3, 3, 3, 2, 2)), {}),
    ("conv_dim[1]", dict(conv_dim=(32, 2064, 32, 32, 32, 32, 32), feat_extract_norm="layer"), {}),
    ("final generator width 256", {}, dict(upsample_rates=(1,), upsample_kernel_sizes=(3,), upsample_initial_channel=512)),
    ("up_kernels[0]", {}, dict(upsample_rates=(3,), upsample_kernel_sizes=(6,), upsample_initial_channel=512)),
]


@pytest.mark.parametrize("field,hkw,vkw", REFUSED, ids=[f"{r[0]} {i}" for i, r in enumerate(REFUSED)])
def test_widths_no_kernel_takes_are_refused_at_load(field, hkw, vkw):
    """The neighbours that used to load and fail inside the first forward (H = 2112, conv_dim[0] = 48 and 2048, conv kernel 8, a layer
    flavour 2064 wide, a generator that ends 256 wide; and u = 3, k = 6, whose odd difference never loaded): the engine refuses them when
    it is created from the descriptor, naming the field, before any launch."""
    from speech_inpainting_amd import native
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.engine import InpaintingEngine
    harch, varch = HubertArch.tiny(**hkw), (VocoderArch(**vkw) if vkw else VocoderArch.tiny())
    with pytest.raises(native.NativeError, match=field.replace("[", r"\[").replace("]", r"\]")):
        InpaintingEngine(harch, varch, 20, "cuda:0", "bf16", "fp16")


def test_zz_encoder_summary():
    """(last) per (GEMM K | LayerNorm C): the largest share of bf16 outputs off rne(float64) and the largest err / E over this file's runs.
    Measured on MI355X: see DESIGN.md 4.38."""
    rows = {}
    for case, tag, what, width, kind, share, worst in ENC_NOTES:
        r = rows.setdefault((what, width), [0.0, 0.0, 0])
        r[0], r[1], r[2] = max(r[0], share or 0.0), max(r[1], worst), r[2] + 1
    for (what, width), (share, worst, n) in sorted(rows.items()):
        print(f"   ENC SUMMARY {what} width {width}: share off rne {100 * share:.4f} %, max err/E {worst:.4f} over {n} checks")
        assert worst <= 1.0


def test_zz_summary_of_ratios():
    """(last of the generator's) the largest err / E per kernel family over every check above."""
    SUMMARY.report()
