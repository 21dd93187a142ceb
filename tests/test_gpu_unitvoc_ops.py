"""The I_da unit vocoder's kernels (hubert_lut.json: rates (5, 4, 4, 2, 2), kernels (11, 8, 8, 4, 4), 384 input channels, 512 -> 16
channels) launch by launch against the float64 references of tests/vocoder_ref.py, through the checks of tests/vocoder_checks.py (the fp16
stream) and tests/tapgemm_checks.py (fp32, bf16x3, bf16).  The geometry reaches code no V1 case enters:

  u = 5, k = 11     three taps per phase ((k + u - 1) / u), 4 of the 15 (phase, tap) slots zero weights, crop pad = 3, ooff = -3 Cout: the
                    tap-GEMM in all four arithmetics (gemmcu's TC kernels take two taps only).  Lin = 1, 2, 3 (every output row meets the crop)
                    and Lin + 1 = M = 127, 128, 129, 255, 256, 257, the GEMM row counts at which launch_math changes the tile.
  u = 4, k = 8      gemmcu.hip's TC instantiations at N = u Cout = 512 (256 -> 128, two column tiles) and 256 (128 -> 64, one), crop pad = 2.
                    192 x 256 serves the small batches; 256 x 256 wins the cost rule rounds x (BM + 256) where 192-row tiles need a second
                    round of the chip and 256-row tiles do not: with 256 CUs, 32 clips of M = 800 rows at N = 512 (4 x 32 x 2 = 256 tiles
                    against 5 x 32 x 2 = 320) and 32 clips of M = 1600 at N = 256 (7 x 32 = 224 against 9 x 32 = 288).  `_tc_batch` restates the
                    rule with the device's own CU count and searches for such a batch, so both instantiations are reached at both widths.
  16 channels       fp16: the stage is carried padded to 32 (stage_channels): the upsampler on the tap-GEMM with N = 2 x 32, the stage on
                    reschain_f16_c32 / respair_f16_c32, conv_post on the MFMA kernel; channels 16..31 must be exactly zero in every tap and
                    channels 0..15 meet the references of the REAL width (sixteen exact zero products round nothing).  u = 2 puts the stage
                    at even rows only, so the (u = 2, k = 4) architecture runs at the even rows on both sides of every seam and a (u = 1, k = 3)
                    one puts the same padded stage at exactly the rows of the C = 32 pair and chain tests.
                    fp32 / bf16x3 / bf16: width 16 is real: N = 16 inside a 32-column tile, Cin = 16 so BK = 16 on an ungrouped conv,
                    conv_post_kernel at C = 16.
  conv_pre 384      packed K = 7 x 384 on an N(0, 0.5^2) input.
  the whole vocoder every tap of every stage in fp16 and bf16x3, the hand-off of stage 0 to the TC upsampler, taps inert, ragged = alone.

Every assertion is |got - ref| <= E over all real rows and channels of a clip with the bounds of vocoder_ref.py as they stand: no new tolerance.
Uniform batches hold one clip twice (clip 1 must equal clip 0 bit for bit); every run asserts the kernel families in its profile.
tests/test_vocoder_ref.py composes the references of every fp16 input below (`fp16_inputs`, tests/cases.py) on the CPU and asserts the saturation condition
(max |ref| < 65504 / 4) that `_one` asserts on the device.

Measured on MI355X (test_zz_summary_of_ratios; max err / E over rows near a seam or clip edge | the rest; records, not limits; RECORD has
every group and kernel): fp16 stream -- tap-GEMM as the (5, 11) upsampler 0.89 | 0.90, as the padded stage's upsampler and pairs 0.94 | 0.97,
conv_pre at 384 inputs 0.13 | 0.14; gemmcu TC at u = 4: 192 x 256 0.84 | 0.84, 256 x 256 0.82 | 0.86; the padded stage on reschain_f16_c32 0.86 |
0.70 and respair_f16_c32 0.86 | 0.69; conv_post (MFMA, padded rows) 0.006 | 0.007.  fp32 / bf16x3 / bf16 -- the tap-GEMM at 0.0001 - 0.054 of E (the
bounds are linear in K, a correct kernel's error grows like sqrt(K)), conv_post_kernel at C = 16 0.013 | 0.015: these catch a wrong row, tap, phase,
crop or slope (tests/test_vocoder_ref.py emulates each for (5, 11) and (4, 8)), not a mistake of a few ulp."""
import pytest
import torch

from tests import tapgemm_checks as TG
from tests import vocoder_checks as VO
from tests.cases import SWITCH, U5_LIN, _arch_c16, _arch_pre384, _arch_u4, _arch_u5, _config, _mel, _tc_batch, _tc_pick, fp16_inputs, unit_arch
from tests.harness import RatioSummary

pytestmark = pytest.mark.gpu

SUMMARY = RatioSummary()                              # this file's figures, by group: each test names its group before it runs

# max err / E per group and kernel as measured on MI355X by test_zz_summary_of_ratios (records, not limits): (seam + edge rows, the rest)
RECORD = {
    "16 channels bf16 | conv_post_kernel C=16": (0.0116, 0.0126),
    "16 channels bf16 | tapgemm_bf16_128x32": (0.0268, 0.037),
    "16 channels bf16 | tapgemm_bf16_256x32": (0.0326, 0.0329),
    "16 channels bf16x3 | conv_post_kernel C=16": (0.0121, 0.0101),
    "16 channels bf16x3 | tapgemm_bf16x3_128x32": (0.0094, 0.0132),
    "16 channels bf16x3 | tapgemm_bf16x3_256x32": (0.0121, 0.0152),
    "16 channels fp16 SI_VOC_FUSE=0 | conv_post": (0.0039, 0.0053),
    "16 channels fp16 SI_VOC_FUSE=0 | tapgemm_f16_*": (0.89, 0.96),
    "16 channels fp16 | conv_post": (0.0055, 0.007),
    "16 channels fp16 | reschain_f16_c32": (0.72, 0.67),
    "16 channels fp16 | reschain_f16_c32_acc": (0.86, 0.63),
    "16 channels fp16 | respair_f16_c32": (0.86, 0.69),
    "16 channels fp16 | respair_f16_c32_acc": (0.86, 0.61),
    "16 channels fp16 | tapgemm_f16_*": (0.94, 0.97),
    "16 channels fp32 | conv_post_kernel C=16": (0.0103, 0.0112),
    "16 channels fp32 | tapgemm_f32_128x32": (0.0419, 0.0426),
    "16 channels fp32 | tapgemm_f32_256x32": (0.0446, 0.0537),
    "conv_pre 384 bf16 | tapgemm_bf16_128x128": (0.0002, 0.0003),
    "conv_pre 384 bf16 | tapgemm_bf16_128x64": (0.0053, 0.0059),
    "conv_pre 384 bf16 | tapgemm_bf16_256x128w8": (0.0002, 0.0002),
    "conv_pre 384 bf16 | tapgemm_bf16_256x64": (0.007, 0.0068),
    "conv_pre 384 bf16x3 | tapgemm_bf16x3_128x128": (0.0001, 0.0002),
    "conv_pre 384 bf16x3 | tapgemm_bf16x3_128x64": (0.0017, 0.0026),
    "conv_pre 384 bf16x3 | tapgemm_bf16x3_256x128w8": (0.0001, 0.0002),
    "conv_pre 384 bf16x3 | tapgemm_bf16x3_256x64": (0.0023, 0.0034),
    "conv_pre 384 fp16 | tapgemm_f16_*": (0.13, 0.14),
    "conv_pre 384 fp32 | tapgemm_f32_128x128": (0.0008, 0.001),
    "conv_pre 384 fp32 | tapgemm_f32_128x64": (0.0124, 0.0137),
    "conv_pre 384 fp32 | tapgemm_f32_256x128w8": (0.0006, 0.0009),
    "conv_pre 384 fp32 | tapgemm_f32_256x64": (0.0115, 0.0157),
    "u=4 k=8 bf16 | tapgemm_bf16_128x128": (0.003, 0.0046),
    "u=4 k=8 bf16 | tapgemm_bf16_256x128w8": (0.0025, 0.0049),
    "u=4 k=8 bf16 | tapgemm_bf16_256x64": (0.0045, 0.0059),
    "u=4 k=8 bf16x3 | tapgemm_bf16x3_128x128": (0.0016, 0.0025),
    "u=4 k=8 bf16x3 | tapgemm_bf16x3_256x128w8": (0.0015, 0.002),
    "u=4 k=8 bf16x3 | tapgemm_bf16x3_256x64": (0.0022, 0.0033),
    "u=4 k=8 fp16 | gemmcu_f16_192x256": (0.84, 0.84),
    "u=4 k=8 fp16 | gemmcu_f16_256x256": (0.82, 0.86),
    "u=4 k=8 fp16 | tapgemm_f16_*": (0.8, 0.83),
    "u=4 k=8 fp32 | tapgemm_f32_128x128": (0.0088, 0.0124),
    "u=4 k=8 fp32 | tapgemm_f32_256x128w8": (0.0059, 0.0102),
    "u=4 k=8 fp32 | tapgemm_f32_256x64": (0.0159, 0.0165),
    "u=5 k=11 bf16 | conv_post_kernel C=32": (0.0054, 0.0093),
    "u=5 k=11 bf16 | tapgemm_bf16_128x128": (0.0031, 0.0048),
    "u=5 k=11 bf16 | tapgemm_bf16_128x32": (0.0106, 0.0071),
    "u=5 k=11 bf16 | tapgemm_bf16_128x64": (0.0005, 0.0006),
    "u=5 k=11 bf16 | tapgemm_bf16_256x128w8": (0.0036, 0.0045),
    "u=5 k=11 bf16 | tapgemm_bf16_256x32": (0.0109, 0.0128),
    "u=5 k=11 bf16 | tapgemm_bf16_256x64": (0.0004, 0.0006),
    "u=5 k=11 bf16x3 | conv_post_kernel C=32": (0.0064, 0.0114),
    "u=5 k=11 bf16x3 | tapgemm_bf16x3_128x128": (0.0019, 0.0021),
    "u=5 k=11 bf16x3 | tapgemm_bf16x3_128x32": (0.0042, 0.0045),
    "u=5 k=11 bf16x3 | tapgemm_bf16x3_128x64": (0.0003, 0.0004),
    "u=5 k=11 bf16x3 | tapgemm_bf16x3_256x128w8": (0.0017, 0.0021),
    "u=5 k=11 bf16x3 | tapgemm_bf16x3_256x32": (0.0068, 0.0064),
    "u=5 k=11 bf16x3 | tapgemm_bf16x3_256x64": (0.0003, 0.0004),
    "u=5 k=11 fp16 | respair_f16_c128": (0.23, 0.18),
    "u=5 k=11 fp16 | respair_f16_c256": (0.17, 0.08),
    "u=5 k=11 fp16 | respair_f16_c32": (0.51, 0.56),
    "u=5 k=11 fp16 | tapgemm_f16_*": (0.89, 0.9),
    "u=5 k=11 fp32 | conv_post_kernel C=32": (0.0069, 0.0097),
    "u=5 k=11 fp32 | tapgemm_f32_128x128": (0.0114, 0.0154),
    "u=5 k=11 fp32 | tapgemm_f32_128x32": (0.0293, 0.019),
    "u=5 k=11 fp32 | tapgemm_f32_128x64": (0.0018, 0.0025),
    "u=5 k=11 fp32 | tapgemm_f32_256x128w8": (0.0102, 0.0166),
    "u=5 k=11 fp32 | tapgemm_f32_256x32": (0.0305, 0.0376),
    "u=5 k=11 fp32 | tapgemm_f32_256x64": (0.0017, 0.0021),
    "unit vocoder bf16x3 | conv_post_kernel C=16": (0.0122, 0.0143),
    "unit vocoder bf16x3 | tapgemm_bf16x3_128x128": (0.0017, 0.002),
    "unit vocoder bf16x3 | tapgemm_bf16x3_256x32": (0.0095, 0.0127),
    "unit vocoder bf16x3 | tapgemm_bf16x3_256x64": (0.0025, 0.0041),
    "unit vocoder fp16 | conv_post": (0.003, 0.0051),
    "unit vocoder fp16 | gemmcu_f16_192x256": (0.76, 0.81),
    "unit vocoder fp16 | reschain_f16_c32": (0.66, 0.7),
    "unit vocoder fp16 | reschain_f16_c32_acc": (0.59, 0.6),
    "unit vocoder fp16 | respair_f16_c128": (0.24, 0.22),
    "unit vocoder fp16 | respair_f16_c128_acc": (0.13, 0.06),
    "unit vocoder fp16 | respair_f16_c256": (0.15, 0.07),
    "unit vocoder fp16 | respair_f16_c256_acc": (0.17, 0.0),
    "unit vocoder fp16 | respair_f16_c64": (0.41, 0.37),
    "unit vocoder fp16 | respair_f16_c64_acc": (0.27, 0.22),
    "unit vocoder fp16 | tapgemm_f16_*": (0.92, 0.97),
    "unit vocoder fp16 | upsample_f16_c64": (0.84, 0.92),
}


def _inputs(prefix):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [c for c in fp16_inputs(cus) if c[0].startswith(prefix)]


def _eng16(varch, **env):
    """An fp16 engine per (architecture, knobs), kept for the session."""
    return VO._engine(varch, env, key=("unitvoc", repr(varch), tuple(sorted(env.items()))))


def _mel_of(case):
    tag, varch, seed, lens, Tm, clips = case
    if lens is None:
        one = _mel(1, Tm, seed, varch.num_mels)
        return torch.cat([one, one]).contiguous()
    return _mel(len(lens), max(lens), seed, varch.num_mels)


def _run16(case, eng, x2_eng=None, **kw):
    """One fp16 case: run, verify every produced tap of the clips the case checks; a uniform batch's two copies must be bit-equal."""
    tag, varch, seed, lens, Tm, clips = case
    mel = _mel_of(case)
    x2 = VO._run(x2_eng, varch, mel, lens) if x2_eng is not None else None
    taps, wave, prof = VO._run(eng, varch, mel, lens)
    VO._verify(varch, mel, lens, taps, wave, prof, tag + (f" L={Tm}" if lens is None else ""), summary=SUMMARY, clips=clips, x2_from=x2[0] if x2 else None, **kw)
    if lens is None:
        for k, t in taps.items():
            assert torch.equal(t[0], t[1]), f"{tag} L={Tm}: {k} differs between two copies of one clip"
        assert torch.equal(wave[0], wave[1])
    if x2 is not None:
        assert torch.equal(wave, x2[1]), f"{tag}: the chain run's samples differ from the pairs run's"
    return taps, wave, prof, x2


def _only_tapgemm_upsampler(prof):
    assert any(n.startswith("tapgemm_f16_") for n in prof), sorted(prof)
    assert not any(n.startswith(("gemmcu_f16_", "upsample_f16_")) for n in prof), sorted(prof)


# ------------------------------------------------------------------------------------------------------- 1. u = 5, k = 11
@pytest.mark.parametrize("C", [256, 32])
def test_u5_k11_upsampler_fp16_on_the_tap_gemm(C):
    """fp16 stream, 2 C -> C with u = 5, k = 11: only tapgemm_f16_* may serve the upsampler (three taps: neither gemmcu's TC kernels nor
    upsample.hip).  One ragged batch of Lin = 1, 2, 3, 126 .. 256 with the stage's k = 3 block behind it, and every Lin as a uniform batch."""
    SUMMARY.group = "u=5 k=11 fp16"
    eng = _eng16(_arch_u5(C), SI_VOC_CHAIN="0")             # (pair by pair: at C = 32 the chain kernel would keep x_1, x_2 to itself)
    for case in _inputs(f"u5 C={C} "):
        prof = _run16(case, eng, ops=("pre", "ups", "rb") if case[3] is not None else ("ups",))[2]
        _only_tapgemm_upsampler(prof)


@pytest.mark.parametrize("L", U5_LIN)
@pytest.mark.parametrize("C", [256, 32])
@pytest.mark.parametrize("mode", list(TG.MODES))
def test_u5_k11_upsampler_in_the_tapgemm_modes(mode, C, L):
    """fp32 / bf16x3 / bf16: every launch of the one-stage architecture at Lin = L; `_config(math, 5 C, Lin + 1, 3, -1, 2 C)` names the
    upsampler's launch and the profile holds exactly the names `_config` gives."""
    SUMMARY.group = f"u=5 k=11 {mode}"
    cfgs, _, _ = TG._uniform(_arch_u5(C), mode, L, 2100 + C + L, f"{mode} u=5 k=11 C={C}", summary=SUMMARY)
    assert _config(TG.MODES[mode][1], 5 * C, L + 1, 3, -1, 2 * C)[0] in cfgs


@pytest.mark.parametrize("mode", list(TG.MODES))
def test_u5_k11_ragged_in_the_tapgemm_modes(mode):
    SUMMARY.group = f"u=5 k=11 {mode}"
    varch = _arch_u5(32)
    lens = [257, 1, 128, 3, 127, 2]
    mel = _mel(len(lens), max(lens), 2200)
    taps, wave, prof = TG._run(TG._engine(varch, mode), varch, mel, lens)
    TG._verify(varch, mode, mel, lens, taps, prof, f"{mode} u=5 k=11 ragged", summary=SUMMARY, wave=wave)


# ------------------------------------------------------------------------------------------------------- 2. u = 4, k = 8
@pytest.mark.parametrize("C", [128, 64])
def test_u4_k8_on_gemmcu_tc_at_both_tile_heights(C):
    """gemmcu.hip's TC kernels at N = 4 C = 512 / 256: Lin + 1 = BM - 1, BM, BM + 1 for BM = 192 and 256 and Lin = 1, ragged and uniform (few
    tiles: 192 x 256); a batch chosen by the cost rule for 256 x 256 (`_tc_batch`; its clips at M - 1, M, M + 1 rows); conv_pre's tap carries the
    activated value (checked by its own reference with out_slope 0.1); with SI_VOC_UPSGEMM=0 the tap-GEMM meets the same reference."""
    SUMMARY.group = "u=4 k=8 fp16"
    varch = _arch_u4(C)
    eng = _eng16(varch)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    seen = set()
    for case in _inputs(f"u4 C={C} "):
        tag, _, _, lens, Tm, _ = case
        if tag.endswith("tap-GEMM"):
            prof = _run16(case, _eng16(varch, SI_VOC_UPSGEMM="0"), ops=("pre", "ups"), upsgemm=False)[2]
            _only_tapgemm_upsampler(prof)
            continue
        prof = _run16(case, eng, ops=("pre", "ups"))[2]
        tc = {n for n in prof if n.startswith("gemmcu_f16_")}
        ms = [l + 1 for l in lens] if lens is not None else [Tm + 1] * 2
        assert tc == {f"gemmcu_f16_{_tc_pick(ms, 4 * C, cus)}x256"}, (tag, sorted(prof), ms)
        seen |= tc
    assert _tc_batch(4 * C, cus) is not None, f"no batch of 32 clips reaches 256 x 256 at N = {4 * C} on {cus} CUs"
    assert seen == {"gemmcu_f16_192x256", "gemmcu_f16_256x256"}, sorted(seen)


@pytest.mark.parametrize("L", [m - 1 for m in SWITCH])
@pytest.mark.parametrize("C", [128, 64])
@pytest.mark.parametrize("mode", list(TG.MODES))
def test_u4_k8_upsampler_in_the_tapgemm_modes(mode, C, L):
    SUMMARY.group = f"u=4 k=8 {mode}"
    cfgs, _, _ = TG._uniform(_arch_u4(C), mode, L, 2300 + C + L, f"{mode} u=4 k=8 C={C}", summary=SUMMARY)
    assert _config(TG.MODES[mode][1], 4 * C, L + 1, 2, -1, 2 * C)[0] in cfgs


# ------------------------------------------------------------------------------------------------------- 3. the 16-channel stage
C16_CASES = [c[0] for c in fp16_inputs() if c[0].startswith("c16") and "tap-GEMM" not in c[0]]


@pytest.mark.parametrize("name", C16_CASES)
def test_c16_stage_fp16_padded_to_32(name):
    """The fp16 stream carries the 16-channel stage at 32: `ups0.f16` and every stage tap have 32 channels, channels 16..31 are exactly zero
    in every tap of every clip (vocoder_ref.real_channels), channels 0..15 meet the references at the real width.  Default knobs: the
    upsampler on tapgemm_f16_*, reschain_f16_c32[_acc], conv_post on the MFMA kernel; SI_VOC_CHAIN=0: respair_f16_c32[_acc], bit-equal to
    the chain run.  Rows: the C = 32 pair seams and the chain seams, conv_post's 511, 512, 513."""
    SUMMARY.group = "16 channels fp16"
    for case in [c for c in fp16_inputs() if c[0] == name]:
        varch = case[1]
        chain, pairs = _eng16(varch), _eng16(varch, SI_VOC_CHAIN="0")
        taps, wave, prof, x2 = _run16(case, chain, x2_eng=pairs)
        _only_tapgemm_upsampler(prof)
        assert "reschain_f16_c32" in prof and "reschain_f16_c32_acc" in prof and "conv_post" in prof and not any(n.startswith("respair") for n in prof), sorted(prof)
        assert "stage0.rb0.p0.f16" not in taps and taps["ups0.f16"].shape[2] == 32 and all(t.shape[2] == 32 for k, t in taps.items() if k != "pre.f16")
        ptaps, pwave, pprof = x2
        assert "respair_f16_c32" in pprof and "respair_f16_c32_acc" in pprof and not any(n.startswith("reschain") for n in pprof), sorted(pprof)
        mel = _mel_of(case)
        VO._verify(varch, mel, case[3], ptaps, pwave, pprof, case[0] + " pairs", summary=SUMMARY, clips=case[5])


@pytest.mark.parametrize("u", [2, 1])
def test_c16_stage_fp16_tap_gemm_pairs(u):
    """SI_VOC_FUSE=0: the padded stage's pairs as two tap-GEMM launches each, the same references and the same exact zeros."""
    SUMMARY.group = "16 channels fp16 SI_VOC_FUSE=0"
    varch = _arch_c16(u)
    for case in _inputs(f"c16 u={u} tap-GEMM"):
        prof = _run16(case, _eng16(varch, SI_VOC_FUSE="0"))[2]
        assert all(n.startswith("tapgemm_f16_") or n in ("conv_post", "extend_mel") for n in prof), sorted(prof)


C16_TG = [(2, L) for L in (63, 64, 65) + tuple(m - 1 for m in SWITCH)] + [(1, L) for L in SWITCH]


@pytest.mark.parametrize("u,L", C16_TG)
@pytest.mark.parametrize("mode", list(TG.MODES))
def test_c16_stage_in_the_tapgemm_modes(mode, u, L):
    """fp32 / bf16x3 / bf16: width 16 is real -- N = 16 inside a 32-column tile, Cin = 16 (BK = 16, ungrouped) -- every launch against
    tapgemm_ref, the names `_config` gives, conv_post_kernel at C = 16 (20-float LDS rows) against conv_post_ref(mfma=False).  u = 2: the
    upsampler's M = Lin + 1 at the switch rows and the stage at 126, 128, 130 rows; u = 1: the stage at the switch rows themselves."""
    SUMMARY.group = f"16 channels {mode}"
    math = TG.MODES[mode][1]
    cfgs, _, _ = TG._uniform(_arch_c16(u), mode, L, 2400 + 10 * u + L, f"{mode} 16 channels u={u}", summary=SUMMARY, post=True)
    k = 4 if u == 2 else 3
    assert cfgs == {_config(math, 32, L, 7, 1, 96)[0], _config(math, u * 16, L + 1, -(-k // u), -1, 32)[0], _config(math, 16, u * L, 3, 1, 16)[0]}
    assert _config(math, 16, u * L, 11, 5, 16)[0].endswith("x32")


# ------------------------------------------------------------------------------------------------------- 4. conv_pre at 384 inputs
def test_conv_pre_384_fp16():
    """conv_pre 384 -> 128 on the fp16 tap-GEMM (packed K = 7 x 384; its fp32 input is clamped and rounded while staging) at the switch rows."""
    SUMMARY.group = "conv_pre 384 fp16"
    eng = _eng16(_arch_pre384())
    for case in _inputs("pre384"):
        prof = _run16(case, eng, ops=("pre",))[2]
        assert any(n.startswith("tapgemm_f16_") for n in prof)


@pytest.mark.parametrize("L", SWITCH)
@pytest.mark.parametrize("mode", list(TG.MODES))
def test_conv_pre_384_in_the_tapgemm_modes(mode, L):
    SUMMARY.group = f"conv_pre 384 {mode}"
    cfgs, _, _ = TG._uniform(_arch_pre384(), mode, L, 2500 + L, f"{mode} 384 inputs", summary=SUMMARY)
    assert cfgs == TG._reached(mode, 64, L, num_mels=384) and _config(TG.MODES[mode][1], 128, L, 7, 1, 384)[0] in cfgs


# ------------------------------------------------------------------------------------------------------- 5. the whole unit vocoder
UNIT_FAMILIES = ("tapgemm_f16_", "gemmcu_f16_", "upsample_f16_c64", "respair_f16_c256", "respair_f16_c128_acc", "respair_f16_c64", "reschain_f16_c32", "conv_post")


def test_whole_unit_vocoder_fp16_every_tap():
    """The unit vocoder, B = 2 at 7 frames and a ragged batch [7, 1, 4]: every tap of every stage against its reference from the tapped
    input (x_2 of the chained stages from a SI_VOC_CHAIN=0 run).  ups0 (u = 5) runs on the tap-GEMM, so conv_pre stores the raw value; ups1
    and ups2 run on gemmcu's TC kernels (two launches per pass), so stage 0's last launch stores the activated value -- `_verify` checks it
    against pair_ref(out_slope = 0.1) -- and stage 1's does; ups3 on upsample_f16_c64; ups4 and the padded stage as in the 16-channel tests.
    The taps are inert, and each clip of the ragged batch equals that clip alone bit for bit."""
    SUMMARY.group = "unit vocoder fp16"
    varch = unit_arch()
    eng, pairs = _eng16(varch), _eng16(varch, SI_VOC_CHAIN="0")
    for case in _inputs("unit "):
        tag, _, _, lens, _, _ = case
        mel = _mel_of(case)
        _, plain, prof0 = VO._run(eng, varch, mel, lens, tapped=False)
        taps, wave, prof, _ = _run16(case, eng, x2_eng=pairs)
        assert torch.equal(wave, plain), f"{tag}: registering the taps changed the waveform"
        assert prof == prof0, (prof, prof0)
        for fam in UNIT_FAMILIES:
            assert any(n.startswith(fam) for n in prof), (fam, sorted(prof))
        assert sum(v for n, v in prof.items() if n.startswith("gemmcu_f16_")) == 2 and "upsample_f16_c128" not in prof, prof
        if lens is not None:
            for b, L in enumerate(lens):
                t1, w1, _ = VO._run(eng, varch, mel[b:b + 1, :, :L].contiguous())
                for k in t1:
                    assert torch.equal(t1[k][0], taps[k][b, :t1[k].shape[1]]), f"{tag} clip {b} (L = {L}): {k} differs from the clip alone"
                assert torch.equal(w1[0], wave[b, :w1.shape[1]]) and not bool(wave[b, w1.shape[1]:].any())


def test_whole_unit_vocoder_bf16x3_every_tap():
    """The same two batches in bf16x3 (real widths down to 16, conv_post_kernel at C = 16): every launch against tapgemm_ref, the names
    `_config` gives; taps inert; ragged = alone."""
    SUMMARY.group = "unit vocoder bf16x3"
    varch = unit_arch()
    eng = TG._engine(varch, "bf16x3")
    one = _mel(1, 7, 1600, 384)
    for mel, lens, tag in ((torch.cat([one, one]).contiguous(), None, "unit bf16x3 B=2"), (_mel(3, 7, 1601, 384), [7, 1, 4], "unit bf16x3 ragged")):
        _, plain, prof0 = TG._run(eng, varch, mel, lens, tapped=False)
        taps, wave, prof = TG._run(eng, varch, mel, lens)
        assert torch.equal(wave, plain) and prof == prof0, (tag, prof, prof0)
        TG._verify(varch, "bf16x3", mel, lens, taps, prof, tag, summary=SUMMARY, clips=[0] if lens is None else None, wave=wave)
        if lens is None:
            assert all(torch.equal(t[0], t[1]) for t in taps.values()) and torch.equal(wave[0], wave[1])
        else:
            for b, L in enumerate(lens):
                t1, w1, _ = TG._run(eng, varch, mel[b:b + 1, :, :L].contiguous())
                for k in t1:
                    assert torch.equal(t1[k][0], taps[k][b, :t1[k].shape[1]]), f"{tag} clip {b} (L = {L}): {k} differs from the clip alone"
                assert torch.equal(w1[0], wave[b, :w1.shape[1]]) and not bool(wave[b, w1.shape[1]:].any())


def test_zz_summary_of_ratios():
    """(last in the file) the largest err / E per group and kernel over every check above: near seams and clip edges | elsewhere."""
    SUMMARY.report()
