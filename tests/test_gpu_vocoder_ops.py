"""Each kernel of the fp16 vocoder (the fp16 activation stream bench.py times) against a float64 reference of its own operation
(tests/vocoder_ref.py) on the operands the kernel itself read, captured through the ".f16" taps: the fused ResBlock-pair kernels
(respair.hip C = 32 / 64, respair_wide.hip C = 128 / 256), reschain.hip, upsample.hip, gemmcu.hip's fp16 TC upsamplers, both
conv_post kernels and the tap-GEMM's fp16 path as the fallback of all of them.

One-stage architectures (upsample_rates = (1,), kernel 3, upsample_initial_channel = 2 C; the launchers take u = 1) put ONE stage of
C channels at exactly Tm rows, so every row count around a tile seam is reachable: a pair kernel's tile stores R1 - (k - 1) rows (R1 = 256, 512, 256, 128
for C = 32, 64, 128, 256: respair.hip's respair_launch<32, 256, ..> / <64, 512, ..>, respair_wide.hip's <128, 256, ..> / <256, 128, ..>),
reschain.hip's 768 - (k - 1)(d0 + d1 + d2 + 3) (RC_R and H in si_launch_reschain), upsample.hip's UP_RT = 256 GEMM rows, gemmcu's TC
instantiations 256 / 192 rows, conv_post_mfma_kernel's CPM_ROWS = 512.  Every assertion is |got - ref| <= E over ALL real rows and
channels of a clip, E being the derived bound of vocoder_ref.py; the line printed per check gives max err / E over the rows within
the kernel's reach of a tile seam or clip edge and over the rest, and on a failure op, kernel, clip, row, channel and distances.
Uniform batches hold the same clip twice: clip 0 is checked against the reference and clip 1, whose tiles other workgroups
compute, must equal clip 0 bit for bit.

Measured on MI355X (max err / E, rows near a seam or clip edge | the rest): respair C = 32 0.86 | 0.53, C = 64 0.81 | 0.42, C = 128 0.66 |
0.21, C = 256 0.43 | 0.08; reschain 0.76 | 0.64; upsample.hip 0.91 | 0.94; gemmcu TC 192 x 256 0.66 | 0.72, 256 x 256 0.47 | 0.46; tap-GEMM
0.94 | 0.96; conv_post 0.004 | 0.005.  The fp16 tensors' bounds are led by the store's half ulp wherever K is small, so one ulp more is a
failure there.  Two are loose: conv_post's (fp32 output, worst-case growth of 225 additions) and the pair bound at C = 256, k = 11 (0.006 -
0.008 on whole V1 clips: the worst-case passage of t's rounding through 2816 products): they catch a wrong row, tap, slope or operand
order, not a one-ulp mistake.  A packed leaky-ReLU computed in fp32 and rounded once instead (one ulp on some negative operands, a
tenth of the activations' size) stays under the pair bound (0.72 against 0.71 at C = 64); the bit-equality of reschain.hip with the pair
kernels is what notices it."""
import re

import pytest
import torch

from tests import vocoder_ref as V
from tests.cases import R1, _arch, _mel, _pair_lengths
from tests.harness import RatioSummary
from tests.vocoder_checks import _engine, _run
from tests.vocoder_checks import _ragged as _ragged_into
from tests.vocoder_checks import _uniform as _uniform_into
from tests.vocoder_checks import _verify as _verify_into

pytestmark = pytest.mark.gpu

SUMMARY = RatioSummary(digits=3)                      # this file's max err / E per kernel


def _verify(*args, summary=SUMMARY, **kw):
    return _verify_into(*args, summary=summary, **kw)


def _ragged(*args, summary=SUMMARY, **kw):
    return _ragged_into(*args, summary=summary, **kw)


def _uniform(*args, summary=SUMMARY, **kw):
    return _uniform_into(*args, summary=summary, **kw)


@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_pair_kernels_at_every_tile_seam(C):
    """respair.hip / respair_wide.hip, the three V1 blocks (k = 3, 7, 11 x dilation 1, 3, 5, up to (k - 1) d = 50; alpha 1 and 1/3, accumulate
    off and on): clips of 1, 2, k - 1, (k - 1) d, stored - 1, stored, stored + 1, 2 stored + 1, R1, R1 + 1 rows for every k in one ragged
    batch, and the k = 7 set again as uniform batches.  Also conv_post at this width (C = 32: the MFMA kernel at 1, 3, 511, 512, 513, 1025)."""
    varch = _arch(C)
    eng = _engine(varch, {"SI_VOC_CHAIN": "0"})
    extra = {3, 511, 512, 513, 1025} if C == 32 else set()
    prof = _ragged(eng, varch, _pair_lengths(C) | extra, 100 + C, f"C={C}")
    for fam in (f"respair_f16_c{C}", f"respair_f16_c{C}_acc", "conv_post"):
        assert fam in prof, (fam, sorted(prof))
    assert not any(n.startswith("reschain") for n in prof)
    st = R1[C] - 6
    for L in sorted({1, 2, 6, 30, st - 1, st, st + 1, 2 * st + 1, R1[C], R1[C] + 1}):
        _uniform(eng, varch, L, 200 + C, f"C={C}", ops=("rb", "post"))


def test_single_block_pairs_alpha_one():
    """A generator with ONE resblock per stage: the last pair runs with alpha = 1 and never accumulates (k = 11, the widest reach)."""
    for C in (64, 128):
        varch = _arch(C, resblock_kernel_sizes=(11,), resblock_dilation_sizes=((1, 3, 5),))
        eng = _engine(varch, {"SI_VOC_CHAIN": "0"})
        prof = _ragged(eng, varch, _pair_lengths(C, ks=(11,)), 300 + C, f"C={C} one block", ops=("rb", "post"))
        assert f"respair_f16_c{C}" in prof and f"respair_f16_c{C}_acc" not in prof


def test_reschain_at_its_tile_seams_and_equal_to_the_pairs():
    """reschain.hip (C = 32; a tile stores 768 - (k - 1)(1 + 3 + 5 + 3) = 744 / 696 / 648 rows for k = 3 / 7 / 11): its output against
    pair_ref on the x_2 tapped from the pairs' run of the same input, and equal to the pairs' output bit for bit."""
    varch = _arch(32)
    lengths = {1, 2, 768, 769}
    for k in (3, 7, 11):
        st = 768 - 12 * (k - 1)
        lengths |= {k - 1, 5 * (k - 1), st - 1, st, st + 1, 2 * st + 1}
    lengths = sorted(lengths)
    lens = lengths[::2] + lengths[1::2][::-1]
    mel = _mel(len(lens), max(lens), 77)
    pairs = _run(_engine(varch, {"SI_VOC_CHAIN": "0"}), varch, mel, lens)
    taps, wave, prof = _run(_engine(varch), varch, mel, lens)
    assert "reschain_f16_c32" in prof and "reschain_f16_c32_acc" in prof and not any(n.startswith("respair") for n in prof), sorted(prof)
    assert "stage0.rb0.p0.f16" not in taps and "stage0.rb0.p2.f16" in taps
    _verify(varch, mel, lens, taps, wave, prof, "chain ragged", ops=("rb", "post"), x2_from=pairs[0])
    assert torch.equal(wave, pairs[1])
    one = _mel(1, 1489, 78)
    mel2 = torch.cat([one, one]).contiguous()
    p2 = _run(_engine(varch, {"SI_VOC_CHAIN": "0"}), varch, mel2)
    t2, w2, prof2 = _run(_engine(varch), varch, mel2)
    _verify(varch, mel2, None, t2, w2, prof2, "chain uniform L=1489", ops=("rb",), clips=[0], x2_from=p2[0])
    assert torch.equal(t2["stage0.f16"][0], t2["stage0.f16"][1]) and torch.equal(w2, p2[1])


@pytest.mark.parametrize("C0", [128, 64])
def test_streaming_upsampler_alone(C0):
    """upsample.hip (u = 2, k = 4, Cin = 128 / 64, 256 GEMM rows per tile) as the only upsampler: Lin = 1, 2, 255, 256, 257, 513; the first
    and last output rows of every clip depend on the zero rows outside it."""
    varch = _arch(C0 // 2, u=2, k=4, resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1, 3, 5),))
    eng = _engine(varch, {"SI_VOC_CHAIN": "0"})
    prof = _ragged(eng, varch, {1, 2, 255, 256, 257, 513}, 400 + C0, f"Cin={C0}", ops=("pre", "ups", "post"))
    assert f"upsample_f16_c{C0}" in prof, sorted(prof)
    for L in (1, 2, 255, 256, 257, 513):
        _uniform(eng, varch, L, 410 + C0, f"Cin={C0}", ops=("ups",))


@pytest.mark.parametrize("C0", [512, 256])
def test_gemmcu_tc_upsampler_at_its_tile_heights(C0):
    """gemmcu.hip's fp16 TC instantiations (u = 8, k = 16, 512 -> 256 and 256 -> 128; 256 and 192 rows per tile, M = Lin + 1 GEMM rows per
    clip): Lin + 1 = BM - 1, BM, BM + 1 for both heights, ragged and uniform.  conv_pre's tap carries the activation the kernel expects
    (out16_slope 0.1), checked by conv_pre's own reference."""
    varch = _arch(C0 // 2, u=8, k=16, resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1,),))
    eng = _engine(varch)
    lengths = {1, 190, 191, 192, 254, 255, 256}
    prof = _ragged(eng, varch, lengths, 500 + C0, f"Cin={C0}", ops=("pre", "ups"))
    assert any(n.startswith("gemmcu_f16_") for n in prof), sorted(prof)
    for L in (191, 255, 256):
        p = _uniform(eng, varch, L, 510 + C0, f"Cin={C0}", ops=("pre", "ups"))
        assert any(n.startswith("gemmcu_f16_") for n in p), sorted(p)
    if C0 == 512:
        # The launcher takes the height with fewer rounds of the chip x (BM + 256): few tiles run on 192 rows.  Sixteen clips of 256 GEMM
        # rows, one of 257 and one of 255 are 19 x 8 tiles of 256 rows (one round of 256 CUs) against 36 x 8 of 192 (two): the 256 x 256
        # instantiation at BM - 1, BM and BM + 1.  (256 -> 128 has N / 256 = 4 column tiles: no batch of one chunk of 32 clips gets there.)
        p = _ragged(eng, varch, [255] * 8 + [256, 254] + [255] * 8, 520, f"Cin={C0} 18 clips", ops=("pre", "ups"), clips=[0, 8, 9, 17])
        assert "gemmcu_f16_256x256" in p, sorted(p)
    off = _engine(varch, {"SI_VOC_UPSGEMM": "0"})
    p = _ragged(off, varch, {1, 191, 256}, 500 + C0, f"Cin={C0} tap-GEMM", ops=("pre", "ups"), upsgemm=False)
    assert not any(n.startswith("gemmcu_f16_") for n in p), sorted(p)


def test_tap_gemm_fallback_in_fp16_mode():
    """SI_VOC_FUSE=0, SI_VOC_UPSGEMM=0: every op on the tap-GEMM (two launches per pair, t stored as fp16 between them), the same
    references; its staging of a 16-bit input is the packed form too (tapgemm.hip:198).  And the v3 architecture's ResBlock2 loop."""
    from speech_inpainting_amd.arch import VocoderArch
    env = {"SI_VOC_FUSE": "0", "SI_VOC_UPSGEMM": "0"}
    varch = _arch(64)
    prof = _ragged(_engine(varch, env), varch, {1, 2, 10, 127, 128, 129, 300}, 600, "tap-GEMM C=64", upsgemm=False)
    assert all(n.startswith("tapgemm_f16_") or n in ("conv_post", "extend_mel") for n in prof), sorted(prof)
    assert not any(re.match("respair|reschain|upsample|gemmcu", n) for n in prof)
    varch = _arch(64, u=2, k=4)
    prof = _ragged(_engine(varch, env), varch, {1, 2, 129}, 601, "tap-GEMM u=2", ops=("pre", "ups"), upsgemm=False)
    assert not any(n.startswith("upsample") for n in prof), sorted(prof)
    v3 = VocoderArch.v3()
    mel = _mel(2, 5, 602)
    taps, wave, prof = _run(_engine(v3, {"SI_VOC_UPSGEMM": "0"}), v3, mel, [5, 2])
    _verify(v3, mel, [5, 2], taps, wave, prof, "v3 ResBlock2", upsgemm=False)


def test_full_v1_every_tap_and_taps_are_inert():
    """The V1 generator, B = 3, Tm = 57 and a ragged batch: every tap of every stage against its reference from the tapped input -- the
    real widths, the real accumulate order over the blocks, the real hand-offs (conv_pre and stage 0 store the gemmcu upsamplers' activated
    input).  And the taps are inert: with every tap registered the waveform, the profiled kernel names and their launch counts are
    those of a run without."""
    from speech_inpainting_amd.arch import VocoderArch
    varch = VocoderArch.v1()
    eng = _engine(varch)
    pairs_eng = _engine(varch, {"SI_VOC_CHAIN": "0"})
    for mel, lens, tag in ((_mel(3, 57, 700), None, "V1 B=3 Tm=57"), (_mel(3, 57, 701), [57, 1, 23], "V1 ragged")):
        _, plain, prof0 = _run(eng, varch, mel, lens, tapped=False)
        taps, wave, prof = _run(eng, varch, mel, lens)
        assert torch.equal(wave, plain), f"{tag}: registering the taps changed the waveform"
        assert prof == prof0, (prof, prof0)
        for fam in ("gemmcu_f16_", "upsample_f16_c128", "upsample_f16_c64", "respair_f16_c256", "respair_f16_c128_acc", "respair_f16_c64", "reschain_f16_c32", "conv_post"):
            assert any(n.startswith(fam) for n in prof), (fam, sorted(prof))
        x2 = _run(pairs_eng, varch, mel, lens)[0]
        _verify(varch, mel, lens, taps, wave, prof, tag, x2_from=x2)


def test_hot_input_saturates_exactly_where_it_must():
    """synth_mel * 3e4 drives the stream into fp16 overflow (as the sign checks of test_gpu_respair.py do): per op and per element, where
    |ref| - E > 65504 the stored value is exactly +-65504, where |ref| + E < 65504 the ordinary bound holds, in between either."""
    from speech_inpainting_amd.arch import VocoderArch
    varch = VocoderArch.v1()
    mel = _mel(2, 9, 79) * 3.0e4
    x2 = _run(_engine(varch, {"SI_VOC_CHAIN": "0"}), varch, mel)[0]
    taps, wave, prof = _run(_engine(varch), varch, mel)
    assert bool(torch.isfinite(wave).all())
    assert sum(int((t.abs() == V.F16_MAX).sum()) for t in taps.values()) > 0, "the input is not hot"
    _verify(varch, mel, None, taps, wave, prof, "hot V1", hot=True, x2_from=x2)


def test_zz_summary_of_ratios():
    """(last in the file) the largest err / E per kernel over every check above: near seams and clip edges | elsewhere."""
    SUMMARY.report()
