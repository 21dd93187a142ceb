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
import os
import re

import pytest
import torch

from tests import vocoder_ref as V

pytestmark = pytest.mark.gpu

torch.set_num_threads(16)
R1 = {32: 256, 64: 512, 128: 256, 256: 128}           # rows of a pair kernel's tile (see the module docstring)
V1_BLOCKS = dict(resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3)
SUMMARY = {}                                          # kernel -> [max err / E near seams and edges, max elsewhere, checks]


def _arch(C, u=1, k=3, num_mels=80, **kw):
    """One stage of C channels behind an upsampler (u, k).  C = 256 gets a second u = 1 stage of 128 channels behind it: conv_post_kernel
    keeps 262 rows of C + 4 floats in LDS and refuses 256 channels (no generator ends that wide).  num_mels: conv_pre's input width
    (80 mel bins; the unit vocoder's 384 embedding channels)."""
    from speech_inpainting_amd.arch import VocoderArch
    blocks = dict(V1_BLOCKS)
    blocks.update(kw)
    us, ks = ((u, 1), (k, 3)) if C == 256 else ((u,), (k,))
    return VocoderArch(upsample_rates=us, upsample_kernel_sizes=ks, upsample_initial_channel=2 * C, num_mels=num_mels, **blocks)


def _padded(C):
    """The width the fp16 stream carries a stage of C channels at (api.hip, stage_channels: 4 <= C < 32 is padded to 32 with zero weights)."""
    return 32 if 4 <= C < 32 else C


_STATE = {}
_FOLDED = {}


def _key(varch):
    return repr(varch)


def _state(varch):
    from speech_inpainting_amd import synth
    if _key(varch) not in _STATE:
        _STATE[_key(varch)] = synth.synth_generator_state(varch, 47)
    return _STATE[_key(varch)]


def _w(varch, name):
    """The kernel's fp16 weight of a module, as float64 (vocoder_ref.fold: the packer's fold, rounded once)."""
    if (_key(varch), name) not in _FOLDED:
        _FOLDED[(_key(varch), name)] = V.fold(_state(varch), name)
    return _FOLDED[(_key(varch), name)]


def _engine(varch, env=None):
    """fp16 vocoder; `env` knobs (SI_VOC_FUSE, SI_VOC_CHAIN, SI_VOC_UPSGEMM) are read when the context is created."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch
    from speech_inpainting_amd.engine import InpaintingEngine
    harch = HubertArch.tiny()
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = InpaintingEngine(harch, varch, 20, "cuda:0", "fp32", "fp16")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return eng.load_state(synth.synth_hubert_state(harch), _state(varch), synth.synth_codebook(20))


def _shapes(varch, B, Tm):
    """{tap name: (B, rows, channels)} of every tap the architecture can produce at Tm frames (stretch off); a stage's taps have the
    width the stream carries it at (`_padded`)."""
    C, L = varch.upsample_initial_channel, Tm
    out = {"pre.f16": (B, L, C)}
    for i, u in enumerate(varch.upsample_rates):
        C, L = C // 2, L * u
        out[f"ups{i}.f16"] = out[f"stage{i}.f16"] = (B, L, _padded(C))
        for j, dil in enumerate(varch.resblock_dilation_sizes):
            for n in range(len(dil)):
                out[f"stage{i}.rb{j}.p{n}.f16"] = (B, L, _padded(C))
    return out


def _run(eng, varch, mel, lens=None, tapped=True):
    """One generator pass -> (taps {name: (B, rows, C) cpu fp16} of the taps the path produced, wave cpu, {kernel: launches})."""
    B, _, Tm = mel.shape
    shapes = _shapes(varch, B, Tm)
    eng.ctx.clear_captures()
    caps = eng.ctx.capture(list(shapes), capacity={k: s[0] * s[1] * s[2] for k, s in shapes.items()}) if tapped else {}
    eng.ctx.profile_start(4000)
    wave = eng.vocode_ragged(mel.cuda(), lens, stretch=False) if lens is not None else eng.vocode(mel.cuda(), stretch=False)
    prof = {e["name"]: e["launches"] for e in eng.ctx.profile_stop()}
    torch.cuda.synchronize()
    taps = {}
    for k, t in caps.items():
        assert t.dtype == torch.float16
        if eng.ctx.lib.si_debug_size(eng.ctx._h, k.encode()) == t.numel():
            taps[k] = t.cpu().view(shapes[k])
    eng.ctx.clear_captures()
    return taps, wave.cpu(), prof


def _kernel(prof, *patterns):
    """The one profiled kernel family matching any of the patterns; asserts that it ran."""
    hit = sorted(n for n in prof if any(re.fullmatch(p, n) for p in patterns))
    assert hit, (patterns, sorted(prof))
    return "+".join(hit)


def _note(kernel, near, rest):
    kernel = "tapgemm_f16_*" if kernel.startswith("tapgemm") else kernel          # (its tile shapes follow the layer: one line for the family)
    s = SUMMARY.setdefault(kernel, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], near), max(s[1], rest), s[2] + 1


def _one(tag, kernel, clip, got, ref, E, stored, halo, hot, f32=False):
    L = ref.shape[0]
    if not hot:                                            # the case is built to stay far from saturation: only then is every element an ordinary check
        assert float(ref.abs().max()) < V.F16_MAX / 4, (tag, float(ref.abs().max()))
    r = (V.check_f32 if f32 else V.check_f16)(got.reshape(ref.shape), ref, E)
    line, near, rest = V.report(tag, kernel, clip, r, L, stored, halo)
    print("   " + line)
    assert r["finite"] and r["bad"] == 0, line
    _note(kernel, near, rest)
    return r


def _verify(varch, mel, lens, taps, wave, prof, tag, ops=("pre", "ups", "rb", "post"), clips=None, hot=False, x2_from=None, upsgemm=True):
    """Every produced tap of every clip against its reference from the tapped input.  x2_from: the taps of a run of the SAME input with
    the pairs one by one (SI_VOC_CHAIN=0), which supply the x_2 a reschain.hip launch keeps to itself."""
    sd = _state(varch)
    B, _, Tm = mel.shape
    nk = len(varch.resblock_kernel_sizes)
    two = str(varch.resblock) == "2"
    # stored activated: the producer of an upsampler that ran in gemmcu's TC kernels (include/si_hip.h); all candidates or none
    cand = [i for i, (u, k) in enumerate(zip(varch.upsample_rates, varch.upsample_kernel_sizes))
            if -(-k // u) == 2 and (u * (varch.upsample_initial_channel >> (i + 1))) % 256 == 0 and (varch.upsample_initial_channel >> i) % 64 == 0]
    n_tc = sum(v for k, v in prof.items() if k.startswith("gemmcu_f16_"))
    assert n_tc in (0, len(cand)), (n_tc, cand, prof)
    on_tc = set(cand) if n_tc else set()
    assert upsgemm or not on_tc
    def real(name, b, L, C):
        """Rows :L of clip b of a stage tap as the C real channels; the channels the stream pads the stage with must hold exact zeros."""
        t = taps[name][b, :L]
        assert t.shape[1] == _padded(C), (name, t.shape, C)
        return V.real_channels(t, C, f"{tag} {name} clip {b}")

    for b in (range(B) if clips is None else clips):
        L = int(lens[b]) if lens is not None else Tm
        x = taps["pre.f16"][b, :L]
        if "pre" in ops:
            a = V.h16(mel[b, :, :L].t().clamp(-V.F16_MAX, V.F16_MAX))
            ref, E = V.tapconv_ref(a, _w(varch, "conv_pre"), sd["conv_pre.bias"], out_slope=V.SLOPE32 if 0 in on_tc else 1.0)
            _one(f"{tag} conv_pre", _kernel(prof, r"tapgemm_f16_.*"), b, x, ref, E, None, 3, hot)
        C = varch.upsample_initial_channel
        for i, (u, k) in enumerate(zip(varch.upsample_rates, varch.upsample_kernel_sizes)):
            staged = x.double() if i in on_tc else V.lrelu16(x).double()
            Lo, C = L * u, C // 2
            U16 = real(f"ups{i}.f16", b, Lo, C)
            Cp = _padded(C)                                        # the kernels' width: names and tile heights follow it, the references C
            if "ups" in ops:
                ref, E = V.upsample_ref(staged, _w(varch, f"ups.{i}"), sd[f"ups.{i}.bias"], u)
                if i in on_tc:
                    kern = _kernel(prof, r"gemmcu_f16_.*")
                    rows = int(re.search(r"gemmcu_f16_(\d+)x", kern).group(1)) * u           # BM GEMM rows = BM u output rows per tile
                elif u == 2 and k == 4 and 2 * C in (128, 64) and f"upsample_f16_c{2 * C}" in prof:
                    kern, rows = f"upsample_f16_c{2 * C}", 256 * u
                else:
                    kern, rows = _kernel(prof, r"tapgemm_f16_.*"), None
                _one(f"{tag} ups{i} {2 * C}->{C} u={u}", kern, b, U16, ref, E, rows, k, hot)
            L = Lo
            act_next = (i + 1) in on_tc
            xs_prev = None
            for j, (rk, dils) in enumerate(zip(varch.resblock_kernel_sizes, varch.resblock_dilation_sizes)):
                r = f"resblocks.{i * nk + j}."
                xin = U16
                last_n = len(dils) - 1
                for n, d in enumerate(dils):
                    name = f"stage{i}.rb{j}.p{n}.f16"
                    last = n == last_n
                    chained = name not in taps or (last and f"stage{i}.rb{j}.p0.f16" not in taps and last_n > 0)
                    if name not in taps:                               # inside a reschain.hip launch: x_n from the pairs run
                        assert x2_from is not None and not last, (name, sorted(taps))
                        xin = x2_from[name][b, :L, :C]
                        continue
                    out = real(name, b, L, C)
                    if "rb" in ops:
                        alpha = V.alpha32(nk) if last else 1.0
                        prev = xs_prev.double() if (last and j > 0) else None
                        os_ = V.SLOPE32 if (last and j == nk - 1 and act_next) else 1.0
                        a = V.lrelu16(xin).double()
                        if two:
                            ref, E = V.rb2_ref(a, xin.double(), _w(varch, f"{r}convs.{n}"), sd[f"{r}convs.{n}.bias"], d, alpha, prev, os_)
                            kern, stored, halo = _kernel(prof, r"tapgemm_f16_.*"), None, (rk - 1) * d
                        else:
                            ref, E = V.pair_ref(a, xin.double(), _w(varch, f"{r}convs1.{n}"), sd[f"{r}convs1.{n}.bias"],
                                                _w(varch, f"{r}convs2.{n}"), sd[f"{r}convs2.{n}.bias"], d, alpha, prev, os_)
                            halo = (rk - 1) * (d + 1)
                            acc = "_acc" if (last and j > 0) else ""
                            if chained:
                                kern, stored = f"reschain_f16_c{Cp}{acc}", 768 - (rk - 1) * (sum(dils) + 3)
                                assert torch.equal(taps[name][b, :L], x2_from[name][b, :L]), f"{tag} {name}: the chain kernel and the pair kernels differ"
                            elif f"respair_f16_c{Cp}{acc}" in prof:
                                kern, stored = f"respair_f16_c{Cp}{acc}", R1[Cp] - (rk - 1)
                            else:
                                kern, stored = _kernel(prof, r"tapgemm_f16_.*"), None
                            assert kern.startswith("tapgemm") or kern in prof, (kern, sorted(prof))
                        _one(f"{tag} {name} k={rk} d={d}" + (" acc" if prev is not None else "") + (" act" if os_ != 1.0 else ""),
                             kern, b, out, ref, E, stored, halo, hot)
                    xin = out
                xs_prev = xin
            assert torch.equal(real(f"stage{i}.f16", b, L, C), xs_prev), f"{tag} stage{i}.f16 is not the last resblock's running sum"
            x = xs_prev
        if "post" in ops:
            ref, E = V.conv_post_ref(x, V.fold(sd, "conv_post", round16=False).float(), sd["conv_post.bias"], mfma=(_padded(C) == 32))
            _one(f"{tag} conv_post C={C}", _kernel(prof, "conv_post"), b, wave[b, :L], ref, E, 512 if _padded(C) == 32 else 256, 3, True, f32=True)
            assert not bool(wave[b, L:].any()), f"{tag}: samples past clip {b}'s end are not silence"


def _mel(B, Tm, seed, num_mels=80):
    """The generator's input: a synthetic log-mel at 80 bins; at any other width (the unit vocoder's 384 channels of concatenated
    embeddings) N(0, 0.5^2), as test_ida_style_generator_geometry_matches_oracle draws it."""
    from speech_inpainting_amd import synth
    if num_mels == 80:
        return synth.synth_mel(B, Tm, 80, seed)
    return torch.randn(B, num_mels, Tm, generator=torch.Generator().manual_seed(seed)) * 0.5


def _ragged(eng, varch, lengths, seed, tag, **kw):
    if isinstance(lengths, list):
        lens = lengths                                     # (a list: the batch as given)
    else:
        lengths = sorted(set(int(v) for v in lengths if v >= 1))
        lens = lengths[::2] + lengths[1::2][::-1]          # long and short clips interleaved: workgroups get different tile counts
    assert len(lens) <= 32
    mel = _mel(len(lens), max(lens), seed, varch.num_mels)
    taps, wave, prof = _run(eng, varch, mel, lens)
    _verify(varch, mel, lens, taps, wave, prof, f"{tag} ragged", **kw)
    return prof


def _uniform(eng, varch, L, seed, tag, **kw):
    one = _mel(1, L, seed, varch.num_mels)
    mel = torch.cat([one, one]).contiguous()
    taps, wave, prof = _run(eng, varch, mel)
    _verify(varch, mel, None, taps, wave, prof, f"{tag} uniform L={L}", clips=[0], **kw)
    for k, t in taps.items():
        assert torch.equal(t[0], t[1]), f"{tag} uniform L={L}: {k} differs between two copies of one clip"
    assert torch.equal(wave[0], wave[1])
    return prof


def _pair_lengths(C, ks=(3, 7, 11), dils=(1, 3, 5)):
    out = {1, 2, R1[C], R1[C] + 1}
    for k in ks:
        st = R1[C] - (k - 1)
        out |= {k - 1, st - 1, st, st + 1, 2 * st + 1} | {(k - 1) * d for d in dils}
    return out


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
    for k in sorted(SUMMARY):
        s = SUMMARY[k]
        print(f"   SUMMARY {k}: max err/E seam+edge rows {s[0]:.3f}, interior {s[1]:.3f} over {s[2]} checks")
        assert s[0] <= 1.0 and s[1] <= 1.0
