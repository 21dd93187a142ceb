"""The fp16 vocoder's tapped run and its check of every ".f16" tap against tests/vocoder_ref.py, for tests/test_gpu_vocoder_ops.py (the V1
widths) and tests/test_gpu_unitvoc_ops.py (the unit vocoder's geometry).  What is checked and why: test_gpu_vocoder_ops.py's docstring."""
import re

import torch

from tests import vocoder_ref as V
from tests.cases import R1, _interleave, _mel, _padded, _state, _w
from tests.harness import build_engine, tapped_run
from tests.shape_rules import holds


def _engine(varch, env=None, key=None):
    """fp16 vocoder; `env` knobs (SI_VOC_FUSE, SI_VOC_CHAIN, SI_VOC_UPSGEMM) are read when the context is created."""
    from speech_inpainting_amd.arch import HubertArch
    return build_engine(HubertArch.tiny(), varch, 20, "fp32", "fp16", env=env, state=(None, _state(varch), None), key=key)


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
    cap = {k: s[0] * s[1] * s[2] for k, s in shapes.items()} if tapped else {}
    taps, wave, prof = tapped_run(eng.ctx, cap, lambda: eng.vocode_ragged(mel.cuda(), lens, stretch=False) if lens is not None
                                  else eng.vocode(mel.cuda(), stretch=False))
    assert all(t.dtype == torch.float16 for t in taps.values())
    return {k: t.view(shapes[k]) for k, t in taps.items()}, wave.cpu(), prof


def _kernel(prof, *patterns):
    """The one profiled kernel family matching any of the patterns; asserts that it ran."""
    hit = sorted(n for n in prof if any(re.fullmatch(p, n) for p in patterns))
    assert hit, (patterns, sorted(prof))
    return "+".join(hit)


def _one(summary, tag, kernel, clip, got, ref, E, stored, halo, hot, f32=False):
    L = ref.shape[0]
    if not hot:                                            # the case is built to stay far from saturation: only then is every element an ordinary check
        assert float(ref.abs().max()) < V.F16_MAX / 4, (tag, float(ref.abs().max()))
    r = (V.check_f32 if f32 else V.check_f16)(got.reshape(ref.shape), ref, E)
    line, near, rest = V.report(tag, kernel, clip, r, L, stored, halo)
    print("   " + line)
    assert r["finite"] and r["bad"] == 0, line
    summary.note(kernel, near, rest)
    return r


def _verify(varch, mel, lens, taps, wave, prof, tag, summary, ops=("pre", "ups", "rb", "post"), clips=None, hot=False, x2_from=None, upsgemm=True,
            chain_equal=True):
    """Every produced tap of every clip against its reference from the tapped input, noted into `summary`.  x2_from: the taps of a run
    of the SAME input with the pairs one by one (SI_VOC_CHAIN=0), which supply the x_2 a reschain.hip launch keeps to itself.
    chain_equal: the chain's output must equal that run's bit for bit (False where the pair kernels do not cover the block and that run
    went through the tap-GEMM, whose sums are ordered differently: then the float64 bound alone holds the chain)."""
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
            _one(summary, f"{tag} conv_pre", _kernel(prof, r"tapgemm_f16_.*"), b, x, ref, E, None, 3, hot)
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
                _one(summary, f"{tag} ups{i} {2 * C}->{C} u={u}", kern, b, U16, ref, E, rows, k, hot)
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
                                assert not chain_equal or torch.equal(taps[name][b, :L], x2_from[name][b, :L]), f"{tag} {name}: the chain kernel and the pair kernels differ"
                            elif f"respair_f16_c{Cp}{acc}" in prof and holds("respair", dict(C=Cp, k=rk, d=d)):    # (per pair: a block may hold both)
                                kern, stored = f"respair_f16_c{Cp}{acc}", R1[Cp] - (rk - 1)
                            else:
                                kern, stored = _kernel(prof, r"tapgemm_f16_.*"), None
                            assert kern.startswith("tapgemm") or kern in prof, (kern, sorted(prof))
                        _one(summary, f"{tag} {name} k={rk} d={d}" + (" acc" if prev is not None else "") + (" act" if os_ != 1.0 else ""),
                             kern, b, out, ref, E, stored, halo, hot)
                    xin = out
                xs_prev = xin
            assert torch.equal(real(f"stage{i}.f16", b, L, C), xs_prev), f"{tag} stage{i}.f16 is not the last resblock's running sum"
            x = xs_prev
        if "post" in ops:
            ref, E = V.conv_post_ref(x, V.fold(sd, "conv_post", round16=False).float(), sd["conv_post.bias"], mfma=(_padded(C) == 32))
            _one(summary, f"{tag} conv_post C={C}", _kernel(prof, "conv_post"), b, wave[b, :L], ref, E, 512 if _padded(C) == 32 else 256, 3, True, f32=True)
            assert not bool(wave[b, L:].any()), f"{tag}: samples past clip {b}'s end are not silence"


def _ragged(eng, varch, lengths, seed, tag, summary, **kw):
    """One ragged batch of at most 32 clips of the given lengths (a set: long and short interleaved; a list: as given), every tap verified."""
    lens = lengths if isinstance(lengths, list) else _interleave(lengths)
    assert len(lens) <= 32
    mel = _mel(len(lens), max(lens), seed, varch.num_mels)
    taps, wave, prof = _run(eng, varch, mel, lens)
    _verify(varch, mel, lens, taps, wave, prof, f"{tag} ragged", summary, **kw)
    return prof


def _uniform(eng, varch, L, seed, tag, summary, **kw):
    """One clip of L rows twice: clip 0 against the references, clip 1 (other workgroups' tiles) equal to clip 0 bit for bit."""
    one = _mel(1, L, seed, varch.num_mels)
    mel = torch.cat([one, one]).contiguous()
    taps, wave, prof = _run(eng, varch, mel)
    _verify(varch, mel, None, taps, wave, prof, f"{tag} uniform L={L}", summary, clips=[0], **kw)
    for k, t in taps.items():
        assert torch.equal(t[0], t[1]), f"{tag} uniform L={L}: {k} differs between two copies of one clip"
    assert torch.equal(wave[0], wave[1])
    return prof
