"""The fp32 / bf16x3 / bf16 vocoder's tapped run and its check of every launch of the tap-GEMM against vocoder_ref.tapgemm_ref, for
tests/test_gpu_tapgemm_ops.py (the V1 widths) and tests/test_gpu_unitvoc_ops.py (the unit vocoder's geometry).  What is checked and
why: test_gpu_tapgemm_ops.py's docstring."""
import torch

from tests import vocoder_ref as V
from tests.cases import _config, _mel, _state
from tests.harness import build_engine, tapped_run

MODES = {"fp32": ("fp32", "f32", {}), "bf16x3": ("bf16x3", "bf16x3", {}), "bf16": ("bf16", "bf16", {"SI_VOC_OPREADY": "0"})}

_FOLDED = {}


def _mel_ld(num_mels):
    return -(-num_mels // 32) * 32


def _engine(varch, mode, opready=False):
    """An engine per (architecture, arithmetic), kept for the session: the knobs are read when the context is created."""
    from speech_inpainting_amd.arch import HubertArch
    voc, _, env = MODES[mode]
    return build_engine(HubertArch.tiny(), varch, 20, "fp32", voc, env={} if opready else env, state=(None, _state(varch), None),
                        key=("tapgemm", repr(varch), mode, opready))


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
    """One generator pass -> (taps {name: (B, rows, C) cpu}, wave cpu, {kernel: launches}); every tap must have been produced."""
    B, _, Tm = mel.shape
    shapes = _shapes(varch, B, Tm, t_suffix)
    cap = {k: s[0] * s[1] * s[2] for k, s in shapes.items()} if tapped else {}
    taps, wave, prof = tapped_run(eng.ctx, cap, lambda: eng.vocode_ragged(mel.cuda(), lens, stretch=False) if lens is not None
                                  else eng.vocode(mel.cuda(), stretch=False), require_all=True)
    return {k: t.view(shapes[k]) for k, t in taps.items()}, wave.cpu(), prof


def _one(summary, tag, kernel, clip, got, r, stored, halo):
    L = r.ref.shape[0]
    c = V.check_f32(got.reshape(r.ref.shape), r.ref, r.E)
    line, near, rest = V.report(tag, kernel, clip, c, L, stored, halo)
    print("   " + line)
    assert c["finite"] and c["bad"] == 0, line
    if r.exact is not None and r.exact is not r.ref:           # bf16x3: also within the derived distance of the exact fp32 product
        cx = V.check_f32(got.reshape(r.ref.shape), r.exact, r.E_exact)
        linex, _, _ = V.report(tag + " vs the fp32 product", kernel, clip, cx, L, stored, halo)
        assert cx["bad"] == 0, linex
    summary.note(kernel, near, rest)


def _verify(varch, mode, mel, lens, taps, prof, tag, summary, clips=None, wave=None):
    """Every tap of every clip against its reference from the tapped input, noted into `summary`; -> the configurations the launches
    must have taken.
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
        _one(summary, f"{tag} conv_pre {nm}->{C0}", kern, b, x, r, bm, 6)
        C, Lm = C0, Lmax
        for i, (u, k) in enumerate(zip(varch.upsample_rates, varch.upsample_kernel_sizes)):
            w = _w(varch, f"ups.{i}")
            ntaps, pad = -(-k // u), (k - u) // 2
            Lo, Lmo, Cin, C = L * u, Lm * u, C, C // 2
            kern, bm = _config(math, u * C, (pad + Lmo - 1) // u + 1, ntaps, -1, Cin)
            want.add(kern)
            r = V.tapgemm_ref(x, w, sd[f"ups.{i}.bias"], math, V.tconv_geom(u), ntaps * Cin, slope=V.SLOPE32)
            U = taps[f"ups{i}"][b, :Lo]
            _one(summary, f"{tag} ups{i} {Cin}->{C} u={u} k={k}", kern, b, U, r, bm * u, k)
            L, Lm = Lo, Lmo
            xs_prev = None
            for j, (rk, dils) in enumerate(zip(varch.resblock_kernel_sizes, varch.resblock_dilation_sizes)):
                p = f"resblocks.{i * nk + j}."
                xin = U
                for n, d in enumerate(dils):
                    last = n == len(dils) - 1
                    # (the dilated conv's halo decides its tile: up to V1's 255 + 10 * 5 + 1 <= 384 rows it never changes it)
                    kern, bm = _config(math, C, Lm, rk, d, C)
                    want.add(kern)
                    t = taps[f"stage{i}.rb{j}.t{n}"][b, :L]
                    r = V.tapgemm_ref(xin, _w(varch, f"{p}convs1.{n}"), sd[f"{p}convs1.{n}.bias"], math, V.conv_geom(d), rk * C, slope=V.SLOPE32)
                    _one(summary, f"{tag} stage{i}.rb{j}.t{n} k={rk} d={d}", kern, b, t, r, bm, (rk - 1) * d)
                    prev = xs_prev if (last and j > 0) else None
                    kern, bm = _config(math, C, Lm, rk, 1, C)
                    want.add(kern)
                    r = V.tapgemm_ref(t, _w(varch, f"{p}convs2.{n}"), sd[f"{p}convs2.{n}.bias"], math, V.conv_geom(1), rk * C, slope=V.SLOPE32,
                                      res=xin, alpha=a_last if last else 1.0, prev=prev)
                    out = taps[f"stage{i}.rb{j}.p{n}"][b, :L]
                    _one(summary, f"{tag} stage{i}.rb{j}.p{n} k={rk}" + (" alpha" if last else "") + (" acc" if prev is not None else ""), kern, b, out, r, bm, rk - 1)
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
            summary.note(f"conv_post_kernel C={C}", near, rest)
    got = {n for n in prof if n.startswith("tapgemm_")}
    assert got == want, f"{tag}: the launches took {sorted(got)}, launch_math restated gives {sorted(want)}"
    return want


def _uniform(varch, mode, L, seed, tag, summary, post=False):
    one = _mel(1, L, seed, varch.num_mels)
    mel = torch.cat([one, one]).contiguous()
    taps, wave, prof = _run(_engine(varch, mode), varch, mel)
    cfgs = _verify(varch, mode, mel, None, taps, prof, f"{tag} L={L}", summary, clips=[0], wave=wave if post else None)
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
