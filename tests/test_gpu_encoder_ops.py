"""Each kernel of the bf16 encoder against a float64 reference of its own operation (tests/encoder_ref.py), on the operands
the kernel itself read, captured through the encoder's per-op taps: the GEMMs (gemmcu.hip's six instantiations, lingemm.hip's
three tile heights, the tap-GEMM's bf16 path) at M = BM - 1, BM, BM + 1 and on ragged per-clip segments; the attention kernels
at the 32-key tile edges, across the whole-K/V / tiled switch (T = 256 / 257), on padded and ragged batches; LayerNorm at
C = 512, 768, 1024 (its bf16 operand bit-equal to rne of its fp32 rows); conv0 + GroupNorm + GELU.  Real layer widths, one
layer.  Every bound is an error bound derived in encoder_ref.py, not a tolerance fitted to these runs."""
import dataclasses
import os

import pytest
import torch

from tests import encoder_ref as E

pytestmark = pytest.mark.gpu

torch.set_num_threads(16)
GEMMCU_BM = {10: 320, 11: 256, 12: 160, 13: 224, 14: 128, 15: 208}
GEMMCU_BN = {10: 256, 11: 256, 12: 128, 13: 128, 14: 128, 15: 256}
# Fraction of a launch's bf16 outputs that differ from rne(float64 result), the bf16 value nearest to the exact one: twice the
# worst measured over this file's runs on MI355X (GEMM / conv 0.395 %, conv0 + GroupNorm 0.051 %, LayerNorm + GELU 0.032 %,
# attention_kernel with a bf16 output 0.0061 %).  The bf16-input attention kernels round P to bf16 before P V, so about one
# output in five lands on the other neighbour of the exact value (measured up to 18.6 %, at T = 31); their limit is the same
# twice-measured guard, the error bound above being the check on their arithmetic.
MISMATCH_LIMIT = {"gemm": 0.0079, "conv0": 0.00103, "ln": 0.00064, "attention": 0.00012, "attention_p16": 0.372}


def _base():
    from speech_inpainting_amd.arch import HubertArch
    return HubertArch(num_hidden_layers=1)


def _large():
    from speech_inpainting_amd.arch import HubertArch
    return dataclasses.replace(HubertArch.large(), num_hidden_layers=1)


_STATES = {}


def _state(harch):
    from speech_inpainting_amd import synth
    key = (harch.hidden_size, harch.feat_extract_norm, harch.do_stable_layer_norm)
    if key not in _STATES:
        _STATES[key] = synth.synth_hubert_state(harch, 31)
    return _STATES[key]


def _engine(harch, env=None):
    """bf16 encoder; `env` knobs are read when the context is created."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import VocoderArch
    from speech_inpainting_amd.engine import InpaintingEngine
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = InpaintingEngine(harch, VocoderArch.tiny(), 50, "cuda:0", "bf16", "fp32")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return eng.load_state(_state(harch), synth.synth_generator_state(VocoderArch.tiny()), synth.synth_codebook(50))


def _run(eng, harch, wave, lens=None, valid_len=None, profile=False):
    """One encoder forward with every per-op tap registered -> (taps {name: cpu tensor} of the taps the path produced,
    rows of the transformer, kernel names if profiled)."""
    B, N = wave.shape
    R = sum(harch.num_frames(n) for n in lens) if lens is not None else B * harch.num_frames(N)
    cap = E.tap_capacities(harch, B, N, R)
    eng.ctx.clear_captures()
    caps = eng.ctx.capture(list(cap), capacity=cap)
    if profile:
        eng.ctx.profile_start(4000)
    if lens is not None:
        out = eng.encode_ragged(wave, lens)
    else:
        out = eng.encode(wave, valid_len=valid_len, normalize=False)
    names = {e["name"] for e in eng.ctx.profile_stop()} if profile else set()
    torch.cuda.synchronize()
    produced = {k: eng.ctx.lib.si_debug_size(eng.ctx._h, k.encode()) for k in cap}
    got = {k: v.cpu() for k, v in caps.items() if produced[k] > 0 and produced[k] == cap[k]}
    eng.ctx.clear_captures()
    assert bool(torch.isfinite(out).all())
    return got, R, names


def _f64(t):
    return t.double()


def _check(tag, kind, got, ref, bound, limit_key="gemm"):
    r = E.check_bf16(got, ref, bound) if kind == "bf16" else E.check_f32(got, ref, bound)
    print("   " + E.fmt(tag, r))
    assert r["bad"] == 0, E.fmt(tag, r)
    if kind == "bf16":
        assert r["mismatch"] <= MISMATCH_LIMIT[limit_key], E.fmt(tag, r)
    return r


def _tap(got, name):
    """(tensor, 'bf16' | 'f32') of whichever form of the tap the path stored."""
    if name + ".bf16" in got:
        return got[name + ".bf16"], "bf16"
    return got[name], "f32"


def _sel_rows(M, k=96, seed=0):
    """Rows to check of a long GEMM: the first 8, the last 336 (every last tile of every height, whole), k random ones."""
    if M <= 512:
        return torch.arange(M)
    g = torch.Generator().manual_seed(seed)
    return torch.unique(torch.cat([torch.arange(8), torch.arange(M - 336, M), torch.randint(0, M, (k,), generator=g)]))


def _check_layers(got, harch, R, tag, rows=None):
    """Every GEMM of every captured layer against linear_ref on its captured operands."""
    sd = _state(harch)
    H = harch.hidden_size
    rows = torch.arange(R) if rows is None else rows
    for l in range(harch.num_hidden_layers):
        p = f"base_model.encoder.layers.{l}."
        pre = harch.do_stable_layer_norm
        hin = got[f"layer{l}.h"].view(R, H)[rows]
        if f"layer{l}.h.bf16" in got:
            a_qkv = got[f"layer{l}.h.bf16"].view(R, H)[rows]
        else:                                                              # fp32 operand, rounded by the GEMM's staging
            a_qkv = E.bf16(got[f"layer{l}.ln1"].view(R, H)[rows] if pre else hin)
        wqkv = torch.cat([sd[p + f"attention.{n}_proj.weight"] for n in "qkv"])
        bqkv = torch.cat([sd[p + f"attention.{n}_proj.bias"] for n in "qkv"])
        qkv, kq = _tap(got, f"layer{l}.qkv")
        _check(f"{tag} layer{l} QKV", kq, qkv.view(R, 3 * H)[rows], *E.linear_ref(_f64(a_qkv), wqkv, bqkv))
        att, ka = _tap(got, f"layer{l}.att")
        a_out = _f64(att.view(R, H)[rows]) if ka == "bf16" else E.bf16(att.view(R, H)[rows])
        _check(f"{tag} layer{l} out-proj + residual", "f32", got[f"layer{l}.att_res"].view(R, H)[rows],
               *E.linear_ref(a_out, sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"], res=hin))
        if pre:
            a_ffn = got[f"layer{l}.ln2.bf16"].view(R, H)[rows] if f"layer{l}.ln2.bf16" in got else E.bf16(got[f"layer{l}.ln2"].view(R, H)[rows])
            res2 = got[f"layer{l}.att_res"].view(R, H)[rows]
        else:
            a_ffn = got[f"layer{l}.ln1.bf16"].view(R, H)[rows] if f"layer{l}.ln1.bf16" in got else E.bf16(got[f"layer{l}.ln1"].view(R, H)[rows])
            res2 = got[f"layer{l}.ln1"].view(R, H)[rows]
        I = harch.intermediate_size
        ffn, kf = _tap(got, f"layer{l}.ffn")
        _check(f"{tag} layer{l} FFN1 + GELU", kf, ffn.view(R, I)[rows],
               *E.linear_ref(_f64(a_ffn), sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"], act="gelu"))
        a2 = _f64(ffn.view(R, I)[rows]) if kf == "bf16" else E.bf16(ffn.view(R, I)[rows])
        _check(f"{tag} layer{l} FFN2 + residual", "f32", got[f"layer{l}.ffn_res"].view(R, H)[rows],
               *E.linear_ref(a2, sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"], res=res2))


def _check_convs(got, harch, B, N, tag, clip_lens=None):
    """Strided convs 1..n-1 of every clip against linear_ref on their captured inputs (rows: _sel_rows of the clip's own length)."""
    sd = _state(harch)
    Ls = harch.feat_lengths(N)
    layer = harch.feat_extract_norm == "layer"
    pre = "base_model.feature_extractor.conv_layers."
    for i in range(1, len(harch.conv_dim)):
        Cin, C, k, s = harch.conv_dim[i - 1], harch.conv_dim[i], harch.conv_kernel[i], harch.conv_stride[i]
        xin, kin = _tap(got, f"conv{i - 1}.ln" if layer else f"conv{i - 1}")
        y, ky = _tap(got, f"conv{i}")
        xin = xin.view(B, Ls[i], Cin)
        y = y.view(B, Ls[i + 1], C)
        w = E.conv_weight(sd[pre + f"{i}.conv.weight"])
        bias = sd[pre + f"{i}.conv.bias"] if harch.conv_bias else None
        for b in sorted({0, 1, B - 1}) if B > 3 and clip_lens is None else range(B):
            Lb = harch.feat_lengths(clip_lens[b])[i + 1] if clip_lens is not None else Ls[i + 1]
            rows = _sel_rows(Lb, seed=b)
            xb = _f64(xin[b]) if kin == "bf16" else E.bf16(xin[b])
            ref, bound = E.linear_ref(E.conv_rows(xb, k, s, rows), w, bias, act=None if layer else "gelu")
            _check(f"{tag} conv{i} clip {b} (L = {Lb})", ky, y[b][rows], ref, bound)


def _pick_wave(harch, B, T, bm):
    """A batch of B clips of exactly T frames whose sample count puts as many strided convs as possible at a last tile of 1 or
    bm - 1 rows (every count 320 (T - 1) + 400 + d, d < 320, has T frames)."""
    from speech_inpainting_amd import synth
    best, bestd = -1, 0
    for d in range(320):
        Ls = harch.feat_lengths(320 * (T - 1) + 400 + d)
        score = sum(L % bm in (1, bm - 1) for L in Ls[2:-1])
        if score > best:
            best, bestd = score, d
    N = 320 * (T - 1) + 400 + bestd
    assert harch.num_frames(N) == T
    return synth.synth_wave(B, N, 7 + T).cuda()


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
    _check_convs(got, harch, len(lens), max(lens), f"ragged {arch}", clip_lens=lens)


# ------------------------------------------------------------------------------------------------------------ attention
def _check_attention(got, harch, clips, tag, kind_out=None, p_bf16=True):
    """clips: [(first packed row, T, Tk)]; every query row of every clip, padded ones included."""
    H, heads = harch.hidden_size, harch.num_attention_heads
    qkv, kq = _tap(got, "layer0.qkv")
    att, ka = _tap(got, "layer0.att")
    R = att.numel() // H
    qkv, att = qkv.view(R, 3 * H), att.view(R, H)
    if kind_out is not None:
        assert ka == kind_out, (ka, kind_out)
    for r0, T, Tk in clips:
        q = _f64(qkv[r0:r0 + T]) if kq == "bf16" or not p_bf16 else E.bf16(qkv[r0:r0 + T])
        ref, bound = E.attention_ref(q, heads, Tk=Tk, p_bf16=p_bf16)
        _check(f"{tag} T={T} keys={Tk}", ka, att[r0:r0 + T], ref, bound, "attention_p16" if p_bf16 else "attention")


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
    sd = _state(harch)
    H = harch.hidden_size
    p = "base_model.encoder.layers.0."
    if not harch.do_stable_layer_norm:
        for ln, x, key in (("ln1", "att_res", "layer_norm"), ("ln2", "ffn_res", "final_layer_norm")):
            rows = got[f"layer0.{ln}"].view(R, H)
            ref, bound = E.layernorm_ref(got[f"layer0.{x}"].view(R, H), sd[p + key + ".weight"], sd[p + key + ".bias"], harch.layer_norm_eps)
            _check(f"{arch} {ln} (C = {H}) fp32 rows", "f32", rows, ref, bound)
            op = got[f"layer0.{ln}.bf16"].view(R, H)
            assert torch.equal(op, rows.to(torch.bfloat16)), f"{ln}: the bf16 operand is not rne of the fp32 rows"
    else:
        h = got["layer0.h"].view(R, H)
        ref, bound = E.layernorm_ref(h, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], harch.layer_norm_eps)
        _check(f"{arch} ln1 (C = {H}) bf16 operand", "bf16", got["layer0.ln1.bf16"].view(R, H), ref, bound, "ln")
        ref, bound = E.layernorm_ref(got["layer0.att_res"].view(R, H), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], harch.layer_norm_eps)
        _check(f"{arch} ln2 (C = {H}) bf16 operand", "bf16", got["layer0.ln2.bf16"].view(R, H), ref, bound, "ln")
    if harch.feat_extract_norm == "layer":
        pre = "base_model.feature_extractor.conv_layers."
        Ls = harch.feat_lengths(N)
        for i in range(len(harch.conv_dim)):
            C = harch.conv_dim[i]
            x = got[f"conv{i}"].view(B, Ls[i + 1], C)
            y, ky = _tap(got, f"conv{i}.ln")
            y = y.view(B, Ls[i + 1], C)
            for b in range(B):
                rows = _sel_rows(Ls[i + 1], seed=b)
                ref, bound = E.layernorm_ref(x[b][rows], sd[pre + f"{i}.layer_norm.weight"], sd[pre + f"{i}.layer_norm.bias"], 1e-5, act="gelu")
                _check(f"conv{i} LayerNorm + GELU (C = {C}) clip {b}", ky, y[b][rows], ref, bound, "ln")


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
