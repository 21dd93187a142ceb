"""The float64 references of tests/encoder_ref.py pinned on the CPU: with unrounded operands each reproduces the oracle's own
function (ref_cpu.hubert_attention with key_mask, ref_cpu.hubert_ffn, the conv stack of ref_cpu.hubert_feature_extractor,
ref_cpu.hubert_pos_conv, F.layer_norm) in float64 to 1e-12 relative, and each bound helper rejects the first value outside its
bound; the exact-fp32 tap-GEMM's references (fp32_products, the grouped positional conv, LayerNorm + Linear) hold for an fp32
evaluation on the CPU and reject a zeroed last row, a shifted tap and a masked column written wrongly.

The bf16 positional conv (posconv.hip and the bf16 tap-GEMM; tests/test_gpu_encoder_ops.py holds them to tapgemm_ref's "bf16"
bound): an fp32 emulation on bf16 operands at the real widths (Cg = 48 / 64) passes at T = 1, 65, 257, 513 and fails with each of
four seeded mistakes -- a halo off by one row at the 256-row half seam, a dropped tap, a neighbouring clip's rows where the zero
padding belongs, the even kernel's extra last row kept.  What that bound can see: it is the worst case of K = 6144 / 8192 fp32
additions, linear in K, and a correct evaluation sits below 1e-3 of it; it catches a wrong row, tap, halo or clip, not a mistake
of a few ulp."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from speech_inpainting_amd import synth
from speech_inpainting_amd.arch import HubertArch
from tests import encoder_ref as E


class _F64:
    """A state-dict entry whose `.float()` is float64: runs the oracle's functions in double precision unchanged."""

    def __init__(self, t):
        self.t = t.double()

    def float(self):
        return self.t


def _sd64(sd):
    return {k: _F64(v) for k, v in sd.items()}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    harch = HubertArch.tiny()
    return harch, synth.synth_hubert_state(harch)


def test_attention_ref_reproduces_the_oracle_with_key_mask(tiny):
    harch, sd = tiny
    p = "base_model.encoder.layers.0.attention."
    B, T, H = 3, 37, harch.hidden_size
    lens = [37, 20, 1]
    h = torch.randn(B, T, H, dtype=torch.float64)
    key_mask = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    want = R.hubert_attention(_sd64(sd), harch, p, h, key_mask)
    wqkv = torch.cat([sd[p + n + "_proj.weight"] for n in "qkv"])
    bqkv = torch.cat([sd[p + n + "_proj.bias"] for n in "qkv"])
    for b in range(B):
        qkv, _ = E.linear_ref(h[b], wqkv, bqkv, round_w=False)
        for p_bf16 in (True, False):
            o, bound = E.attention_ref(qkv, harch.num_attention_heads, Tk=lens[b], p_bf16=p_bf16)
            assert bool((bound > 0).all())
            got, _ = E.linear_ref(o, sd[p + "out_proj.weight"], sd[p + "out_proj.bias"], round_w=False)
            assert _rel(got, want[b]) <= 1e-12, (b, p_bf16)


def test_ffn_ref_reproduces_the_oracle(tiny):
    harch, sd = tiny
    p = "base_model.encoder.layers.1.feed_forward."
    h = torch.randn(45, harch.hidden_size, dtype=torch.float64)
    want = R.hubert_ffn(_sd64(sd), p, h)
    x, _ = E.linear_ref(h, sd[p + "intermediate_dense.weight"], sd[p + "intermediate_dense.bias"], act="gelu", round_w=False)
    res = torch.randn_like(want)
    got, _ = E.linear_ref(x, sd[p + "output_dense.weight"], sd[p + "output_dense.bias"], res=res, round_w=False)
    assert _rel(got - res, want) <= 1e-12


@pytest.mark.parametrize("norm", ["group", "layer"])
def test_conv_stack_refs_reproduce_the_feature_extractor(norm):
    harch = HubertArch.tiny(feat_extract_norm=norm, conv_bias=norm == "layer")
    sd = synth.synth_hubert_state(harch)
    B, N = 2, 3600
    wave = synth.synth_wave(B, N, 5).double()
    want = R.hubert_feature_extractor(_sd64(sd), harch, wave)            # (B, C, T)
    pre = "base_model.feature_extractor.conv_layers."
    for b in range(B):
        k, s = harch.conv_kernel[0], harch.conv_stride[0]
        L1 = (N - k) // s + 1
        x0 = E.conv_rows(wave[b][:, None], k, s, torch.arange(L1))
        w0 = sd[pre + "0.conv.weight"][:, 0, :]
        if norm == "group":
            h, _ = E.conv0_groupnorm_ref(x0, w0, sd[pre + "0.layer_norm.weight"], sd[pre + "0.layer_norm.bias"])
        else:
            y, _ = E.linear_ref(x0, w0, sd[pre + "0.conv.bias"], round_w=False)
            h, _ = E.layernorm_ref(y, sd[pre + "0.layer_norm.weight"], sd[pre + "0.layer_norm.bias"], 1e-5, act="gelu")
        for i in range(1, len(harch.conv_dim)):
            k, s = harch.conv_kernel[i], harch.conv_stride[i]
            L = (h.shape[0] - k) // s + 1
            xi = E.conv_rows(h, k, s, torch.arange(L))
            wi = E.conv_weight(sd[pre + f"{i}.conv.weight"])
            if norm == "group":
                h, _ = E.linear_ref(xi, wi, act="gelu", round_w=False)
            else:
                y, _ = E.linear_ref(xi, wi, sd[pre + f"{i}.conv.bias"], round_w=False)
                h, _ = E.layernorm_ref(y, sd[pre + f"{i}.layer_norm.weight"], sd[pre + f"{i}.layer_norm.bias"], 1e-5, act="gelu")
        assert _rel(h.t(), want[b]) <= 1e-12, b


@pytest.mark.parametrize("C", [512, 768, 1024])
def test_layernorm_ref_reproduces_f_layer_norm(C):
    x = torch.randn(33, C, dtype=torch.float64) * 3 + 0.5
    g, b = torch.randn(C) * 0.1 + 1, torch.randn(C) * 0.1
    got, bound = E.layernorm_ref(x, g, b, 1e-5)
    want = F.layer_norm(x, (C,), g.double(), b.double(), 1e-5)
    assert _rel(got, want) <= 1e-12
    assert bool((bound > 0).all())


def test_rounding_helpers():
    x = torch.tensor([1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -2.0 - 2 ** -7, 0.0, 3e-3], dtype=torch.float64)
    assert E.rne_bf16(x).tolist() == [1.0, 1.0, 1.0 + 4 * 2 ** -8, -2.0, 0.0, float(torch.tensor(3e-3).to(torch.bfloat16))]
    assert E.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, -0.5], dtype=torch.float64)).tolist() == [2 ** -7, 2 ** -7, 2 ** -6, 2 ** -8]
    w = torch.tensor([[1.0 + 2 ** -9]])                                         # a tie between two bf16 values: to even
    assert E.bf16(w).item() == 1.0


def _cases():
    """(name, ref, E, bf16 output?) of every reference on small random operands."""
    torch.manual_seed(1)
    a = E.bf16(torch.randn(40, 256))
    w = torch.randn(64, 256) / 16
    b = torch.randn(64) * 0.1
    res = torch.randn(40, 64)
    out = [("linear", *E.linear_ref(a, w, b), False), ("linear_res", *E.linear_ref(a, w, b, res=res), False),
           ("linear_gelu_bf16", *E.linear_ref(a, w, b, act="gelu"), True)]
    qkv = E.bf16(torch.randn(40, 3 * 128))
    out.append(("attention_bf16", *E.attention_ref(qkv, 2, Tk=33), True))
    out.append(("attention_f32", *E.attention_ref(torch.randn(40, 3 * 128), 2, Tk=7, p_bf16=False), False))
    x = torch.randn(40, 512) * 2
    out.append(("layernorm", *E.layernorm_ref(x, torch.randn(512) * 0.1 + 1, torch.randn(512) * 0.1, 1e-5), False))
    x0 = torch.randn(300, 10)
    out.append(("conv0_groupnorm", *E.conv0_groupnorm_ref(x0, torch.randn(32, 10) * 0.3, torch.randn(32) * 0.1 + 1, torch.randn(32) * 0.1), True))
    return out


@pytest.mark.parametrize("case", range(7))
def test_each_bound_rejects_the_first_value_outside_it(case):
    """The value the kernel would store from the exact result passes (rne(ref) for a bf16 output, fl32(ref) for an fp32 one);
    moving ONE element to the first value of the output type past its bound -- the next bf16 / fp32 above ref + bound -- is
    reported as exactly one violation."""
    name, ref, bound, is_bf16 = _cases()[case]
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all()), name
    check = E.check_bf16 if is_bf16 else E.check_f32
    got = E.rne_bf16(ref) if is_bf16 else ref.float().double()
    assert check(got, ref, bound)["bad"] == 0, name
    g = got.flatten().clone()
    i = int(bound.flatten().argmin())
    r, e = ref.flatten()[i:i + 1], bound.flatten()[i:i + 1]
    limit = r + e + (0.5 * E.ulp_bf16(r.abs() + e) if is_bf16 else 0)   # the largest |got - ref| the check accepts
    v = E.rne_bf16(limit) if is_bf16 else limit.float().double()
    step = E.ulp_bf16 if is_bf16 else E.ulp_f32
    while float(v - r) <= float(limit - r):
        v = v + step(v)
    assert float(v - r) <= float(limit - r) + float(step(v)), name                 # one step of the output type past it
    g[i] = v[0]
    assert check(g.view_as(got), ref, bound)["bad"] == 1, name


# ------------------------------------------------------------------------------- the exact-fp32 tap-GEMM (fp32 encoder)
def test_pos_conv_reference_reproduces_the_oracle_and_rejects_mistakes(tiny):
    """tapgemm_ref with the grouped geometry, GELU and the residual is h + ref_cpu.hubert_pos_conv(h) in float64; in "f32" an fp32
    evaluation lies inside the bound, a tap shifted by one row and a zeroed last row outside; through the encoder's LayerNorm
    (layernorm_of_bounded) likewise."""
    from tests import vocoder_ref as V
    harch, sd = tiny
    H, G, k = harch.hidden_size, harch.num_conv_pos_embedding_groups, harch.num_conv_pos_embeddings
    p = "base_model.encoder.pos_conv_embed.conv."
    geom = E.pos_conv_geom(k, G)
    for T in (1, 37):
        h = torch.randn(T, H)
        want = h.double() + R.hubert_pos_conv(_sd64(sd), harch, "base_model.", h.double()[None])[0]
        w64 = R._conv_weight(_sd64(sd), p[:-1], dim=2)
        got = V.tapgemm_ref(h, w64, sd[p + "bias"], "f64", geom, k * H // G, act="gelu", res=h)
        assert _rel(got.ref, want) <= 1e-12
        w = E.pos_conv_weight(sd)
        assert _rel(w.double(), w64) <= 1e-6
        r = V.tapgemm_ref(h, w, sd[p + "bias"], "f32", geom, k * H // G, act="gelu", res=h)
        assert bool((r.E > 0).all()) and float(r.E.max()) < 1e-2 * float(r.ref.abs().max())      # a bound, not a blanket

        def fp32(hh):
            y = F.conv1d(hh.t()[None], w, sd[p + "bias"], padding=k // 2, groups=G)[0].t()[:T]
            return hh + F.gelu(y)

        good = fp32(h)
        assert V.check_f32(good, r.ref, r.E)["bad"] == 0
        if T > 1:
            shifted = h + (fp32(torch.cat([h[1:], torch.zeros(1, H)])) - torch.cat([h[1:], torch.zeros(1, H)]))
            assert V.check_f32(shifted, r.ref, r.E)["bad"] > 0
            z = good.clone()
            z[T - 1] = 0
            assert V.check_f32(z, r.ref, r.E)["bad"] > 0
            g_, b_ = sd["base_model.encoder.layer_norm.weight"], sd["base_model.encoder.layer_norm.bias"]
            ref, bound = E.layernorm_of_bounded(r.ref, r.E, g_, b_, 1e-5)
            assert float(bound.max()) < 1e-2 * float(ref.abs().max())
            ln = F.layer_norm(good, (H,), g_, b_, 1e-5)
            assert E.check_f32(ln, ref, bound)["bad"] == 0
            assert E.check_f32(F.layer_norm(shifted, (H,), g_, b_, 1e-5), ref, bound)["bad"] > 0
            # the passage term is needed: the worst-case input inside the conv's bound leaves the LayerNorm's own bound
            own = E.layernorm_ref(r.ref, g_, b_, 1e-5)[1]
            moved = F.layer_norm(r.ref + r.E * torch.sign(torch.randn(T, H, dtype=torch.float64)), (H,), g_.double(), b_.double(), 1e-5)
            assert E.check_f32(moved, ref, bound)["bad"] == 0 and E.check_f32(moved, ref, own)["bad"] > 0


def test_ln_linear_reference_and_the_masked_columns():
    """LayerNorm + Linear(-> 80): F.layer_norm + F.linear in float64 to 1e-12; an fp32 evaluation inside the bound; a last row zeroed, a
    column of the partial tile (64 .. 79) left unwritten and a weight row taken from the padding (80: zeros, so the bias alone) outside."""
    torch.manual_seed(3)
    H, N, M = 256, 80, 129
    x = torch.randn(M, H) * 2 + 0.3
    g, b = torch.randn(H) * 0.1 + 1, torch.randn(H) * 0.1
    w, bias = torch.randn(N, H) / 16, torch.randn(N) * 0.1
    ref, bound = E.ln_linear_ref(x, g, b, 1e-5, w, bias)
    want = F.linear(F.layer_norm(x.double(), (H,), g.double(), b.double(), 1e-5), w.double(), bias.double())
    assert _rel(ref, want) <= 1e-12 and float(bound.max()) < 1e-2 * float(ref.abs().max())
    good = F.linear(F.layer_norm(x, (H,), g, b, 1e-5), w, bias)
    assert E.check_f32(good, ref, bound)["bad"] == 0
    for mutate in (lambda t: t[M - 1].zero_(), lambda t: t[:, 79].zero_(), lambda t: t[:, 64].copy_(bias[64].expand(M))):
        bad = good.clone()
        mutate(bad)
        assert E.check_f32(bad, ref, bound)["bad"] > 0
    lin, lb = E.ln_linear_ref(x, None, None, 0.0, w, bias)
    plain, pb = E.linear_ref(x, w, bias, round_w=False)
    assert torch.equal(lin, plain) and bool((lb > pb).all()) and bool((lb <= pb * (1 + 2.0 ** -8)).all())   # one U per product on K + 1 >= 257 terms' gamma
    assert E.check_f32(F.linear(x, w, bias), lin, lb)["bad"] == 0


def test_pos_conv_bound_at_the_real_width_rejects_a_dropped_halo_row():
    """HuBERT-base's positional conv (K = 128 x 48 = 6144 products: the worst-case bound is some per cent of the output) still separates
    a correct fp32 evaluation (far inside) from a tile that reads the last row of the tile before it as zero (the first row of a
    second 128-row tile, T = 129)."""
    from tests import vocoder_ref as V
    harch = HubertArch(num_hidden_layers=1)
    sd = synth.synth_hubert_state(harch, 31)
    H, G, k, T = harch.hidden_size, harch.num_conv_pos_embedding_groups, harch.num_conv_pos_embeddings, 129
    w, bias = E.pos_conv_weight(sd), sd["base_model.encoder.pos_conv_embed.conv.bias"]
    h = torch.randn(T, H, generator=torch.Generator().manual_seed(2)) * 0.5
    r = V.tapgemm_ref(h, w, bias, "f32", E.pos_conv_geom(k, G), k * H // G, act="gelu", res=h)

    def fp32(x):
        return h + F.gelu(F.conv1d(x.t()[None], w, bias, padding=k // 2, groups=G)[0].t()[:T])

    good = fp32(h)
    assert float(V.check_f32(good, r.ref, r.E)["ratio"].max()) < 1e-2
    h2 = h.clone()
    h2[127] = 0
    bad = good.clone()
    bad[128] = fp32(h2)[128]
    c = V.check_f32(bad, r.ref, r.E)
    assert c["bad"] > 0 and float(c["ratio"].max()) > 3


# ------------------------------------------------------------------------------- the bf16 positional conv (posconv.hip, bf16 tap-GEMM)
_PC = {}


def _pc_setup(cg, T):
    """(h, w, bias, k, G, reference) of the positional conv at the real width (Cg = 48: base, 64: large) on T rows of N(0, 0.5^2);
    computed once per (Cg, T) and shared, never modified."""
    from tests import vocoder_ref as V
    if ("sd", cg) not in _PC:
        import dataclasses
        harch = HubertArch(num_hidden_layers=1) if cg == 48 else dataclasses.replace(HubertArch.large(), num_hidden_layers=1)
        sd = synth.synth_hubert_state(harch, 31)
        _PC[("sd", cg)] = (harch, E.pos_conv_weight(sd), sd["base_model.encoder.pos_conv_embed.conv.bias"])
    harch, w, bias = _PC[("sd", cg)]
    H, G, k = harch.hidden_size, harch.num_conv_pos_embedding_groups, harch.num_conv_pos_embeddings
    if (cg, T) not in _PC:
        h = torch.randn(T, H, generator=torch.Generator().manual_seed(100 + T)) * 0.5
        _PC[(cg, T)] = (h, V.tapgemm_ref(h, w, bias, "bf16", E.pos_conv_geom(k, G), k * H // G, act="gelu", res=h))
    h, r = _PC[(cg, T)]
    return h, w, bias, k, G, r


def _pc_emulate(h, w, bias, k, G, x=None, keep_last_row=False):
    """What posconv.hip and the bf16 tap-GEMM compute, in fp32 on the CPU: operands rounded to bf16, an fp32 conv1d (zero padding k / 2,
    the even kernel's extra last row dropped), erf-GELU, the fp32 residual h.  x: the rows the conv reads when they are not h's own
    (the seeded mistakes); keep_last_row: the FIRST of the T + 1 rows dropped instead of the last."""
    T = h.shape[0]
    x = h if x is None else x
    y = F.conv1d(x.to(torch.bfloat16).float().t()[None], w.to(torch.bfloat16).float(), bias, padding=k // 2, groups=G)[0].t()
    return h + F.gelu(y[1:T + 1] if keep_last_row else y[:T])


@pytest.mark.parametrize("cg", [48, 64])
@pytest.mark.parametrize("T", [1, 65, 257, 513])
def test_bf16_pos_conv_emulation_passes_the_bound(cg, T):
    """The fp32 emulation of the bf16 positional conv lies inside tapgemm_ref's "bf16" bound at every element, and far inside: below
    1e-3 of E (the bound is the worst case of K = 6144 / 8192 fp32 additions).  T = 1 (every tap but one reads padding), 65 (the first
    and last taps reach a real row), 257 and 513 (one row past posconv.hip's 256-row half and 512-row block)."""
    from tests import vocoder_ref as V
    h, w, bias, k, G, r = _pc_setup(cg, T)
    c = V.check_f32(_pc_emulate(h, w, bias, k, G), r.ref, r.E)
    print(f"Cg={cg} T={T}: max err / E {float(c['ratio'].max()):.2e}")
    assert c["finite"] and c["bad"] == 0
    assert float(c["ratio"].max()) < 1e-3


@pytest.mark.parametrize("cg", [48, 64])
def test_bf16_pos_conv_bound_rejects_a_halo_off_by_one_at_the_half_seam(cg):
    """Rows >= 256 (the second half of a posconv.hip tile) computed from an input shifted by one row: outside the bound.
    Measured on the CPU: Cg = 48: 181 647 of 393 984 elements at T = 513, 723 of 197 376 at T = 257 (one wrong row);
    Cg = 64: 232 277 of 525 312 and 949 of 263 168."""
    from tests import vocoder_ref as V
    for T in (257, 513):
        h, w, bias, k, G, r = _pc_setup(cg, T)
        bad = _pc_emulate(h, w, bias, k, G).clone()
        shifted = torch.cat([h[1:], torch.zeros(1, h.shape[1])])
        bad[256:] = _pc_emulate(h, w, bias, k, G, x=shifted)[256:]
        c = V.check_f32(bad, r.ref, r.E)
        print(f"Cg={cg} T={T}: {c['bad']} of {bad.numel()} outside")
        assert c["bad"] > 0 and not bool((~c["ok"][:256]).any())
        assert float(c["ratio"].max()) > 3


@pytest.mark.parametrize("cg", [48, 64])
def test_bf16_pos_conv_bound_rejects_a_dropped_tap(cg):
    """One of the 128 taps left out (tap 0, which reads row t - 64: T >= 65 for it to read a real row at all; at T = 1 it reads
    padding and nothing fails).  Measured on the CPU at T = 257: Cg = 48: 56 993 of 197 376 elements outside the bound; Cg = 64: 53 124 of
    263 168."""
    from tests import vocoder_ref as V
    h, w, bias, k, G, r = _pc_setup(cg, 257)
    w2 = w.clone()
    w2[:, :, 0] = 0
    c = V.check_f32(_pc_emulate(h, w2, bias, k, G), r.ref, r.E)
    print(f"Cg={cg}: {c['bad']} of {h.numel()} outside")
    assert c["bad"] > 0 and not bool((~c["ok"][:64]).any())            # rows < 64: tap 0 reads padding
    h1, _, _, _, _, r1 = _pc_setup(cg, 1)
    assert V.check_f32(_pc_emulate(h1, w2, bias, k, G), r1.ref, r1.E)["bad"] == 0


@pytest.mark.parametrize("cg", [48, 64])
def test_bf16_pos_conv_bound_rejects_a_neighbouring_clip_in_the_padding(cg):
    """Two clips packed (65 and 257 rows): the conv of the first reads the second's rows where its zero padding belongs, and the
    second's the first's.  Measured on the CPU: Cg = 48: 41 342 of 49 920 elements of the first clip and 38 108 of 197 376 of the second outside the bound; Cg = 64:
    51 596 of 66 560 and 46 234 of 263 168."""
    from tests import vocoder_ref as V
    ha, w, bias, k, G, ra = _pc_setup(cg, 65)
    hb, _, _, _, _, rb = _pc_setup(cg, 257)
    both = torch.cat([ha, hb])
    out = _pc_emulate(both, w, bias, k, G)
    ca, cb = V.check_f32(out[:65], ra.ref, ra.E), V.check_f32(out[65:], rb.ref, rb.E)
    print(f"Cg={cg}: {ca['bad']} of {ha.numel()} and {cb['bad']} of {hb.numel()} outside")
    assert ca["bad"] > 0 and cb["bad"] > 0
    assert not bool((~cb["ok"][64:]).any())                            # rows >= 64 of the second clip read none of the first


@pytest.mark.parametrize("cg", [48, 64])
def test_bf16_pos_conv_bound_rejects_the_even_kernels_extra_row_kept(cg):
    """The even kernel gives T + 1 rows; keeping the last and dropping the first shifts the conv's output by one row.  Measured on
    the CPU at T = 65: Cg = 48: 47 703 of 49 920 elements outside the bound; Cg = 64: 62 002 of 66 560."""
    from tests import vocoder_ref as V
    h, w, bias, k, G, r = _pc_setup(cg, 65)
    c = V.check_f32(_pc_emulate(h, w, bias, k, G, keep_last_row=True), r.ref, r.E)
    print(f"Cg={cg}: {c['bad']} of {h.numel()} outside")
    assert c["bad"] > 0 and float(c["ratio"].max()) > 3
