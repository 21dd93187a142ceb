"""The float64 references of tests/encoder_ref.py pinned on the CPU: with unrounded operands each reproduces the oracle's own
function (ref_cpu.hubert_attention with key_mask, ref_cpu.hubert_ffn, the conv stack of ref_cpu.hubert_feature_extractor,
F.layer_norm) in float64 to 1e-12 relative, and each bound helper rejects the first value outside its bound."""
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
