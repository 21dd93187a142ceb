"""tests/weights_ref.py is right and it is sensitive (CPU only; the library is not called here).

Right: the fold against g v / ||v|| in float64 within three fp32 roundings; the three casts against torch's own conversions and
tests/vocoder_ref.py's h16 / split_bf16 at ties, +-65504, the first value above it, subnormals and +-0; the codebook tables against
the oracle's centre / centred / norm in float64 within bounds built from the operands; the permutation property of the fp32 form.
Sensitive: every planted mistake of weights_ref.BUGS changes bytes."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from speech_inpainting_amd import native, synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from tests import vocoder_ref as V
from tests import weights_ref as W

U = 2.0 ** -24


def _pair():
    harch, varch = HubertArch.tiny(), VocoderArch.tiny()
    # (a codebook around 0: around the log-mel level -5 the subtraction of the centre is exact and `raw = v + centre` returns c itself)
    return harch, varch, W.state_arrays(synth.synth_hubert_state(harch, 5), synth.synth_generator_state(varch, 6), synth.synth_codebook(100, 80, 7) + 5.0)


@pytest.mark.parametrize("name,dim", [("generator.conv_pre", 0), ("generator.ups.1", 0), ("generator.resblocks.4.convs2.1", 0),
                                      ("base_model.encoder.pos_conv_embed.conv", 2)])
def test_fold_against_float64(name, dim):
    """w = v * (g / nrm): the norm, the quotient and the product round once each in fp32 (the float64 sum under the root moves the
    norm by far less than its fp32 rounding: the .01), so |w32 - w64| <= 3.01 * 2^-24 |w64| + 2^-149."""
    _, _, sd = _pair()
    gn, vn = (name + ".weight_g", name + ".weight_v") if name + ".weight_g" in sd else (name + ".parametrizations.weight.original0",
                                                                                       name + ".parametrizations.weight.original1")
    v, g = sd[vn], sd[gn]
    w32 = W.fold(v, g, dim).astype(np.float64)
    axes = tuple(a for a in range(v.ndim) if a != dim)
    v64 = v.astype(np.float64)
    w64 = v64 * (g.astype(np.float64).reshape(np.sqrt((v64 ** 2).sum(axis=axes, keepdims=True)).shape) / np.sqrt((v64 ** 2).sum(axis=axes, keepdims=True)))
    err = np.abs(w32 - w64)
    bound = 3.01 * U * np.abs(w64) + 2.0 ** -149
    print(f"{name}: max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert np.array_equal(W.module_weight(sd, name, dim), W.fold(v, g, dim))
    if dim == 0:                                                   # the kernels' tests read their operands through vocoder_ref.fold
        tsd = {"m.weight_g": torch.from_numpy(g), "m.weight_v": torch.from_numpy(v)}
        assert np.array_equal(V.fold(tsd, "m", round16=False).numpy(), w32)


def _edge_values():
    f = np.float32
    vals = [0.0, -0.0, 1.0, -1.0, 65504.0, -65504.0, np.nextafter(f(65504), f(np.inf)), -np.nextafter(f(65504), f(np.inf)), 65519.99, 65520.0, 70000.0, -1e6,
            3.0e38, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -126, 2.0 ** -149, -2.0 ** -140,
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23,           # bf16 ties and their neighbours
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 2048 + 1.0, 2048 + 3.0,             # fp16 ties
            np.pi, -np.e * 1e-3, 1e-7, 123.456]
    rng = np.random.default_rng(0)
    return np.concatenate([np.array(vals, dtype=np.float32), rng.standard_normal(4096).astype(np.float32) * np.float32(3.0),
                           (rng.standard_normal(512) * 2e4).astype(np.float32)])


def test_casts_against_torch_and_the_kernel_tests_helpers():
    x = _edge_values()
    t = torch.from_numpy(x)
    # bf16, round to nearest even
    assert np.array_equal(W.bf16_bits(x), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(W.bf16_val(W.bf16_bits(x)), V.bf16r(t).numpy())
    # the bf16x3 planes
    hi, lo = W.bf16_split_bits(x)
    vhi, vlo = V.split_bf16(t)
    assert np.array_equal(W.bf16_val(hi).astype(np.float64), vhi.numpy()) and np.array_equal(W.bf16_val(lo).astype(np.float64), vlo.numpy())
    big = np.abs(x) < 1e30                                          # hi + lo restores v to 2^-16 relative (17 significant bits)
    assert (np.abs(W.bf16_val(hi).astype(np.float64) + W.bf16_val(lo).astype(np.float64) - x)[big] <= 2.0 ** -16 * np.abs(x)[big] + 2.0 ** -133).all()
    # fp16: round to nearest even below the limit, saturation above it
    want = t.clamp(-65504.0, 65504.0).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(W.f16_bits(x), want)
    inr = np.abs(x) <= 65504.0
    assert np.array_equal(W.f16_bits(x)[inr].view(np.float16).astype(np.float64), V.h16(t).numpy()[inr])
    pin = lambda v: int(W.f16_bits(np.array([v], np.float32))[0])
    assert pin(65504.0) == 0x7BFF and pin(-65504.0) == 0xFBFF and pin(np.nextafter(np.float32(65504), np.float32(np.inf))) == 0x7BFF
    assert pin(65520.0) == 0x7BFF and pin(-1e6) == 0xFBFF and pin(0.0) == 0 and pin(-0.0) == 0x8000
    assert pin(2.0 ** -24) == 1 and pin(2.0 ** -25) == 0 and pin(1.5 * 2.0 ** -25) == 1 and pin(2.0 ** -25 * (1 + 2.0 ** -20)) == 1
    assert pin(1 + 2.0 ** -11) == 0x3C00 and pin(1 + 3 * 2.0 ** -11) == 0x3C02
    assert int(W.bf16_bits(np.array([1 + 2.0 ** -8], np.float32))[0]) == 0x3F80 and int(W.bf16_bits(np.array([1 + 3 * 2.0 ** -8], np.float32))[0]) == 0x3F82
    assert int(W.bf16_bits(np.array([-0.0], np.float32))[0]) == 0x8000
    assert int(W.f16_bits(np.array([np.nan], np.float32))[0]) == 0x7E00 and np.isnan(W.bf16_val(W.bf16_bits(np.array([np.nan], np.float32))))[0]


@pytest.mark.parametrize("K,D,mean", [(100, 80, -5.0), (500, 80, -5.0), (7, 3, 100.0)])
def test_codebook_tables_against_the_oracle(K, D, mean):
    """The oracle's tables in float64 (oracle/ref_cpu.py::codebook_tables).  u = 2^-24.  Centre: a sequential fp32 sum of K terms and one
    division, |c32 - c64| <= Ec = gamma(K) sum|c_k| / K + u |c64|, gamma(K) = K u / (1 - K u).  Centred: one subtraction from the rounded
    centre, Ev = Ec + u (|v64| + Ec).  raw = fl(fl(c - centre) + centre) against the centroid itself: u (|v32| + |c|) (1 + u).
    1 / norm: ||v32|| moves by at most ||Ev||_2; the root's fp32 rounding and the reciprocal's add 2.01 u relative."""
    c = (synth.synth_codebook(K, D, 11) + (mean + 5.0)).numpy()
    v32, raw, rn, centre = W.codebook_tables(c)
    c64, v64 = (t.numpy() for t in R.codebook_tables(torch.from_numpy(c).double()))
    gam = K * U / (1 - K * U)
    Ec = gam * np.abs(c.astype(np.float64)).sum(axis=0) / K + U * np.abs(c64)
    assert (np.abs(centre - c64) <= Ec).all()
    Ev = Ec[None, :] + U * (np.abs(v64) + Ec[None, :])
    assert (np.abs(v32 - v64) <= Ev).all()
    assert (np.abs(raw.astype(np.float64) - c) <= U * (np.abs(v32.astype(np.float64)) + np.abs(c)) * (1 + U)).all()
    n64 = np.sqrt((v64 ** 2).sum(axis=1))
    rel = np.sqrt((Ev ** 2).sum(axis=1)) / n64 + 2.01 * U
    assert (np.abs(rn * n64 - 1.0) <= rel * 1.001).all()           # (1.001: the second-order products of the terms above)
    # an all-equal codebook: centred = 0 and the norm is clamped at 1e-8
    assert np.array_equal(W.codebook_tables(np.zeros((4, 3), np.float32))[2], np.full(4, np.float32(1.0) / np.float32(1e-8), np.float32))


def test_permutation_property_of_the_fp32_form():
    """An address-coded checkpoint in the fp32 form: every source element is a distinct integer below 2^24, every module comes as
    plain `.weight`.  Packing only moves words: the non-zero words of each matrix are exactly its source's elements, nothing
    duplicated, nothing dropped (an upsampler with absent (phase, tap) pairs included, 11 taps at rate 5), its bias once per phase; every
    other word of the image is zero.  The codebook is zero: its tables are arithmetic, not a permutation (centred = raw = 0, 1 / norm = 1e8)."""
    from tests.cases import unit_arch
    harch = HubertArch.tiny(conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True, num_hidden_layers=1)
    varch = VocoderArch(upsample_rates=(5, 4), upsample_kernel_sizes=(11, 8), upsample_initial_channel=64, num_mels=40,
                        resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 3), (1, 3)))
    assert unit_arch().upsample_rates[0] == 5 and unit_arch().upsample_kernel_sizes[0] == 11
    d = native.make_desc(harch, varch, 10, "fp32", "fp32")
    sd, nxt = {}, 1
    for item in W.required(d):
        name, shape = (item[1] + ".weight" if item[0] == "module" else item[1]), item[2]
        n = int(np.prod(shape))
        sd[name] = np.zeros(shape, np.float32) if name == "codebook" else np.arange(nxt, nxt + n, dtype=np.float32).reshape(shape)
        nxt += 0 if name == "codebook" else n
    assert nxt < 2 ** 24
    out = W.pack(d, sd)
    L, img = out["layout"], np.concatenate([np.zeros(32, np.uint8), out["image"]])
    words = img.view(np.float32)

    def region(G):
        return words[G.w // 4:G.w // 4 + G.groups * G.ntaps * G.Npad * G.Cin]

    def same(reg, *names):
        got, want = np.sort(reg[reg != 0]), np.sort(np.concatenate([sd[n].reshape(-1) for n in names]))
        return got.size == want.size and np.array_equal(got, want)

    Bm, Gn = "base_model.", "generator."
    assert same(region(L.pre), Gn + "conv_pre.weight") and same(region(L.pos), Bm + "encoder.pos_conv_embed.conv.weight")
    assert same(region(L.layers[0].qkv), *[Bm + f"encoder.layers.0.attention.{n}_proj.weight" for n in "qkv"])
    assert same(region(L.head), "final_layers.1.weight") and same(region(L.convs[0].g), Bm + "feature_extractor.conv_layers.1.conv.weight")
    for i, u in enumerate(varch.upsample_rates):
        U_ = L.ups[i]
        assert same(region(U_), Gn + f"ups.{i}.weight")
        b = words[U_.bias // 4:U_.bias // 4 + U_.N]
        assert np.array_equal(b, np.tile(sd[Gn + f"ups.{i}.bias"], u))
    assert L.ups[0].ntaps == 3 and region(L.ups[0]).size > sd[Gn + "ups.0.weight"].size          # 11 = 2 * 5 + 1: four absent pairs per (co, ci)
    assert same(words[L.post_w // 4:L.post_w // 4 + 7 * L.post_C], Gn + "conv_post.weight")
    # the whole image: outside the codebook tables the non-zero words are the checkpoint, each once (upsampler biases once per phase)
    keep = np.ones(words.size, bool)
    keep[L.cb_centered // 4:L.cb_rnorm // 4 + d.num_clusters] = False
    keep[:64] = False
    got = np.sort(words[keep][words[keep] != 0])
    want = [a.reshape(-1) for n, a in sd.items() if n != "codebook"]
    want += [np.tile(sd[Gn + f"ups.{i}.bias"], u - 1) for i, u in enumerate(varch.upsample_rates)]
    assert np.array_equal(got, np.sort(np.concatenate(want)))
    assert (words[L.cb_centered // 4:L.cb_raw // 4 + 10 * 80] == 0).all() and (words[L.cb_rnorm // 4:L.cb_rnorm // 4 + 10] == 1e8).all()


@pytest.mark.parametrize("bug", W.BUGS)
def test_planted_mistake_changes_bytes(bug):
    harch, varch, sd = _pair()
    d = native.make_desc(harch, varch, 100, "fp32", "bf16x3")
    good = _GOOD.setdefault("img", W.pack(d, sd)["image"])
    bad = W.pack(d, sd, bug=(bug,))["image"]
    assert bad.size == good.size and not np.array_equal(bad, good)


_GOOD = {}
