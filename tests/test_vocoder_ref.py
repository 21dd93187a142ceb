"""The float64 references of tests/vocoder_ref.py pinned on the CPU: with unrounded weights and the rounding steps switched
off they reproduce the oracle's generator (ref_cpu.generator_forward run in float64, tapped at ups<i> / stage<i>) to 1e-12
relative on the V1, v3 and a one-stage u = 1 architecture; each bound accepts ref +- E and rejects the first fp16 value past it;
the packed leaky-ReLU emulation is checked on all 65536 bit patterns; the weight folding reproduces torch._weight_norm bit for
bit on the synthetic checkpoint."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from speech_inpainting_amd import synth
from speech_inpainting_amd.arch import VocoderArch
from tests import vocoder_ref as V


class _F64:
    """An entry whose `.float()` is float64: runs the oracle's functions in double precision unchanged."""

    def __init__(self, t):
        self.t = t.double()

    def float(self):
        return self.t


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _one_stage(C, u=1, k=3, rk=(3, 7, 11), dil=((1, 3, 5),) * 3, resblock="1"):
    return VocoderArch(resblock=resblock, upsample_rates=(u,), upsample_kernel_sizes=(k,), upsample_initial_channel=2 * C,
                       resblock_kernel_sizes=rk, resblock_dilation_sizes=dil)


ARCHS = {
    "v1": dataclasses.replace(VocoderArch.v1(), upsample_initial_channel=128),     # V1's rates and blocks at an eighth of the width
    "v3": dataclasses.replace(VocoderArch.v3(), upsample_initial_channel=64),
    "u1": _one_stage(32),
    # the I_da unit vocoder (hubert_lut.json) at its real widths: three taps per phase with empty slots (5, 11), k = 2 u at u = 4, 16 channels at the end
    "unit": VocoderArch(upsample_rates=(5, 4, 4, 2, 2), upsample_kernel_sizes=(11, 8, 8, 4, 4), upsample_initial_channel=512, num_mels=384,
                        sampling_rate=16000),
}


def _input(arch, B, Tm, seed):
    """A synthetic log-mel for 80 bins; the unit vocoder's 384 embedding channels as N(0, 0.5^2)."""
    if arch.num_mels == 80:
        return synth.synth_mel(B, Tm, 80, seed)
    return torch.randn(B, arch.num_mels, Tm, generator=torch.Generator().manual_seed(seed)) * 0.5


def _plain(x):
    return V.lrelu(x, 0.1)


def _generator_by_refs(sd, arch, mel):
    """The generator of one clip composed from the references, nothing rounded: mel (num_mels, Tm) -> ({name: (L, C)}, wave (L,))."""
    sd64 = {k: _F64(v) for k, v in sd.items()}
    f = lambda n: R._conv_weight(sd64, n)                                        # noqa: E731  (the fold itself in float64, as the oracle's run)
    taps = {}
    x, _ = V.tapconv_ref(mel.t().double(), f("conv_pre"), sd["conv_pre.bias"])
    nk = len(arch.resblock_kernel_sizes)
    for i, (u, k) in enumerate(zip(arch.upsample_rates, arch.upsample_kernel_sizes)):
        x, _ = V.upsample_ref(_plain(x), f(f"ups.{i}"), sd[f"ups.{i}.bias"], u)
        taps[f"ups{i}"] = x
        xs = None
        for j, (rk, dil) in enumerate(zip(arch.resblock_kernel_sizes, arch.resblock_dilation_sizes)):
            r = f"resblocks.{i * nk + j}."
            if arch.resblock == "2":
                y = x
                for n, d in enumerate(dil):
                    last = n == len(dil) - 1
                    y, E = V.rb2_ref(_plain(y), y, f(f"{r}convs.{n}"), sd[f"{r}convs.{n}.bias"], d, 1.0 / nk if last else 1.0,
                                     xs if last else None)
                xs = y
            else:
                pairs = [(f(f"{r}convs1.{n}"), sd[f"{r}convs1.{n}.bias"], f(f"{r}convs2.{n}"), sd[f"{r}convs2.{n}.bias"], d)
                         for n, d in enumerate(dil)]
                xs, E = V.chain_ref(x, pairs, 1.0 / nk, xs, staged=_plain, round_x=False, t_slope=0.1)
            assert bool((E > 0).all())
        x = xs
        taps[f"stage{i}"] = x
    wave, E = V.conv_post_ref(x, f("conv_post"), sd["conv_post.bias"], mfma=False, slope=0.01)
    assert bool((E > 0).all())
    return taps, wave


@pytest.mark.parametrize("name", list(ARCHS))
def test_references_reproduce_the_oracle_generator(name):
    arch = ARCHS[name]
    sd = synth.synth_generator_state(arch)
    B, Tm = 2, (3 if name == "unit" else 13)
    mel = _input(arch, B, Tm, 5)
    want_taps = {}
    want = R.generator_forward({k: _F64(v) for k, v in sd.items()}, arch, _F64(mel), want_taps)
    assert want.dtype == torch.float64 and want.shape == (B, 1, Tm * arch.hop)
    for b in range(B):
        taps, wave = _generator_by_refs(sd, arch, mel[b])
        for nm, t in taps.items():
            assert _rel(t, want_taps[nm][b].t()) <= 1e-12, (name, nm)
        assert _rel(wave, want[b, 0]) <= 1e-12


def test_u1_arch_is_one_stage_at_the_mel_rate():
    arch = ARCHS["u1"]
    sd = synth.synth_generator_state(arch)
    for Tm in (1, 2, 255):
        taps = {}
        out = R.generator_forward(sd, arch, synth.synth_mel(1, Tm, 80, 6), taps)
        assert out.shape == (1, 1, Tm) and taps["stage0"].shape == (1, 32, Tm)


def test_packed_leaky_relu_on_every_bit_pattern():
    """lrelu16 against max(h, h * fp16(slope)) evaluated in float64 and rounded ONCE to fp16, on all 65536 patterns (NaNs stay NaN)."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    h = bits.view(torch.float16)
    for slope in (0.1, 0.01):
        s16 = float(torch.tensor(slope).to(torch.float16))
        assert s16 == (0.0999755859375 if slope == 0.1 else float(np.float16(0.01)))
        got = V.lrelu16(h, slope)
        hd = h.double()
        prod = V.rne_f16(hd * s16)
        want = torch.where(hd > prod, hd, prod)
        want = torch.where(torch.isinf(hd), hd, want)
        nan = torch.isnan(hd)
        assert bool(torch.isnan(got.double())[nan].all())
        assert torch.equal(got.double()[~nan], want[~nan])
        # and it is NOT the fp32 form rounded once: the two differ on some pattern (a kernel that staged that way would read other operands)
        other = V.lrelu(hd, V.SLOPE32).float().to(torch.float16).double()
        assert int((other[~nan] != want[~nan]).sum()) > 0


def test_weight_folding_is_torch_weight_norm_bit_for_bit():
    """fold's operation order is torch._weight_norm's: with torch's own fp32 norm it reproduces torch._weight_norm(...).half() bit
    for bit.  With the packer's norm (squares summed in double, one rounding) the fp32 weight is within the error of torch's fp32 norm
    and the fp16 weight is the same or, on fewer than one in 10^3, the neighbouring fp16 value."""
    for arch in (VocoderArch.v1(), ARCHS["v3"], ARCHS["u1"]):
        sd = synth.synth_generator_state(arch)
        names = sorted({k[:-len(".weight_g")] for k in sd if k.endswith(".weight_g")})
        assert names
        for n in names:
            want32 = torch._weight_norm(sd[n + ".weight_v"], sd[n + ".weight_g"], 0)
            want = want32.half().double()
            assert torch.equal(V.fold(sd, n, norm="torch"), want), n
            assert torch.equal(V.fold(sd, n, round16=False, norm="torch"), want32.double()), n
            got32 = V.fold(sd, n, round16=False)
            # torch's norm sums n squares in fp32 (relative error <= n 2^-24 in any order, halved by the square root); two roundings behind it
            n_row = want32[0].numel()
            assert bool(((got32 - want32.double()).abs() <= (n_row * 2.0 ** -25 + 2.0 ** -22) * want32.double().abs()).all()), n
            got = V.fold(sd, n)
            diff = got != want
            assert int(diff.sum()) <= max(2, diff.numel() // 1000) and bool(((got - want).abs()[diff] == V.ulp_f16(torch.minimum(got.abs(), want.abs()))[diff]).all()), n
        folded = synth.synth_generator_state(arch, folded=True)
        assert torch.equal(V.fold(folded, "conv_pre"), folded["conv_pre.weight"].half().double())


def _bound_accepts_and_rejects(ref, E, f16=True):
    """The last representable value inside ref +- E passes; the first one past it fails, on every element and both sides."""
    check = V.check_f16 if f16 else V.check_f32
    for sgn in (1.0, -1.0):
        edge = ref + sgn * E
        if f16:
            q = V.ulp_f16(edge)
            inside = torch.floor(edge / q) * q if sgn > 0 else torch.ceil(edge / q) * q
            inside = torch.where((inside - ref).abs() <= E, inside, inside - sgn * q)
            beyond = V.next_f16(inside, ref)
        else:
            far = torch.full_like(edge, sgn * 4.0).float()
            inside = edge.float()
            inside = torch.where((inside.double() - ref).abs() <= E, inside, torch.nextafter(inside, -far))
            beyond = torch.nextafter(inside, far).double()
            inside = inside.double()
        assert bool(((beyond - ref).abs() > E).all()) and bool(((inside - ref).abs() <= E).all())
        assert check(inside, ref, E)["bad"] == 0
        r = check(beyond, ref, E)
        assert r["bad"] == ref.numel(), (r["bad"], ref.numel())


def _operands(C, L, k, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(L, C, generator=g) * scale).to(torch.float16)
    w = lambda: V.h16(torch.randn(C, C, k, generator=g) / (C * k) ** 0.5)       # noqa: E731
    b = lambda: torch.randn(C, generator=g) * 0.05                              # noqa: E731
    return y, w, b


@pytest.mark.parametrize("C,k,dil", [(32, 3, 1), (64, 7, 3), (32, 11, 5)])
def test_every_bound_accepts_its_edge_and_rejects_the_next_value(C, k, dil):
    y, w, b = _operands(C, 40, k, 3)
    a = V.lrelu16(y).double()
    prev = torch.randn(40, C).to(torch.float16).double()
    cases = {
        "tapconv": V.tapconv_ref(a, w(), b(), dil),
        "tapconv activated": V.tapconv_ref(a, w(), b(), dil, out_slope=V.SLOPE32),
        "pair": V.pair_ref(a, y.double(), w(), b(), w(), b(), dil),
        "pair alpha acc": V.pair_ref(a, y.double(), w(), b(), w(), b(), dil, V.alpha32(3), prev),
        "pair activated": V.pair_ref(a, y.double(), w(), b(), w(), b(), dil, V.alpha32(3), prev, out_slope=V.SLOPE32),
        "rb2": V.rb2_ref(a, y.double(), w(), b(), dil, V.alpha32(3), prev),
        "chain": V.chain_ref(y.double(), [(w(), b(), w(), b(), d) for d in (1, 3, 5)], V.alpha32(3), prev),
    }
    g = torch.Generator().manual_seed(9)
    wt = V.h16(torch.randn(C, C // 2, 4, generator=g) / (2 * C) ** 0.5)
    cases["upsample"] = V.upsample_ref(a, wt, torch.randn(C // 2, generator=g) * 0.05, 2)
    for name, (ref, E) in cases.items():
        assert bool((E > 0).all()) and bool(torch.isfinite(ref).all()), name
        assert float(E.max()) < 1e-2 * float(ref.abs().max()), name                # a bound, not a blanket
        _bound_accepts_and_rejects(ref, E)
    wp = torch.randn(1, C, 7, generator=g) / (7 * C) ** 0.5
    for mfma in (True, False):
        ref, E = V.conv_post_ref(y, wp, torch.tensor([0.01]), mfma)
        assert ref.shape == (40,) and float(E.max()) < 2e-3
        _bound_accepts_and_rejects(ref, E, f16=False)
    m, _ = V.conv_post_ref(y, wp, torch.tensor([0.01]), True)
    f, _ = V.conv_post_ref(y, wp, torch.tensor([0.01]), False)
    assert 0 < float((m - f).abs().max()) < 2e-3                                  # fp16 weights and slope: different, and close


def test_pair_reference_with_t_rounded_stays_inside_the_bound_of_the_unrounded_one():
    """The bound's dt term covers the kernel's rounding of t: the reference evaluated WITH t rounded lies inside E of the one without."""
    y, w, b = _operands(32, 64, 7, 4, scale=30.0)
    a = V.lrelu16(y).double()
    ws = (w(), b(), w(), b())
    ref, E = V.pair_ref(a, y.double(), *ws, 3)
    ref_t, _ = V.pair_ref(a, y.double(), *ws, 3, round_t=True)
    assert float((ref_t - ref).abs().max()) > 0 and bool(((ref_t - ref).abs() <= E).all())
    assert V.check_f16(V.rne_f16(ref_t), ref, E)["bad"] == 0


def test_saturation_rule():
    ref = torch.tensor([70000.0, -70000.0, 65500.0, 65500.0, 100.0, 70000.0])
    E = torch.tensor([10.0, 10.0, 40.0, 40.0, 1.0, 10.0])
    got = torch.tensor([65504.0, -65504.0, 65504.0, 65472.0, 100.5, 65472.0])
    r = V.check_f16(got, ref, E)
    assert r["ok"].tolist() == [True, True, True, True, True, False] and r["saturated"] == 4
    assert V.check_f16(torch.tensor([65504.0]), torch.tensor([-70000.0]), torch.tensor([10.0]))["bad"] == 1


def test_seam_distance_and_report():
    seam, edge = V.seam_distance(10, 4)
    assert seam.tolist() == [3, 2, 1, 0, 0, 1, 1, 0, 0, 1] and edge.tolist() == [0, 1, 2, 3, 4, 4, 3, 2, 1, 0]
    assert V.seam_distance(4, 4)[0].tolist() == [4] * 4
    ref = torch.zeros(10, 2, dtype=torch.float64)
    E = torch.ones(10, 2, dtype=torch.float64)
    got = ref.clone()
    got[4, 1] = 3.0
    line, near, rest = V.report("op", "kern", 1, V.check_f16(got, ref, E), 10, 4, 0)
    assert "FAILED" in line and "row 4, channel 1, 0 rows from a tile seam, 4 from the clip edge, err/E 3.000" in line and near == 3.0 and rest == 0.0


# ------------------------------------------------------------------------------- the tap-GEMM on an fp32 activation stream
def _generator_by_tapgemm_ref(sd, arch, mel, math="f64"):
    """The ResBlock1 generator of one clip composed from tapgemm_ref the way api.hip's forward launches it (conv_pre, the upsampler
    as a transposed conv, conv 1, conv 2 with residual / alpha / accumulate): mel (80, Tm) -> {name: (L, C)}."""
    sd64 = {k: _F64(v) for k, v in sd.items()}
    f = (lambda n: R._conv_weight(sd64, n)) if math == "f64" else (lambda n: V.fold(sd, n, round16=False).float())      # noqa: E731
    nk = len(arch.resblock_kernel_sizes)
    alpha = 1.0 / nk if math == "f64" else V.alpha32(nk)
    slope = 0.1 if math == "f64" else V.SLOPE32
    cast = (lambda t: t) if math == "f64" else (lambda t: t.float())                                                    # noqa: E731
    taps = {}
    w = f("conv_pre")
    x = cast(V.tapgemm_ref(mel.t(), w, sd["conv_pre.bias"], math, V.conv_geom(1), 7 * arch.num_mels).ref)
    taps["pre"] = x
    for i, (u, k) in enumerate(zip(arch.upsample_rates, arch.upsample_kernel_sizes)):
        w = f(f"ups.{i}")
        x = cast(V.tapgemm_ref(x, w, sd[f"ups.{i}.bias"], math, V.tconv_geom(u), -(-k // u) * w.shape[0], slope=slope).ref)
        taps[f"ups{i}"] = x
        xs = None
        for j, (rk, dil) in enumerate(zip(arch.resblock_kernel_sizes, arch.resblock_dilation_sizes)):
            r = f"resblocks.{i * nk + j}."
            y = x
            for n, d in enumerate(dil):
                last = n == len(dil) - 1
                K = rk * y.shape[1]
                t = cast(V.tapgemm_ref(y, f(f"{r}convs1.{n}"), sd[f"{r}convs1.{n}.bias"], math, V.conv_geom(d), K, slope=slope).ref)
                y = cast(V.tapgemm_ref(t, f(f"{r}convs2.{n}"), sd[f"{r}convs2.{n}.bias"], math, V.conv_geom(1), K, slope=slope, res=y,
                                       alpha=alpha if last else 1.0, prev=xs if (last and j > 0) else None).ref)
            xs = y
        x = xs
        taps[f"stage{i}"] = x
    return taps


@pytest.mark.parametrize("name", ["v1", "u1", "unit"])
def test_tapgemm_ref_reproduces_the_oracle_generator(name):
    """math = "f64" (nothing rounded) is the oracle's generator to 1e-12; the three arithmetics stay within their modes' distance of it."""
    arch = ARCHS[name]
    sd = synth.synth_generator_state(arch)
    mel = _input(arch, 2, 3 if name == "unit" else 11, 5)
    want = {}
    R.generator_forward({k: _F64(v) for k, v in sd.items()}, arch, _F64(mel), want)
    for b in range(2):
        taps = _generator_by_tapgemm_ref(sd, arch, mel[b])
        for nm in want:
            assert _rel(taps[nm], want[nm][b].t()) <= 1e-12, (name, nm)
    for math, tol in (("f32", 1e-5), ("bf16x3", 1e-4), ("bf16", 5e-2)):
        taps = _generator_by_tapgemm_ref(sd, arch, mel[0], math)
        for nm in want:
            assert _rel(taps[nm].double(), want[nm][0].t()) <= tol, (name, math, nm)


def _h_f2bf(v):
    """Packer's h_f2bf restated on the bit patterns: u += 0x7FFF + ((u >> 16) & 1); u >> 16 (finite inputs)."""
    u = v.float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16) << 16


def test_bf16_split_is_the_packers_and_the_kernels():
    """bf16r is h_f2bf (api.hip) on random values and on exact ties; split_bf16's lo plane is h_f2bf(v - bf2f(hi)); hi + lo leaves
    |r| <= 2^-16 |v| and |lo| <= 2^-8 (1 + 2^-8) |v| (two roundings to 8 significant bits), the figures E_exact's closed form rests on."""
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.randn(20000, generator=g) * 3, torch.randn(2000, generator=g) * 1e-4,
                   torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 2.0 ** -20 * (1 + 2.0 ** -8), 0.0])])
    bits = _h_f2bf(v)
    want = (bits & 0xFFFFFFFF).to(torch.int64)
    got = V.bf16r(v).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got, want)
    assert V.bf16r(torch.tensor([1.0 + 2.0 ** -8])).item() == 1.0 and V.bf16r(torch.tensor([1.0 + 3 * 2.0 ** -8])).item() == 1.0 + 2.0 ** -6
    hi, lo = V.split_bf16(v)
    assert torch.equal(hi, V.bf16r(v).double())
    rem32 = v - V.bf16r(v)
    assert torch.equal(rem32.double(), v.double() - hi), "the fp32 subtraction v - hi is exact"
    assert torch.equal((_h_f2bf(rem32) & 0xFFFFFFFF), lo.float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF)
    r = v.double() - hi - lo
    assert bool((lo.abs() <= 2.0 ** -8 * (1 + 2.0 ** -8) * v.double().abs()).all()) and bool((r.abs() <= 2.0 ** -16 * v.double().abs()).all())


def _tg_case(C, k, dil, L, seed, Cout=None):
    g = torch.Generator().manual_seed(seed)
    Cout = Cout or C
    x = torch.randn(L, C, generator=g)
    w = torch.randn(Cout, C, k, generator=g) / (C * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.05
    res = torch.randn(L, Cout, generator=g)
    prev = torch.randn(L, Cout, generator=g)
    return x, w, b, res, prev


def _emulate(x, w, b, math, contract, slope=1.0, res=None, alpha=1.0, prev=None, drop=(), slope_after=False):
    """What a kernel would store, with its accumulation done in float32 on the CPU (a different order from any MFMA's, within the
    same gamma): the operand planes as fp32 tensors, contracted in fp32, summed lo-terms first, the epilogue in fp32 in the kernel's
    order.  drop / slope_after: the mistakes."""
    v = V.lrelu32(x, slope)
    wf = w.float()
    if math == "f32":
        planes = [("v*w", v, wf)]
    elif math == "bf16":
        a = V.bf16r(V.lrelu32(V.bf16r(x), slope)) if slope_after else V.bf16r(v)
        planes = [("hi*hi", a, V.bf16r(wf))]
    else:
        vh, wh = V.bf16r(v), V.bf16r(wf)
        planes = [("lo*hi", V.bf16r(v - vh), wh), ("hi*lo", vh, V.bf16r(wf - wh)), ("hi*hi", vh, wh)]
    acc = None
    for nm, a, ww in planes:
        if nm in drop:
            continue
        t = contract(a, ww)
        assert t.dtype == torch.float32
        acc = t if acc is None else acc + t
    out = acc + b.float()
    if res is not None:
        out = out + res.float()
    out = out * torch.tensor(alpha, dtype=torch.float32)
    if prev is not None:
        out = out + prev.float()
    return out


MATHS = ("f32", "bf16x3", "bf16")


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("C,k,dil", [(32, 3, 1), (64, 7, 3), (32, 11, 5)])
def test_tapgemm_bounds_hold_for_an_fp32_evaluation_and_reject_every_listed_mistake(math, C, k, dil):
    """An honest fp32 evaluation of the same operation lies inside E (and, for bf16x3, inside E_exact of the fp32 product); each
    mistake the bounds exist for lands outside on at least one element: a dropped bf16x3 cross term, a tap shifted by one row,
    a dilation off by one, the slope applied after the bf16 rounding, alpha omitted, the last valid row of a 128-row tile zeroed."""
    L = 150
    x, w, b, res, prev = _tg_case(C, k, dil, L, 11 + C + k)
    a3 = V.alpha32(3)
    geom = V.conv_geom(dil)
    kw = dict(slope=V.SLOPE32, res=res, alpha=a3, prev=prev)
    r = V.tapgemm_ref(x, w, b, math, geom, k * C, **kw)
    assert bool((r.E > 0).all()) and float(r.E.max()) < 1e-3 * float(r.ref.abs().max())            # a bound, not a blanket

    def bad(got, exact=False):
        return V.check_f32(got, r.exact if exact else r.ref, r.E_exact if exact else r.E)["bad"]

    good = _emulate(x, w, b, math, geom, **kw)
    assert bad(good) == 0
    assert bad(r.ref.float()) == 0
    if math != "bf16":
        assert bad(good, exact=True) == 0
    if math == "bf16x3":
        # the split's distance to the fp32 product is inside its computed part of E_exact, and that part is small: <= 3.1 * 2^-16 S
        S = V.conv_geom(dil)(V.lrelu32(x, V.SLOPE32).double().abs(), w.double().abs())
        assert bool(((r.ref - r.exact).abs() <= r.E_exact - r.E + 1e-18).all())
        assert bool((r.E_exact - r.E <= a3 * 3.1 * 2.0 ** -16 * S * (1 + 1e-6)).all())
        for term in ("lo*hi", "hi*lo"):
            assert bad(_emulate(x, w, b, math, geom, drop=(term,), **kw)) > 0, term
            assert bad(V.tapgemm_ref(x, w, b, math, geom, k * C, drop=(term,), **kw).ref.float()) > 0, term
    assert bad(_emulate(x, w, b, math, V.conv_geom(dil, shift=1), **kw)) > 0
    assert bad(_emulate(x, w, b, math, V.conv_geom(dil + 1), **kw)) > 0
    assert bad(_emulate(x, w, b, math, geom, slope=V.SLOPE32, res=res, alpha=1.0, prev=prev)) > 0
    zeroed = good.clone()
    zeroed[127] = 0.0
    assert bad(zeroed) > 0
    if math == "bf16":
        assert bad(_emulate(x, w, b, math, geom, slope_after=True, **kw)) > 0
    # the same layer as a transposed convolution (u = 2, k = 4; two taps per phase): honest inside, a shifted phase outside
    g = torch.Generator().manual_seed(5)
    wt = torch.randn(C, C // 2, 4, generator=g) / (2 * C) ** 0.5
    bt = torch.randn(C // 2, generator=g) * 0.05
    rt = V.tapgemm_ref(x, wt, bt, math, V.tconv_geom(2), 2 * C, slope=V.SLOPE32)
    up = _emulate(x, wt, bt, math, V.tconv_geom(2), slope=V.SLOPE32)
    assert up.shape == (2 * L, C // 2) and V.check_f32(up, rt.ref, rt.E)["bad"] == 0
    assert V.check_f32(torch.roll(up, 1, 0), rt.ref, rt.E)["bad"] > 0


# ------------------------------------------------------------------------------- the unit vocoder's geometry: (5, 11), (4, 8), 16 channels
def _by_phases(a, w, b, u, swap=False, pad=None, crop=True, fill=False):
    """ConvTranspose1d the way the kernels run it, in float32: tap j of the kernel is slot (tap q = j div u, phase p = j mod u); input row i
    adds a[i] w[:, :, j] to row u (i + q) + p of the uncropped result (GEMM row m = i + q reads input rows m, m - 1, ...), slots j >= k hold
    zero weights, and the first `pad` = (k - u) / 2 rows are cropped (ooff = -pad Cout) to leave u Lin rows.  a (Lin, Cin) and w (Cin, Cout, k)
    float32.  The mistakes: swap -- phase and tap exchanged (j mod u for j div u); pad -- another crop; crop=False -- ooff = 0; fill -- an empty
    (phase, tap) slot filled with the neighbouring tap's weight of the same phase."""
    Lin, k = a.shape[0], w.shape[2]
    ntaps = -(-k // u)
    p0 = (k - u) // 2 if pad is None else pad
    full = torch.zeros(u * (Lin + max(ntaps, u)) + u, w.shape[1], dtype=torch.float32)
    for j in range(ntaps * u):
        if j < k:
            wj = w[:, :, j]
        elif fill:
            wj = w[:, :, j - u]
        else:
            continue
        q, p = (j % u, j // u) if swap else (j // u, j % u)
        rows = u * (torch.arange(Lin) + q) + p
        full.index_add_(0, rows, a @ wj)
    off = p0 if crop else 0
    return full[off:off + u * Lin] + b.float()


UPS_GEOM = [(5, 11, 64, 32), (4, 8, 64, 32), (5, 11, 32, 16)]


@pytest.mark.parametrize("u,k,Cin,Cout", UPS_GEOM)
def test_upsampler_bounds_at_the_unit_vocoders_geometry(u, k, Cin, Cout):
    """(5, 11) and (4, 8): upsample_ref / tconv_geom are F.conv_transpose1d; a float32 evaluation by phases and taps (fp16 operands and an
    fp16 store for the fp16 stream, fp32 operands for the tap-GEMM's exact path) stays inside the bound at Lin = 1, 2, 5, 7 and 40, and each
    mistake of the phase / tap / crop bookkeeping lands outside it."""
    g = torch.Generator().manual_seed(100 + u)
    w32 = torch.randn(Cin, Cout, k, generator=g) / (Cin * k / u) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.05
    pad = (k - u) // 2
    for Lin in (1, 2, 5, 7, 40):
        x16 = torch.randn(Lin, Cin, generator=g).to(torch.float16)
        a = V.lrelu16(x16).double()
        ref, E = V.upsample_ref(a, V.h16(w32), b, u)
        assert ref.shape == (u * Lin, Cout)
        want = torch.nn.functional.conv_transpose1d(a.t()[None], V.h16(w32), b.double(), stride=u, padding=pad)[0].t()
        assert torch.equal(ref, want)
        w16 = V.h16(w32).float()

        def bad16(**kw):
            return V.check_f16(_by_phases(a.float(), w16, b, u, **kw).to(torch.float16), ref, E)["bad"]

        x32 = x16.float() * 1.37
        r = V.tapgemm_ref(x32, w32, b, "f32", V.tconv_geom(u), -(-k // u) * Cin, slope=V.SLOPE32)

        def bad32(**kw):
            return V.check_f32(_by_phases(V.lrelu32(x32, V.SLOPE32), w32, b, u, **kw), r.ref, r.E)["bad"]

        for bad in (bad16, bad32):
            assert bad() == 0
            assert bad(swap=True) > 0
            assert bad(pad=pad - 1) > 0 and bad(pad=pad + 1) > 0
            assert bad(crop=False) > 0
            if k % u and Lin >= 2:               # (tap 2 of GEMM row m reads input row m - 2: with one input row an empty slot meets zeros only)
                assert bad(fill=True) > 0


def test_padded_stage_rejects_a_non_zero_value_in_channel_16():
    """The fp16 stream's 16-channel stage at 32: real_channels hands back the 16 real channels and refuses any non-zero value in the padding,
    down to the smallest subnormal; -0 is zero."""
    t = torch.zeros(5, 32, dtype=torch.float16)
    t[:, :16] = 1.5
    t[3, 20] = -0.0
    assert torch.equal(V.real_channels(t, 16), t[:, :16])
    t[2, 16] = 2.0 ** -24
    with pytest.raises(AssertionError, match="not exactly zero"):
        V.real_channels(t, 16, "stage")
    assert V.real_channels(t, 32) is not None


def _compose16(arch, sd, mel):
    """The fp16 stream of one clip composed from the references (the packer's fp16 weights, every stored tensor rounded to fp16 as the next
    kernel reads it; hand-offs unactivated, which is the larger value): -> {tensor name: max |ref|} over every stored tensor."""
    out = {}
    nk = len(arch.resblock_kernel_sizes)

    def keep(name, ref):
        out[name] = float(ref.abs().max())
        return V.rne_f16(ref.clamp(-V.F16_MAX, V.F16_MAX)).to(torch.float16)

    x = keep("pre", V.tapconv_ref(V.h16(mel.t().clamp(-V.F16_MAX, V.F16_MAX)), V.fold(sd, "conv_pre"), sd["conv_pre.bias"])[0])
    for i, u in enumerate(arch.upsample_rates):
        x = keep(f"ups{i}", V.upsample_ref(V.lrelu16(x).double(), V.fold(sd, f"ups.{i}"), sd[f"ups.{i}.bias"], u)[0])
        xs = None
        for j, dils in enumerate(arch.resblock_dilation_sizes):
            r = f"resblocks.{i * nk + j}."
            y = x
            for n, d in enumerate(dils):
                last = n == len(dils) - 1
                ref = V.pair_ref(V.lrelu16(y).double(), y.double(), V.fold(sd, f"{r}convs1.{n}"), sd[f"{r}convs1.{n}.bias"], V.fold(sd, f"{r}convs2.{n}"),
                                 sd[f"{r}convs2.{n}.bias"], d, V.alpha32(nk) if last else 1.0, xs.double() if (last and xs is not None) else None)[0]
                y = keep(f"stage{i}.rb{j}.p{n}", ref)
            xs = y
        x = xs
    return out


def test_every_fp16_input_of_the_unit_vocoder_tests_stays_far_from_saturation():
    """tests/test_gpu_unitvoc_ops.py checks every element as an ordinary bound only where max |ref| < 65504 / 4 (`_one` asserts it on the
    device): here the same inputs (architecture, seed, frames), composed on the CPU for the clips the GPU test checks, one clip per distinct
    (architecture, seed, length)."""
    from tests.cases import _mel, _state, fp16_inputs
    torch.set_num_threads(min(16, torch.get_num_threads()))
    seen, worst = set(), 0.0
    for tag, arch, seed, lens, Tm, clips in fp16_inputs():
        sd = _state(arch)
        mel = _mel(1 if lens is None else len(lens), Tm if lens is None else max(lens), seed, arch.num_mels)
        for b in ([0] if lens is None else (clips if clips is not None else range(len(lens)))):
            L = Tm if lens is None else lens[b]
            if (repr(arch), seed, b, L) in seen:
                continue
            seen.add((repr(arch), seed, b, L))
            for name, m in _compose16(arch, sd, mel[b, :, :L]).items():
                worst = max(worst, m)
                assert m < V.F16_MAX / 4, (tag, b, L, name, m)
    print(f"   largest |ref| over every tensor of {len(seen)} clips: {worst:.1f}")
