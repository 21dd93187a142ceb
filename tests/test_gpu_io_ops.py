"""The kernels that take a file in, push PCM out and feed the unit vocoder, one by one against their float64 definitions
(tests/io_ref.py): resample_poly_kernel, resample_sinc_kernel, pcm16_kernel, extend_mel_cf_kernel / extend_mel_kernel,
unit_frontend_kernel, and the two routes of si_f0_encoder_forward (f0enc_fused_kernel | 37 x small_conv1d_kernel).

Every comparison is element-wise, |got - ref| <= E with E from the reference's own operands (io_ref's docstring derives each E), at the
sizes where these kernels take another path: one and two inputs, an input shorter than the filter's reach, the 256-output block seam,
the row stride of a batch, a base off the vector grid, an index outside its table, the LDS limit between the two F0 routes.
tests/test_io_ref.py shows on the CPU that the references alone stay inside E at these very cases and that seeded mistakes do not.
max err / E is noted per kernel, near-edge outputs (tap window cut by an end of the input, by a clamp, or next to a block seam) | the
rest, and printed by the last test.

MEASURED (MI355X) -- max err / E, near-edge | rest:
    resample_poly   0.8689 | 0.2211 over 35 checks (the fp32 chain alone on the CPU: 0.87)
    resample_sinc   0.9794 | 0.9797 over 78 checks (the final cast alone: 0.98)
    extend_mel      0.5924 | 0.6490 over 7 checks (the oracle's fp32 statement: 0.65)
    pcm16, unit_frontend: exact.  Stretch outputs not bit-identical to the oracle's extend_mel: 0 of 262 080.
    F0 routes: T = 876, 877 one f0enc_fused launch; T = 878, 879 37 f0enc_conv1d launches; m_conv 2, stride 3, in_width 2, down_t 1
    one fused launch at T = 16, 17, 33, 200; width 12 the 37 launches.  No kernel or launcher needed a fix.
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from speech_inpainting_amd import audio, native, synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from speech_inpainting_amd.engine import pack_f0_encoder
from speech_inpainting_amd.native import NativeError
from tests import io_ref as IO
from tests.common import rms
from tests.harness import RatioSummary, build_engine, scoped_env

pytestmark = pytest.mark.gpu

SUMMARY = RatioSummary()
NOT_BIT_IDENTICAL = {}                                     # Tm -> (stretch outputs that differ from the oracle's bits, outputs)
ROUTES = {}                                                # F0 case -> the route its profile showed
B = 3


def _engine():
    return build_engine(HubertArch.tiny(), VocoderArch.tiny(), 10, key="test_gpu_io_ops")


def _ctx():
    return _engine().ctx


def _profiled(fn):
    """fn() with the context's launches counted -> (result or None, the NativeError or None, {kernel family: launches})."""
    ctx = _ctx()
    out = err = None
    ctx.profile_start(4000)
    try:
        out = fn()
    except NativeError as e:
        err = e
    finally:
        prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
    return out, err, prof


def _rates_id(r):
    return f"{r[0]}to{r[1]}"


# ------------------------------------------------------------------------------------------------------------ polyphase resampler
def _poly_gpu(x, taps, up, down, pre, n_out):
    return _ctx().resample_poly(torch.from_numpy(x).cuda(), torch.from_numpy(taps).cuda(), up, down, pre, n_out).cpu().numpy()


@pytest.mark.parametrize("rates", list(IO.POLY_CASES), ids=_rates_id)
def test_resample_poly_at_one_input_the_filter_reach_and_the_block_seam(rates):
    """Three different clips per size (a wrong row stride shows), every output under E; and against scipy.signal.resample_poly itself,
    which filters with the float64 taps: E + 2^-24 S."""
    from scipy.signal import resample_poly
    for n_in in IO.POLY_CASES[rates]:
        x = IO.clips(B, n_in, 100 + n_in)
        taps, up, down, pre, n_out = audio.design_resampler(*rates, n_in)
        y, S, K, near = IO.poly_ref(x, taps, up, down, pre, n_out)
        got = _poly_gpu(x, taps, up, down, pre, n_out)
        assert got.shape == y.shape == (B, n_out)
        E = IO.poly_bound(S, K)
        a, b = IO.ratios(got, y, E, near)
        print(f"   {rates} n_in={n_in} n_out={n_out} K<={int(K.max())}: err / E near-edge {a:.4f}, rest {b:.4f}")
        SUMMARY.note("resample_poly", a, b)
        assert max(a, b) <= 1.0, (rates, n_in, a, b)
        sci = resample_poly(x.astype(np.float64), up, down, axis=1, window=("kaiser", audio.KAISER_BETA))
        assert (np.abs(got - sci) <= E + IO.U24 * S + 1e-13).all(), (rates, n_in, float(np.abs(got - sci).max()))


@pytest.mark.parametrize("rates", list(IO.POLY_CASES), ids=_rates_id)
def test_resample_poly_of_an_impulse_is_the_tap_table_bit_for_bit(rates):
    """x = delta at j0: y[m] = taps[(m + pre) down - j0 up], 0 outside the table -- every other term is fmaf(h, 0, acc)."""
    for n_in in IO.POLY_CASES[rates]:
        taps, up, down, pre, n_out = audio.design_resampler(*rates, n_in)
        j0s = sorted({0, n_in - 1, n_in // 2})
        got = _poly_gpu(np.concatenate([IO.impulse(n_in, j0) for j0 in j0s]), taps, up, down, pre, n_out)
        for row, j0 in zip(got, j0s):
            k = (np.arange(n_out) + pre) * down - j0 * up
            want = np.where((k >= 0) & (k < taps.size), taps[np.clip(k, 0, taps.size - 1)], np.float32(0.0))
            assert np.array_equal(row, want), (rates, n_in, j0, int((row != want).sum()))


def test_resample_poly_refuses_a_tap_table_larger_than_lds_before_any_launch():
    taps, up, down, pre, n_out = audio.design_resampler(22050, 16001, 16)
    assert taps.size * 4 > 150 * 1024
    x = torch.from_numpy(IO.clips(1, 16, 1)).cuda()
    t = torch.from_numpy(taps).cuda()
    _, err, prof = _profiled(lambda: _ctx().resample_poly(x, t, up, down, pre, n_out))
    assert err is not None and "ntaps" in str(err), err
    assert prof == {}, prof


# ------------------------------------------------------------------------------------------------------------ sinc resampler
def _sinc_gpu(x, f, lens=None, n_out=None):
    dev = {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in f.items()}
    n_len = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
    return _ctx().resample_sinc(torch.from_numpy(np.ascontiguousarray(x)).cuda(), dev, f["n_out"] if n_out is None else n_out, n_len).cpu().numpy()


@pytest.mark.parametrize("rates", list(IO.SINC_CASES), ids=_rates_id)
def test_resample_sinc_from_one_input_to_past_the_block_seam(rates):
    """Clips shorter than the window (both wings cut at once, by large taps), ratios whose accumulated times are integers, the zero
    fill from int(n_in ratio) to the row stride; impulses at the first and the last input under the same E."""
    for n_in in IO.SINC_CASES[rates]:
        f = IO.sinc_filter(*rates, n_in)
        live = int(n_in * f["ratio"])
        for what, x in (("clips", IO.clips(B, n_in, 200 + n_in)), ("impulses", np.concatenate([IO.impulse(n_in, j) for j in sorted({0, n_in - 1})]))):
            y, S, K, near = IO.sinc_ref(x, f, n_in)
            got = _sinc_gpu(x, f)
            assert got.shape == y.shape == (x.shape[0], f["n_out"])
            a, b = IO.ratios(got, y, IO.sinc_bound(y, S, K), near)
            print(f"   {rates} n_in={n_in} live={live} of {f['n_out']} {what}: err / E near-edge {a:.4f}, rest {b:.4f}")
            SUMMARY.note("resample_sinc", a, b)
            assert max(a, b) <= 1.0, (rates, n_in, what, a, b)
            assert not got[:, live:].any()                 # exactly zero, not merely inside E


@pytest.mark.parametrize("rates,n", [((22050, 16000), 90), ((22050, 16000), 354), ((48000, 16000), 770), ((8000, 16000), 129)],
                         ids=lambda v: _rates_id(v) if isinstance(v, tuple) else str(v))
def test_resample_sinc_ragged_rows_are_the_clips_alone(rates, n):
    lens = [n, 0, 1, n // 2]
    x = IO.clips(4, n, 300 + n)
    f = IO.sinc_filter(*rates, n)
    y, S, K, near = IO.sinc_ref(x, f, lens)
    got = _sinc_gpu(x, f, lens)
    a, b = IO.ratios(got, y, IO.sinc_bound(y, S, K), near)
    SUMMARY.note("resample_sinc", a, b)
    assert max(a, b) <= 1.0, (rates, n, a, b)
    assert not got[1].any()
    for r, nb in enumerate(lens):
        live = int(nb * f["ratio"])
        assert not got[r, live:].any()
        if nb:
            fa = IO.sinc_filter(*rates, nb)
            alone = _sinc_gpu(x[r:r + 1, :nb], fa)[0]
            assert np.array_equal(got[r, :live], alone[:live]), (rates, n, r)


def test_resample_sinc_refuses_more_outputs_than_time_registers_before_any_launch():
    f = IO.sinc_filter(22050, 16000, 90)
    _, err, prof = _profiled(lambda: _sinc_gpu(IO.clips(1, 90, 1), f, n_out=f["n_out"] + 1))
    assert err is not None and "time-register" in str(err), err
    assert prof == {}, prof


# ------------------------------------------------------------------------------------------------------------ PCM cast
def test_pcm16_on_every_int16_step_its_neighbours_and_what_lies_outside():
    """k / 32768 gives k for every k; the fp32 neighbours fall to the side truncation sends them; subnormals, +-0 -> 0; beyond full
    scale, +-inf -> the clamp; NaN of either sign -> 0.  Equal to audio.to_int16_pcm(clip=True) wherever x is not NaN and to clip=False
    (the script's statement) wherever -32769 < p: below that, and at NaN, the host cast is undefined (numpy wraps or gives
    INT_MIN), while the kernel clamps -- the one place they part ways."""
    x = IO.pcm_values()
    ref = IO.pcm_ref(x)
    got = _ctx().pcm16(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]
    assert np.array_equal(got[:65536], np.arange(-32768, 32768))
    with np.errstate(invalid="ignore"):
        p = x.astype(np.float64) * 32768.0
        ok, ok2 = ~np.isnan(p), p > -32769.0
        t = torch.from_numpy(x)
        assert np.array_equal(got[ok], audio.to_int16_pcm(t, clip=True)[ok])
        assert np.array_equal(got[ok2], audio.to_int16_pcm(t, clip=False)[ok2])
    assert (got[~ok] == 0).all() and (got[~ok2 & ok] == -32768).all()


@pytest.mark.parametrize("n", IO.PCM_LENGTHS)
def test_pcm16_scalar_path_lengths_and_bases_off_the_vector_grid(n):
    """The input base 0..3 floats off the 16-byte grid, the output base 0..3 int16 off the 8-byte grid (slices of larger 1-D tensors):
    only (0, 0) takes the vector path, and there the last n % 4 samples the scalar one.  Guard words around the n results stay."""
    x = IO.pcm_mix(n, 500 + n)
    ref = IO.pcm_ref(x)
    GUARD = 0x5A5A
    for io in range(4):
        for oo in range(4):
            src = torch.full((n + 16,), float("nan"), device="cuda")
            src[4 + io:4 + io + n] = torch.from_numpy(x).cuda()
            dst = torch.full((n + 16,), GUARD, dtype=torch.int16, device="cuda")
            wav, out = src[4 + io:4 + io + n], dst[4 + oo:4 + oo + n]
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 8 == 0
            assert wav.data_ptr() % 16 == 4 * io and out.data_ptr() % 8 == 2 * oo
            back = _ctx().pcm16(wav, out=out)
            assert back.data_ptr() == out.data_ptr()
            d = dst.cpu().numpy()
            assert np.array_equal(d[4 + oo:4 + oo + n], ref), (n, io, oo)
            assert (d[:4 + oo] == GUARD).all() and (d[4 + oo + n:] == GUARD).all(), (n, io, oo)


# ------------------------------------------------------------------------------------------------------------ mel stretch
@pytest.mark.parametrize("Tm", IO.STRETCH_TM)
def test_extend_mel_alone_through_the_clamp_and_the_block_seam(Tm):
    """ctx.extend_mel (extend_mel_cf_kernel): Tout = 1, 3, 5, 254, 256, 258, 861; the constant row stays exactly 1.0.  How many outputs
    differ in bits from the oracle's fp32 statement is reported (a contracted l0 a + l1 b), not asserted."""
    D = _ctx().desc.num_mels
    mel = IO.stretch_mel(2, D, Tm, Tm)
    y, E, near = IO.stretch_ref(mel)
    got = _ctx().extend_mel(torch.from_numpy(mel).cuda()).cpu().numpy()
    assert got.shape == y.shape == (2, D, IO.stretch_tout(Tm))
    a, b = IO.ratios(got, y, E, near)
    oracle = R.extend_mel(torch.from_numpy(mel)).numpy()
    NOT_BIT_IDENTICAL[Tm] = (int((got.view(np.int32) != oracle.view(np.int32)).sum()), got.size)
    print(f"   Tm={Tm}: err / E near-edge {a:.4f}, rest {b:.4f}; {NOT_BIT_IDENTICAL[Tm][0]} of {got.size} outputs not bit-identical to the oracle")
    SUMMARY.note("extend_mel", a, b)
    assert max(a, b) <= 1.0, (Tm, a, b)
    assert (got[0, 1] == 1.0).all()


def test_extend_mel_fused_into_the_generator_is_the_stand_alone_stretch():
    """extend_mel_kernel (stretch + transpose, the generator's first launch) has no tap of its own: the waveform of
    hifigan_forward(mel, stretch=True) must be that of hifigan_forward(extend_mel(mel), stretch=False) bit for bit (fp32), and a ragged
    batch [150, 3, 149] must give each clip alone (the clamp at ITS last frame)."""
    ctx = _ctx()
    D = ctx.desc.num_mels
    for Tm in (3, 149, 150):
        mel = torch.from_numpy(IO.stretch_mel(2, D, Tm, 40 + Tm)).cuda()
        fused = ctx.hifigan_forward(mel, stretch=True).cpu()
        split = ctx.hifigan_forward(ctx.extend_mel(mel), stretch=False).cpu()
        assert fused.shape == split.shape and torch.isfinite(fused).all() and float(fused.abs().max()) > 0
        assert torch.equal(fused, split), (Tm, float((fused - split).abs().max()))
    lens = [150, 3, 149]
    mel = torch.from_numpy(IO.stretch_mel(3, D, 150, 77)).cuda()
    rag = ctx.hifigan_forward_varlen(mel, lens, stretch=True).cpu()
    for b, Tm in enumerate(lens):
        alone = ctx.hifigan_forward(mel[b:b + 1, :, :Tm].contiguous(), stretch=True).cpu()[0]
        assert torch.equal(rag[b, :alone.numel()], alone), (b, Tm)
        assert not rag[b, alone.numel():].any()


# ------------------------------------------------------------------------------------------------------------ unit front-end
E_, KC, KP = 8, 11, 7


def _front_tables(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(KC, E_, generator=g), torch.randn(KP, E_, generator=g), torch.randn(B, E_, generator=g), g


def _front_gpu(code, emb_c, f0c=None, emb_p=None, spk=None):
    dev = lambda t: None if t is None else t.contiguous().cuda()
    return _ctx().unit_frontend(dev(code), dev(emb_c), dev(f0c), dev(emb_p) if f0c is not None else None, dev(spk)).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("Fc,Fp", [(256, 256), (257, 257), (255, 85), (64, 256), (513, 171), (1, 4)])
def test_unit_frontend_past_one_block_and_at_repeat_factors_above_two(Fc, Fp):
    """F = 256 | 257 (one block | two), repeat 3 of the F0 series, repeat 4 of the unit series, F = 513 (three blocks), one unit frame;
    with and without the speaker vector; bit for bit against the oracle's restatement of CodeGenerator.forward's front."""
    emb_c, emb_p, spk, g = _front_tables(Fc * 1000 + Fp)
    code, f0c = torch.randint(0, KC, (B, Fc), generator=g), torch.randint(0, KP, (B, Fp), generator=g)
    for s in (spk, None):
        got = _front_gpu(code, emb_c, f0c, emb_p, s)
        assert got.shape == (B, (3 if s is not None else 2) * E_, max(Fc, Fp))
        assert _same_bits(got, R.code_generator_front(code, emb_c, f0c, emb_p, s)), (Fc, Fp, s is not None)


def test_unit_frontend_code_and_speaker_without_f0():
    """`part == 1 && !f0c` is the speaker branch: channels E..2E are the speaker vector, F = 257."""
    emb_c, _, spk, g = _front_tables(5)
    code = torch.randint(0, KC, (B, 257), generator=g)
    got = _front_gpu(code, emb_c, spk=spk)
    assert _same_bits(got, R.code_generator_front(code, emb_c, None, None, spk)) and got.shape == (B, 2 * E_, 257)
    assert _same_bits(_front_gpu(code, emb_c), R.code_generator_front(code, emb_c))


@pytest.mark.parametrize("Fc,Fp", [(257, 257), (513, 171), (64, 256)])
@pytest.mark.parametrize("part", ["code", "f0"])
def test_unit_frontend_marks_exactly_the_columns_of_an_index_outside_its_table(Fc, Fp, part):
    """-1, K, K + 2^32 (equal to K's low word) and -2^63 planted at the source frames of output frames 0, 255, 256 and F - 1 of clip 1:
    NaN in exactly the columns those frames repeat into, in exactly that part's E channels; every other element keeps its bits."""
    emb_c, emb_p, spk, g = _front_tables(Fc * 7 + Fp)
    code, f0c = torch.randint(0, KC, (B, Fc), generator=g), torch.randint(0, KP, (B, Fp), generator=g)
    F = max(Fc, Fp)
    series, K, ch0 = (code, KC, 0) if part == "code" else (f0c, KP, E_)
    rep = F // series.shape[1]
    bad, clean = series.clone(), series.clone()
    want_nan = torch.zeros(B, 3 * E_, F, dtype=torch.bool)
    for t, v in zip((0, 255, 256, F - 1), (-1, K, K + 2 ** 32, -2 ** 63)):
        s = min(t, F - 1) // rep
        bad[1, s], clean[1, s] = v, 0
    for s in (bad[1] != series[1]).nonzero().reshape(-1).tolist():
        want_nan[1, ch0:ch0 + E_, s * rep:(s + 1) * rep] = True
    assert int(want_nan.sum()) >= 2 * E_ * rep            # at least the first and the last source frame
    args = (bad, f0c) if part == "code" else (code, bad)
    ref_args = (clean, f0c) if part == "code" else (code, clean)
    got = _front_gpu(args[0], emb_c, args[1], emb_p, spk)
    ref = R.code_generator_front(ref_args[0], emb_c, ref_args[1], emb_p, spk)
    assert torch.equal(torch.isnan(got), want_nan)
    assert _same_bits(torch.where(want_nan, torch.zeros(()), got), torch.where(want_nan, torch.zeros(()), ref))


# ------------------------------------------------------------------------------------------------------------ F0 encoder routes
def _f0_case(desc, Bn, T, seed):
    sd = synth.synth_f0_vqvae_state(desc, 20, seed=seed)
    g = torch.Generator().manual_seed(seed + T)
    f0 = torch.randn(Bn, desc.in_width, T, generator=g).abs() * 2.0
    f0[:, :, T // 3: T // 2] = 0.0                          # an unvoiced stretch
    return sd, f0


def _f0_both_routes(desc, sd, f0):
    """-> (default route's output, its profile, the SI_F0_FUSED=0 output, its profile), outputs on the CPU."""
    w = pack_f0_encoder(sd, desc).cuda()
    x = f0.cuda()
    a, err, pa = _profiled(lambda: _ctx().f0_encoder(desc, w, x))
    assert err is None, err
    with scoped_env({"SI_F0_FUSED": "0"}):
        b, err, pb = _profiled(lambda: _ctx().f0_encoder(desc, w, x))
    assert err is None, err
    return a.cpu(), pa, b.cpu(), pb


def _f0_oracle_rel(desc, sd, f0, h):
    ref = R.f0_encoder_forward(sd, f0, desc.down_t, desc.stride_t, desc.depth, desc.dilation_growth)
    assert h.shape == (ref.shape[0], ref.shape[2], ref.shape[1])
    return rms(h, ref.transpose(1, 2)) / rms(ref)


@pytest.mark.parametrize("dT", [-1, 0, 1, 2])
def test_f0_encoder_takes_the_single_launch_up_to_the_lds_limit_and_37_launches_past_it(dT):
    """The longest track whose activations fit 158 KiB of LDS by the launcher's formula is T = 877 for the hubert_lut.json descriptor:
    at 876 and 877 the profile shows one f0enc_fused launch and no f0enc_conv1d, at 878 and 879 the 37 convolutions and no fused
    launch; all bit-identical to the SI_F0_FUSED=0 run and within 1e-5 relative rms of the oracle."""
    desc = native.F0EncDesc()
    Tmax = IO.f0_longest_fused(desc)
    assert Tmax == 877
    T = Tmax + dT
    sd, f0 = _f0_case(desc, 2, T, 5)
    a, pa, b, pb = _f0_both_routes(desc, sd, f0)
    want = {"f0enc_fused": 1} if T <= Tmax else {"f0enc_conv1d": IO.f0_launches(desc)}
    ROUTES[f"default T={T}"] = pa
    assert pa == want, (T, pa)
    assert pb == {"f0enc_conv1d": 37}, pb
    assert torch.equal(a, b), (T, float((a - b).abs().max()))
    rel = _f0_oracle_rel(desc, sd, f0, a)
    print(f"   T={T}: {pa}, vs the oracle {rel:.2e} relative")
    assert rel <= 1e-5


F0_VARIANTS = {
    "m_conv=2": dict(m_conv=2.0),                          # n_state 64 > width: the Y buffer is the larger one
    "stride_t=3,down_t=2": dict(stride_t=3, down_t=2),     # k = 7, pad = 2
    "in_width=2": dict(in_width=2),
    "down_t=1": dict(down_t=1),
    "width=12": dict(width=12),                            # off the 8-channel grid: the launcher falls back to the convolutions
}


@pytest.mark.parametrize("T", [16, 17, 33, 200])
@pytest.mark.parametrize("name", list(F0_VARIANTS))
def test_f0_encoder_descriptor_variants_fused_against_layer_by_layer_and_the_oracle(name, T):
    desc = native.F0EncDesc(**F0_VARIANTS[name])
    sd, f0 = _f0_case(desc, 2, T, 9)
    a, pa, b, pb = _f0_both_routes(desc, sd, f0)
    layers = {"f0enc_conv1d": IO.f0_launches(desc)}
    ROUTES[f"{name} T={T}"] = pa
    assert pa == (layers if name == "width=12" else {"f0enc_fused": 1}), (name, T, pa)
    assert pb == layers, (name, T, pb)
    assert torch.equal(a, b), (name, T, float((a - b).abs().max()))
    rel = _f0_oracle_rel(desc, sd, f0, a)
    print(f"   {name} T={T}: {pa}, vs the oracle {rel:.2e} relative")
    assert rel <= 1e-5


# ------------------------------------------------------------------------------------------------------------ summary
def test_zz_summary_of_ratios():
    SUMMARY.report()
    n, total = sum(v[0] for v in NOT_BIT_IDENTICAL.values()), sum(v[1] for v in NOT_BIT_IDENTICAL.values())
    print(f"   SUMMARY extend_mel: {n} of {total} outputs not bit-identical to the oracle's fp32 statement {dict((k, v[0]) for k, v in NOT_BIT_IDENTICAL.items())}")
    for k, v in ROUTES.items():
        print(f"   SUMMARY f0 route {k}: {v}")
