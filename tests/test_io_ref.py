"""tests/io_ref.py against independent sources, on the CPU: poly_ref against scipy.signal.resample_poly, sinc_ref against the oracle's
resampy restatement, the stretch against the oracle's extend_mel, the PCM reference against audio.to_int16_pcm where that is defined --
each at the cases tests/test_gpu_io_ops.py runs and inside the bound E that file asserts, so the inputs are shown to leave the
references alone inside E.  Then every planted mistake is shown to leave E by more than a factor 2 on one of those cases (a kernel that
is within E of the truth and made the mistake would sit more than E from the reference): the evidence that the GPU tests fail for a
subtly wrong kernel."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from speech_inpainting_amd import audio
from speech_inpainting_amd.native import F0EncDesc
from tests import io_ref as IO

B = 3


def _poly(sr_in, sr_out, n_in, x=None, mistake=None):
    taps, up, down, pre, n_out = audio.design_resampler(sr_in, sr_out, n_in)
    x = IO.clips(B, n_in, 100 + n_in) if x is None else x
    return x, (taps, up, down, pre, n_out), IO.poly_ref(x, taps, up, down, pre, n_out, mistake)


@pytest.mark.parametrize("rates", list(IO.POLY_CASES), ids=lambda r: f"{r[0]}to{r[1]}")
def test_poly_ref_is_scipys_resample_poly_and_the_fp32_chain_stays_inside_E(rates):
    """scipy filters with the float64 taps, the definition with their fp32 roundings: the two differ by at most 2^-24 S (+ float64 noise).
    The kernel's own fmaf chain, emulated in fp32, stays inside E at every case; the listed lengths give the listed n_out."""
    from scipy.signal import resample_poly
    worst_abs = worst = 0.0
    for n_in in IO.POLY_CASES[rates]:
        x, (taps, up, down, pre, n_out), (y, S, K, near) = _poly(*rates, n_in)
        assert n_out == IO.POLY_N_OUT.get((*rates, n_in), n_out) and y.shape == (B, n_out)
        ref = resample_poly(x.astype(np.float64), up, down, axis=1, window=("kaiser", audio.KAISER_BETA))
        assert ref.shape == y.shape
        assert (np.abs(y - ref) <= IO.U24 * S + 1e-13).all(), (rates, n_in, float(np.abs(y - ref).max()))
        worst_abs = max(worst_abs, float(np.abs(y - ref).max()))
        chain = IO.poly_fp32_chain(x, taps, up, down, pre, n_out)
        worst = max(worst, *IO.ratios(chain, y, IO.poly_bound(S, K), near))
        assert K.max() >= 1 and (K >= 1).all()             # every output has a term, and K = 1 (E attainable) occurs at n_in = 1
        if n_in > 300:
            assert near.any() and (~near).any()
    print(f"   {rates}: definition vs scipy {worst_abs:.2e} absolute, fp32 chain / E {worst:.3f}")
    assert worst <= 1.0


def test_poly_ref_impulse_is_the_tap_table():
    for rates, lens in IO.POLY_CASES.items():
        n_in = lens[-1]
        taps, up, down, pre, n_out = audio.design_resampler(*rates, n_in)
        for j0 in (0, n_in - 1, n_in // 2):
            y = IO.poly_ref(IO.impulse(n_in, j0), taps, up, down, pre, n_out)[0][0]
            k = (np.arange(n_out) + pre) * down - j0 * up
            want = np.where((k >= 0) & (k < taps.size), taps[np.clip(k, 0, taps.size - 1)], 0.0)
            assert np.array_equal(y, want.astype(np.float64))


@pytest.mark.parametrize("rates", list(IO.SINC_CASES), ids=lambda r: f"{r[0]}to{r[1]}")
def test_sinc_ref_is_the_oracles_resampler_inside_E(rates):
    """Against R.resample_kaiser_best, clip by clip: inside the float64 term of E before the cast, inside E after it; zero at and past
    int(n_in ratio); integer accumulated times where the docstring of the cases says so."""
    worst64 = worst = 0.0
    for n_in in IO.SINC_CASES[rates]:
        x = IO.clips(B, n_in, 200 + n_in)
        f = IO.sinc_filter(*rates, n_in)
        y, S, K, near = IO.sinc_ref(x, f, n_in)
        live = int(n_in * f["ratio"])
        assert y.shape == (B, f["n_out"]) and not y[:, live:].any() and near[:, live:].all()
        for b in range(B):
            ref = R.resample_kaiser_best(x[b], *rates)
            assert ref.shape == (f["n_out"],)
            e64 = (K[b] + 2) * IO.U52 * S[b] + IO.TINY
            worst64 = max(worst64, float((np.abs(y[b] - ref) / e64).max()))
            worst = max(worst, *IO.ratios(ref.astype(np.float32), y[b], IO.sinc_bound(y[b], S[b], K[b]), near[b]))
        if n_in < 60:
            assert near.all()                              # shorter than the window: every output has a wing cut by an end
    tr = IO.sinc_filter(*rates, 64)["time_reg"]
    whole = float((tr == np.floor(tr)).mean())
    print(f"   {rates}: oracle / float64 term {worst64:.3f}, after the cast / E {worst:.3f}, integer times {whole:.2f}")
    assert worst64 <= 1.0 and worst <= 1.0
    assert whole == {(48000, 16000): 1.0, (16000, 8000): 1.0, (8000, 16000): 0.5}.get(rates, whole)


def test_sinc_ref_ragged_rows_are_the_clips_alone():
    rates, n = (22050, 16000), 90
    x = IO.clips(4, n, 7)
    f = IO.sinc_filter(*rates, n)
    lens = [n, 0, 1, n // 2]
    y = IO.sinc_ref(x, f, lens)[0]
    for b, nb in enumerate(lens):
        alone = IO.sinc_ref(x[b, :max(nb, 1)], IO.sinc_filter(*rates, max(nb, 1)), nb)[0][0]
        live = int(nb * f["ratio"])
        assert np.array_equal(y[b, :live], alone[:live]) and not y[b, live:].any()
    assert not y[1].any()


def test_pcm_ref_is_the_host_cast_where_that_is_defined():
    """clip=True clamps before the cast, so it is defined for everything but NaN; clip=False (the script's own statement) clamps only
    above, so below p = -32769 it hands numpy a value outside int16 -- undefined, and there the kernel (which clamps) and the host
    helper part ways, as they do at NaN."""
    x = IO.pcm_values()
    ref = IO.pcm_ref(x)
    k = np.arange(-32768, 32768)
    assert np.array_equal(ref[:65536], k)
    assert np.array_equal(ref[65536:131072], np.where(k >= 0, k, k + 1))         # the neighbour above: toward zero below 0
    assert np.array_equal(ref[131072:196608], np.where(k > 0, k - 1, k))         # the neighbour below: one step down above 0
    with np.errstate(invalid="ignore"):                  # (a signalling NaN among the values)
        p = x.astype(np.float64) * 32768.0
    t = torch.from_numpy(x)
    ok = ~np.isnan(p)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(audio.to_int16_pcm(t, clip=True)[ok], ref[ok])
        ok2 = p > -32769.0
        assert np.array_equal(audio.to_int16_pcm(t, clip=False)[ok2], ref[ok2]) and int((~ok2).sum()) >= 8
    assert (ref[np.isnan(p)] == 0).all() and int(np.isnan(p).sum()) == 4
    assert not np.array_equal(IO.pcm_ref(x, mistake="rounds"), ref)
    for n in IO.PCM_LENGTHS:
        assert IO.pcm_mix(n, n).shape == (n,)


@pytest.mark.parametrize("Tm", IO.STRETCH_TM)
def test_stretch_ref_is_the_oracles_extend_mel_inside_E(Tm):
    mel = IO.stretch_mel(2, 80, Tm, Tm)
    y, E, near = IO.stretch_ref(mel)
    ref = R.extend_mel(torch.from_numpy(mel)).numpy()
    assert ref.shape == y.shape == (2, 80, IO.stretch_tout(Tm))
    a, b = IO.ratios(ref, y, E, near)
    print(f"   Tm={Tm}: oracle / E near {a:.3f}, rest {b:.3f}")
    assert max(a, b) <= 1.0 and near.any()
    assert (ref[0, 1] == 1.0).all() and (np.abs(y[0, 1] - 1.0) <= 2.0 ** -25).all()     # (the float64 form keeps fl(1 - l1)'s rounding)
    # i0's own clamp never binds, at any of these lengths and far beyond them
    for T in list(IO.STRETCH_TM) + [4096, 100003]:
        t = np.arange(IO.stretch_tout(T), dtype=np.float32)
        src = ((t + np.float32(0.5)).astype(np.float64) * np.float64(np.float32(256.0 / 441.0)) - 0.5).astype(np.float32)
        assert np.floor(src).max() <= T - 1


def _worst_over_E(y_wrong, y, E):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(y_wrong == y, 0.0, np.abs(y_wrong - y) / E)
    return float(q.max(initial=0.0))


def test_every_planted_mistake_leaves_E_on_one_of_the_cases():
    """Which case catches which mistake is printed; each must exceed 2 E somewhere (most do by thousands)."""
    caught = {}
    for rates, lens in IO.POLY_CASES.items():
        for n_in in lens:
            x, d, (y, S, K, _) = _poly(*rates, n_in)
            for mk in IO.POLY_MISTAKES:
                r = _worst_over_E(IO.poly_ref(x, *d, mistake=mk)[0], y, IO.poly_bound(S, K))
                if r > caught.get(("poly", mk), (0.0,))[0]:
                    caught[("poly", mk)] = (r, rates, n_in)
    for rates, lens in IO.SINC_CASES.items():
        for n_in in lens:
            x = IO.clips(B, n_in, 200 + n_in)
            f = IO.sinc_filter(*rates, n_in)
            y, S, K, _ = IO.sinc_ref(x, f, n_in)
            for mk in IO.SINC_MISTAKES:
                r = _worst_over_E(IO.sinc_ref(x, f, n_in, mistake=mk)[0], y, IO.sinc_bound(y, S, K))
                if r > caught.get(("sinc", mk), (0.0,))[0]:
                    caught[("sinc", mk)] = (r, rates, n_in)
    for Tm in IO.STRETCH_TM:
        mel = IO.stretch_mel(2, 80, Tm, Tm)
        y, E, _ = IO.stretch_ref(mel)
        for mk in IO.STRETCH_MISTAKES:
            r = _worst_over_E(IO.stretch_ref(mel, mistake=mk)[0], y, E)
            if r > caught.get(("stretch", mk), (0.0,))[0]:
                caught[("stretch", mk)] = (r, "Tm", Tm)
    for key, (r, where, n) in sorted(caught.items()):
        print(f"   {key[0]} {key[1]}: {r:.3g} E at {where} n = {n}")
    want = [("poly", m) for m in IO.POLY_MISTAKES] + [("sinc", m) for m in IO.SINC_MISTAKES] + [("stretch", m) for m in IO.STRETCH_MISTAKES]
    assert sorted(caught) == sorted(want) and all(v[0] > 2.0 for v in caught.values()), caught
    # dropping the last tap in MID-signal is below any fp32 bound (the Kaiser tail is ~1e-8): only a clip shorter than the window shows it
    rates = (22050, 16000)
    for n_in, seen in ((354, False), (64, True)):
        x = IO.clips(B, n_in, 200 + n_in)
        f = IO.sinc_filter(*rates, n_in)
        y, S, K, near = IO.sinc_ref(x, f, n_in)
        q = np.abs(IO.sinc_ref(x, f, n_in, mistake="last_tap_dropped")[0] - y) / IO.sinc_bound(y, S, K)
        mid = slice(100, 150) if n_in == 354 else slice(None)
        assert (float(q[:, mid].max()) > 2.0) == seen, (n_in, float(q[:, mid].max()))


def test_f0_route_formula_gives_877_for_the_default_descriptor():
    d = F0EncDesc()
    assert IO.f0_longest_fused(d) == 877 and IO.f0_launches(d) == 37
    assert IO.f0_fused_lds_bytes(d, 877) == (2 * 32 * 438 + 12288 + 128) * 4 <= 158 * 1024 < IO.f0_fused_lds_bytes(d, 878)
    assert IO.f0_fused_lds_bytes(F0EncDesc(width=12), 64) is None
    assert IO.f0_fused_lds_bytes(F0EncDesc(m_conv=2), 200) == (2 * 64 * 100 + 12288 + 128) * 4
