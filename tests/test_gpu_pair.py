"""si_cut_pair / si_cut_pair_ch alone: both clip sets of a pass cut straight out of a file, in one launch.  No model.

The 22.05 kHz rows must be si_cut_rate's bytes on starts 441 f.  The reference of the 16 kHz rows is tests/pair_ref.py, the definition in
numpy float64; every output must lie within
    2^-24 |y| + (2 H16 + 2) 2^-52 A,   A = sum |c x| over the sample's taps, H16 = taps per wing of the sr -> 16 kHz filter
of it (tests/test_gpu_feed.py's derivation: the one rounding to fp32, and the float64 sum, which the kernel's fma chain and numpy's
separate multiply and add may spend differently).  Where A is zero -- a sample at or past the file's end, a 16 kHz file's own sample --
the output is fl32(y) exactly.  The worst err / bound is reported per rate."""
import ctypes as C

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import channels_ref as CH
from tests import feed_ref as F
from tests import pair_ref as PR
from tests import poison as P
from tests.harness import RatioSummary, build_engine

pytestmark = pytest.mark.gpu

FR = native.CUT_PAIR_FRAMES
T22, T16 = 441 * FR, 320 * FR
RATES = [48000, 44100, 32000, 16000, 11025, 8000, 4000, 192000]
SUMMARY = RatioSummary()
_CASES = {}


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", "fp32", key=("patch", "fp32"))


def _l16(L22):
    return -(-L22 * 320 // 441)


def _filters(eng, sr):
    return eng._feed_filter(sr), eng._feed_filter16(sr)


def _case(sr):
    """An int16 file of a little over 2 FR + 5 frames whose L16 rule allows one 16 kHz sample past N16 (at 11.025 kHz no length does:
    N22 = 2 n, and ceil(640 n / 441) is N16 itself), and the reference of EVERY sample of both axes (the 16 kHz one up to
    ceil(N22 320 / 441))."""
    if sr not in _CASES:
        P22, Q22 = G.rate_ratio(sr)
        first = -(-((2 * FR + 5) * 441 + 300) * Q22 // P22) + 3
        n_file = next((n for n in range(first, first + 2000) if PR.lim16(n, sr) == PR.n_axis(n, sr, 16000) + 1), first)
        v = np.random.default_rng(sr).integers(-20000, 20001, size=n_file).astype(np.int16)
        N22, N16, lim = F.n22(n_file, sr), PR.n_axis(n_file, sr, 16000), PR.lim16(n_file, sr)
        y16, A16, _ = PR.samples16(v, np.arange(lim), sr)
        _CASES[sr] = dict(v=v, N22=N22, N16=N16, lim=lim, y16=y16, A16=A16)
    return _CASES[sr]


def _both(v, dev, off32=0, off16=0):
    """The int16 file v on the device as int16 and as the fp32 file that holds v / 32768."""
    return CH.on_device(v.astype(np.float32) / np.float32(32768.0), dev, off32), CH.on_device(v, dev, off16)


def _last_frame(c, L22, L16):
    return min((c["N22"] - L22) // 441, (c["lim"] - L16) // 320)


def _check16(out16, frames, y, A, sr, label):
    """out16 (C, L16) host fp32 against the reference of the whole 16 kHz axis; exact where A is zero."""
    L16 = out16.shape[1]
    j = 320 * np.asarray(frames, dtype=np.int64)[:, None] + np.arange(L16)[None, :]
    ref, a = y[j], A[j]
    exact = a == 0
    assert np.array_equal(out16[exact].view(np.int32), ref[exact].astype(np.float32).view(np.int32)), label
    E = PR.kernel_bound(ref, a, sr)
    ratio = np.where(exact, 0.0, np.abs(out16.astype(np.float64) - ref) / np.maximum(E, 1e-300))
    seam = (np.arange(L16) % T16 == 0) | (np.arange(L16) % T16 == T16 - 1) | (np.arange(L16) == L16 - 1)
    near = float(ratio[:, seam].max())
    rest = float(ratio[:, ~seam].max()) if (~seam).any() else 0.0
    SUMMARY.note(label, near, rest)
    assert near <= 1.0 and rest <= 1.0, (label, L16, near, rest)


def _i32(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("sr", RATES)
def test_bytes_bound_sample_types_and_tile_seams(sr):
    """L22 in {1, T - 1, T, T + 1, 2 T + 1} with T = 441 FR and L16 = ceil(L22 320 / 441), then the whole recording with L16 at its largest
    permitted value (one 16 kHz sample past N16: zero); frames at 0, mid-file and flush against the recording's end, overlapping and
    unsorted, one frame twice.  out22 is si_cut_rate's bytes; out16 lies within the bound; the fp32 file that holds v / 32768 and the int16
    file give the same bytes, a repeated call gives them again, and C = 1 / 2 / 32 cut the same rows."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    c = _case(sr)
    x32, x16 = _both(c["v"], dev)
    f22, f16 = _filters(eng, sr)
    assert (f16 is None) == (sr == 16000) and c["lim"] == c["N16"] + (sr != 11025)
    seen = np.zeros(c["lim"], dtype=bool)
    for L22, L16 in [(L, _l16(L)) for L in (1, T22 - 1, T22, T22 + 1, 2 * T22 + 1)] + [(c["N22"], c["lim"])]:
        last = _last_frame(c, L22, L16)
        frames = [f for f in (last, 0, 1, 2, 1, last - 1) if 0 <= f <= last]
        assert frames[0] == last and (L22 == c["N22"] or (len(frames) >= 5 and sorted(frames) != frames))
        a22, a16 = ctx.cut_pair(x32, sr, frames, L22, L16, f22, f16)
        b22, b16 = ctx.cut_pair(x16, sr, frames, L22, L16, f22, f16)
        again = ctx.cut_pair(x16, sr, frames, L22, L16, f22, f16, out22=torch.full((len(frames), L22), 7.0, device=dev),
                             out16=torch.full((len(frames), L16), 7.0, device=dev))
        want22 = ctx.cut_rate(x16, sr, [441 * f for f in frames], L22, f22)
        many = (frames * 32)[:32]
        m22, m16 = ctx.cut_pair(x16, sr, many, L22, L16, f22, f16)
        o22, o16 = ctx.cut_pair(x16, sr, many[5:6], L22, L16, f22, f16)
        p22, p16 = ctx.cut_pair(x16, sr, many[6:8], L22, L16, f22, f16)
        torch.cuda.synchronize()
        assert a22.shape == (len(frames), L22) and a16.shape == (len(frames), L16)
        assert torch.equal(_i32(b22), _i32(want22)), (sr, L22, "out22 | si_cut_rate")
        assert torch.equal(_i32(a22), _i32(b22)) and torch.equal(_i32(a16), _i32(b16)), (sr, L22, "fp32 | int16")
        assert torch.equal(_i32(again[0]), _i32(b22)) and torch.equal(_i32(again[1]), _i32(b16)), (sr, L22, "repeated call")
        rows = torch.tensor([k % len(frames) for k in range(32)], device=dev)
        assert torch.equal(_i32(m22), _i32(b22[rows])) and torch.equal(_i32(m16), _i32(b16[rows])), (sr, L22, "C = 32")
        assert torch.equal(_i32(o22), _i32(m22[5:6])) and torch.equal(_i32(o16), _i32(m16[5:6])), (sr, L22, "C = 1")
        assert torch.equal(_i32(p22), _i32(m22[6:8])) and torch.equal(_i32(p16), _i32(m16[6:8])), (sr, L22, "C = 2")
        if L22 > 441 and len(frames) > 2:                             # frames 0 and 1 overlap: the same sample in two clips
            assert torch.equal(_i32(b22[1, 441:]), _i32(b22[2, :L22 - 441])) and torch.equal(_i32(b16[1, 320:]), _i32(b16[2, :L16 - 320]))
        _check16(b16.cpu().numpy(), frames, c["y16"], c["A16"], sr, f"cut_pair {sr} Hz")
        for f in frames:
            seen[320 * f:320 * f + L16] = True
    assert seen.all() and abs(c["y16"][c["N16"] - 1]) > 0 and not c["y16"][c["N16"]:].any() and float(np.abs(c["y16"]).max()) > 0.1


def test_kernel_summary():
    SUMMARY.report()


@pytest.mark.parametrize("sr", [16000, 48000])
def test_a_16_khz_file_s_rows_are_its_samples(sr):
    """At sr = 16000 out16 is the file slice, byte for byte, with zeros past N16 -- for the fp32 file its own bits, -0.0 and a NaN
    included (nothing is computed).  48 kHz stands beside it as the rate where the rows are NOT the file's every third sample."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    c = _case(sr)
    f22, f16 = _filters(eng, sr)
    x = c["v"].astype(np.float32) / np.float32(32768.0)
    if sr == 16000:
        x.view(np.int32)[[5, 700]] = [-2 ** 31, 0x7fc12345]
    frames, L22, L16 = [0, 2], 3 * 441, 3 * 320
    out22, out16 = ctx.cut_pair(torch.from_numpy(x).to(dev), sr, frames, L22, L16, f22, f16)
    whole22, whole16 = ctx.cut_pair(torch.from_numpy(x).to(dev), sr, [0], c["N22"], c["lim"], f22, f16)
    torch.cuda.synchronize()
    got = out16.cpu().numpy()
    if sr == 16000:
        assert np.array_equal(got.view(np.int32), np.stack([x[320 * f:320 * f + L16] for f in frames]).view(np.int32))
        w = whole16.cpu().numpy()[0]
        assert c["N16"] == x.size and np.array_equal(w[:x.size].view(np.int32), x.view(np.int32)) and w[x.size:].view(np.int32).tolist() == [0]
    else:
        assert not np.array_equal(got[0], x[0:3 * L16:3])
        assert whole16.cpu().numpy()[0, c["N16"]:].view(np.int32).tolist() == [0]


@pytest.mark.parametrize("sr", [48000, 16000, 192000])
def test_short_files(sr):
    """A file shorter than one wing, and a file of one sample: every tap count is cut by the file's ends."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    f22, f16 = _filters(eng, sr)
    for n_file in (max(PR.reach(sr, 16000), PR.reach(sr, 22050)) - 3, 1):
        v = np.random.default_rng(n_file).integers(-20000, 20001, size=n_file).astype(np.int16)
        N22, lim = F.n22(n_file, sr), PR.lim16(n_file, sr)
        y16, A16, _ = PR.samples16(v, np.arange(lim), sr)
        x32, x16 = _both(v, dev, 1, 1)
        for L22, L16 in ((N22, lim), (1, 1)):
            a22, a16 = ctx.cut_pair(x32, sr, [0], L22, L16, f22, f16)
            b22, b16 = ctx.cut_pair(x16, sr, [0], L22, L16, f22, f16)
            want22 = ctx.cut_rate(x16, sr, [0], L22, f22)
            torch.cuda.synchronize()
            assert torch.equal(_i32(a22), _i32(b22)) and torch.equal(_i32(a16), _i32(b16)) and torch.equal(_i32(b22), _i32(want22))
            _check16(a16.cpu().numpy(), [0], y16, A16, sr, f"cut_pair short {sr} Hz")
        assert np.abs(y16).max() > 0
    SUMMARY.report(keys=[f"cut_pair short {sr} Hz"])


def test_base_pointers_off_the_16_byte_grid():
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    for sr in (48000, 8000, 16000):
        c = _case(sr)
        f22, f16 = _filters(eng, sr)
        L22, L16 = T22 + 1, _l16(T22 + 1)
        frames = [0, 2, _last_frame(c, L22, L16)]
        x32, x16 = _both(c["v"], dev)
        want = ctx.cut_pair(x32, sr, frames, L22, L16, f22, f16)
        for o32, o16 in ((1, 1), (2, 3), (3, 7)):
            y32, y16 = _both(c["v"], dev, o32, o16)
            assert y32.data_ptr() % 16 == 4 * o32 and y16.data_ptr() % 16 == 2 * o16
            a, b = ctx.cut_pair(y32, sr, frames, L22, L16, f22, f16), ctx.cut_pair(y16, sr, frames, L22, L16, f22, f16)
            torch.cuda.synchronize()
            for k in (0, 1):
                assert torch.equal(_i32(a[k]), _i32(want[k])) and torch.equal(_i32(b[k]), _i32(want[k])), (sr, o32, o16, k)


@pytest.mark.parametrize("sr", [48000, 44100])
def test_the_time_is_64_bit(sr):
    """An int16 file of 15 M samples: at 48 kHz the 22.05 kHz row's j Q22 passes 2^31 (Q22 = 320), at 44.1 kHz the 16 kHz row's j Q16 does
    (Q16 = 441); the clips sit flush against the recording's end and across the crossing."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    Q22, Q16 = G.rate_ratio(sr)[1], G.rate_ratio16(sr)[1]
    n_file = 15_000_000
    v = np.random.default_rng(7).integers(-20000, 20001, size=n_file).astype(np.int16)
    c = dict(N22=F.n22(n_file, sr), lim=PR.lim16(n_file, sr))
    L22, L16 = T22 + 1, _l16(T22 + 1)
    cross = 2 ** 31 // (441 * Q22) if sr == 48000 else 2 ** 31 // (320 * Q16)
    frames = [_last_frame(c, L22, L16), cross]
    assert (441 * frames[0] * Q22 > 2 ** 31) if sr == 48000 else (320 * frames[0] * Q16 > 2 ** 31)
    assert (441 * cross * Q22 < 2 ** 31 < (441 * cross + L22) * Q22) if sr == 48000 else (320 * cross * Q16 < 2 ** 31 < (320 * cross + L16) * Q16)
    f22, f16 = _filters(eng, sr)
    x = torch.from_numpy(v).to(dev)
    out22, out16 = ctx.cut_pair(x, sr, frames, L22, L16, f22, f16)
    want22 = ctx.cut_rate(x, sr, [441 * f for f in frames], L22, f22)
    torch.cuda.synchronize()
    assert torch.equal(_i32(out22), _i32(want22))
    j = np.concatenate([320 * f + np.arange(L16) for f in frames])
    y, A, _ = PR.samples16(v, j, sr)
    got = out16.cpu().numpy().reshape(-1).astype(np.float64)
    ratio = float((np.abs(got - y) / PR.kernel_bound(y, A, sr)).max())
    SUMMARY.note(f"cut_pair 64-bit {sr} Hz", ratio, ratio)
    SUMMARY.report(keys=[f"cut_pair 64-bit {sr} Hz"])
    assert ratio <= 1.0 and float(np.abs(y).max()) > 0.1


# ------------------------------------------------------------------------------------------------------------ si_cut_pair_ch
@pytest.mark.parametrize("ch", [2, 3, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["fp32", "int16"])
def test_cut_pair_ch_equals_cut_pair_on_the_channel(dtype, ch):
    """Each channel of an interleaved file, its neighbours holding noise at ten times its amplitude, byte-equal to the mono call on the
    de-interleaved copy -- clips at the recording's start and flush against its end, where taps fall outside the file."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    for sr in (48000, 16000, 11025):
        c = _case(sr)
        f22, f16 = _filters(eng, sr)
        col = c["v"] if dtype is np.int16 else (c["v"].astype(np.float32) / np.float32(32768.0) * np.float32(0.1))
        if dtype is np.int16:
            col = (col // 10).astype(np.int16)
        L22, L16 = 2 * T22 + 1, _l16(2 * T22 + 1)
        frames = [_last_frame(c, L22, L16), 0, 1]
        for k in sorted({0, ch // 2, ch - 1}):
            x = CH.around(col, k, ch, seed=ch)
            got = ctx.cut_pair(CH.on_device(x, dev, 1), sr, frames, L22, L16, f22, f16, channel=k)
            want = ctx.cut_pair(torch.from_numpy(np.ascontiguousarray(x[:, k])).to(dev), sr, frames, L22, L16, f22, f16)
            whole = ctx.cut_pair(CH.on_device(x, dev), sr, [0], c["N22"], c["lim"], f22, f16, channel=k)
            whole1 = ctx.cut_pair(torch.from_numpy(np.ascontiguousarray(x[:, k])).to(dev), sr, [0], c["N22"], c["lim"], f22, f16)
            torch.cuda.synchronize()
            for a, b in zip(got + whole, want + whole1):
                assert torch.equal(_i32(a), _i32(b)), (sr, ch, k)


def test_full_scale_neighbours_never_leak_in():
    """A silent channel between full-scale neighbours, files shorter than a wing included: every output of the silent channel is +0.0."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    for sr in (48000, 16000, 192000):
        f22, f16 = _filters(eng, sr)
        for n_file in (1, 50, 3 * sr // 50 + 7):
            for dtype, full in ((np.int16, 32767), (np.float32, 1.0)):
                x = np.full((n_file, 3), full, dtype=dtype)
                x[:, 0] = -x[:, 0]
                x[:, 1] = 0
                N22, lim = F.n22(n_file, sr), PR.lim16(n_file, sr)
                out22, out16 = ctx.cut_pair(CH.on_device(x, dev, 1), sr, [0], N22, lim, f22, f16, channel=1)
                loud22, loud16 = ctx.cut_pair(CH.on_device(x, dev, 1), sr, [0], N22, lim, f22, f16, channel=2)
                torch.cuda.synchronize()
                assert not _i32(out22).any() and not _i32(out16).any(), (sr, n_file, dtype)
                assert float(loud22.abs().max()) > 0.05 and float(loud16.abs().max()) > 0.05


# ------------------------------------------------------------------------------------------------------------ the C ABI
def _sinc(f, **kw):
    d = dict(nwin=f["win"].numel(), num_table=f["num_table"], step=f["step"], scale=f["scale"], win=f["win"].data_ptr(), dwin=f["dwin"].data_ptr())
    d.update(kw)
    return native.SincFilter(C.sizeof(native.SincFilter), d["nwin"], d["num_table"], d["step"], 0, 0, d["scale"], 0.0, d["win"], d["dwin"], None)


def test_a_device_frame_table_that_differs_gives_zeros():
    """The host copy is valid; the device table names frames before the file, just past its end and far past it: those rows come
    back as zeros, the row whose device entry is valid holds its clip, and nothing faults (the staging loop reads inside the file only)."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    for sr in (48000, 16000):
        c = _case(sr)
        f22, f16 = _filters(eng, sr)
        x = torch.from_numpy(c["v"]).to(dev)
        L22, L16 = T22 + 1, _l16(T22 + 1)
        host = np.zeros(5, dtype=np.int32)
        devt = torch.tensor([-1, c["N22"] // 441 + 1, 2 ** 31 - 1, 1, -2 ** 31], dtype=torch.int32, device=dev)
        out22 = torch.full((5, L22), 7.0, device=dev)
        out16 = torch.full((5, L16), 7.0, device=dev)
        s22 = _sinc(f22)
        s16 = _sinc(f16) if f16 is not None else None
        rc = ctx.lib.si_cut_pair(ctx._h, native._ptr(x), 1, c["v"].size, sr, host.ctypes.data_as(C.c_void_p), native._ptr(devt), 5, L22, L16,
                                 C.byref(s22), C.byref(s16) if s16 is not None else None, native._ptr(out22), native._ptr(out16), ctx._stream())
        want22, want16 = ctx.cut_pair(x, sr, [1], L22, L16, f22, f16)
        torch.cuda.synchronize()
        assert rc == 0
        for k in (0, 1, 2, 4):
            assert not _i32(out22[k]).any() and not _i32(out16[k]).any(), (sr, k)
        assert torch.equal(_i32(out22[3]), _i32(want22[0])) and torch.equal(_i32(out16[3]), _i32(want16[0]))


def test_refusals_launch_nothing():
    """Straight at the C ABI: every malformed call returns an error code and a message naming the entry and the argument, launches
    nothing and leaves both outputs untouched."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    sr = 48000
    c = _case(sr)
    N22, lim, n_file = c["N22"], c["lim"], c["v"].size
    x = torch.from_numpy(c["v"]).to(dev)
    f22, f16 = _filters(eng, sr)
    L22_0, L16_0 = 441, 320
    out22 = torch.full((2, L22_0), 7.0, device=dev)
    out16 = torch.full((2, L16_0), 7.0, device=dev)
    x2 = torch.from_numpy(np.ascontiguousarray(np.stack([c["v"], c["v"]], axis=1))).to(dev)

    def call(frames=(0, 1), a=None, b=None, sr_=sr, n=n_file, o22=out22, o16=out16, x_=x, L22=L22_0, L16=L16_0, Cn=None, host=True, devt=True,
             chan=None):
        h = np.ascontiguousarray(np.asarray(frames, dtype=np.int32))
        d = torch.from_numpy(h).to(dev)
        a = _sinc(f22) if a is None else a
        b = _sinc(f16) if b is None else b
        tail = (h.ctypes.data_as(C.c_void_p) if host else None, native._ptr(d) if devt else None, len(h) if Cn is None else Cn, L22, L16,
                C.byref(a) if a else None, C.byref(b) if b else None, native._ptr(o22), native._ptr(o16), ctx._stream())
        ctx.profile_start(100)
        if chan is None:
            rc = ctx.lib.si_cut_pair(ctx._h, native._ptr(x_), 1, n, sr_, *tail)
        else:
            rc = ctx.lib.si_cut_pair_ch(ctx._h, native._ptr(x2 if x_ is x else x_), 1, n, chan[0], chan[1], sr_, *tail)
        msg = ctx.lib.si_last_error(ctx._h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        torch.cuda.synchronize()
        return rc, msg, launched

    def refused(**kw):
        rc, msg, launched = call(**kw)
        name = "si_cut_pair_ch: " if kw.get("chan") is not None else "si_cut_pair: "
        assert rc != 0 and msg.startswith(name) and launched == [], (rc, msg, launched)
        assert bool((out22 == 7.0).all()) and bool((out16 == 7.0).all())
        return msg

    # everything si_cut_rate refuses
    assert "x is NULL" in refused(x_=None) and "out22 is NULL" in refused(o22=None) and "out16 is NULL" in refused(o16=None)
    assert "host_frame is NULL" in refused(host=False) and "frame is NULL" in refused(devt=False)
    assert "filt22" in refused(a=False)
    assert "sr = 3999" in refused(sr_=3999) and "sr = 192001" in refused(sr_=192001) and "sr = 22050" in refused(sr_=22050)
    assert "n_file = 0" in refused(n=0) and "n_file = -1" in refused(n=-1)
    assert "at most" in refused(n=2 ** 31 - 1 - 2047)
    assert "at 22050 Hz" in refused(sr_=8000, n=2 ** 30, b=_sinc(eng._feed_filter16(8000)), a=_sinc(eng._feed_filter(8000)))
    for which in ("filt22", "filt16"):
        bad = _sinc(f22 if which == "filt22" else f16)
        bad.struct_size -= 8
        assert f"{which}: si_sinc_filter size mismatch" in refused(**{"a" if which == "filt22" else "b": bad})
        for kw in (dict(nwin=1), dict(num_table=0), dict(step=0), dict(scale=0.0), dict(scale=1.5), dict(win=None), dict(dwin=None)):
            s = _sinc(f22 if which == "filt22" else f16, **kw)
            assert f"{which}: bad filter table" in refused(**{"a" if which == "filt22" else "b": s})
        s = _sinc(f22 if which == "filt22" else f16, step=2)                                 # 16 385 taps per wing: no tile's samples fit
        assert f"{which}: bad filter table" in refused(**{"a" if which == "filt22" else "b": s})
    s = _sinc(f16, step=4)                                                                    # 8 193 taps per wing: 17 348 floats staged
    assert "filt16: bad filter table" in refused(b=s) and "staged samples per tile" in refused(b=s)
    assert "C = -1" in refused(Cn=-1) and "C = 65536" in refused(Cn=65536)
    assert "L22 = 0" in refused(L22=0) and "L22 = -3" in refused(L22=-3)
    # and what the pair adds
    assert "L16 = 0" in refused(L16=0) and "L16 = -3" in refused(L16=-3)
    last = (N22 - L22_0) // 441
    assert "frame[1]" in refused(frames=(0, -1)) and "frame[0]" in refused(frames=(last + 1, 0)) and "22.05 kHz" in refused(frames=(last + 1, 0))
    assert "frame[1]" in refused(frames=(0, 2 ** 31 - 1))
    msg = refused(frames=(0,), L22=1, L16=lim + 1, o16=out16)
    assert "frame[0]" in msg and "16 kHz samples" in msg and "ceil(N22 320 / 441)" in msg
    assert "filt16 is NULL at sr = 48000" in refused(b=False)
    c16 = _case(16000)
    x16k = torch.from_numpy(c16["v"]).to(dev)
    assert "filt16 is not NULL at sr = 16000" in refused(sr_=16000, x_=x16k, n=c16["v"].size, a=_sinc(eng._feed_filter(16000)))
    # the interleaved entry: the same, and its channels
    assert "channels = 0" in refused(chan=(0, 0)) and "channels = 9" in refused(chan=(9, 0))
    assert "channel = 2" in refused(chan=(2, 2)) and "channel = -1" in refused(chan=(2, -1))
    assert "L16 = 0" in refused(chan=(2, 1), L16=0) and "filt16 is NULL" in refused(chan=(2, 1), b=False) and "sr = 22050" in refused(chan=(2, 1), sr_=22050)
    # C = 0 launches nothing and succeeds, whatever the pointers; the good calls work, each in one launch of cut_rate's family
    rc, _, launched = call(frames=(), x_=None, o22=None, o16=None, host=False, devt=False)
    assert rc == 0 and launched == [] and bool((out22 == 7.0).all())
    e22, e16 = ctx.cut_pair(x, sr, [], L22_0, L16_0, f22, f16)
    assert e22.shape == (0, L22_0) and e16.shape == (0, L16_0)
    rc, _, launched = call(frames=(last, 0))
    assert rc == 0 and [(e["name"], e["launches"]) for e in launched] == [("cut_rate", 1)]
    assert not bool((out22 == 7.0).any()) and not bool((out16 == 7.0).any())
    rc, _, launched = call(frames=(last, 0), chan=(2, 1))
    assert rc == 0 and [(e["name"], e["launches"]) for e in launched] == [("cut_rate_ch", 1)]
    rc, _, launched = call(frames=(0, 1), sr_=16000, x_=x16k, n=c16["v"].size, a=_sinc(eng._feed_filter(16000)), b=False)
    assert rc == 0 and [(e["name"], e["launches"]) for e in launched] == [("cut_rate", 1)]


# ------------------------------------------------------------------------------------------------------------ stale scratch
def test_after_other_work_under_poisoned_allocations_the_bytes_are_a_fresh_context_s():
    """The launches are profiled in cut_rate's families, which tests/poison.py lists as holding no scratch: a call that follows other
    work on the same context (the detector, which owns scratch; a resample; a larger cut), with every torch.empty handed out as NaN,
    gives the bytes of a context that has done nothing else."""
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.native import NativeContext, make_desc
    assert P.family_of("cut_rate") in P.NO_SCRATCH_FAMILIES and P.family_of("cut_rate_ch") in P.NO_SCRATCH_FAMILIES
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    for sr in (48000, 16000):
        c = _case(sr)
        f22, f16 = _filters(eng, sr)
        x = torch.from_numpy(c["v"]).to(dev)
        x2 = torch.from_numpy(np.ascontiguousarray(np.stack([c["v"][::-1], c["v"]], axis=1))).to(dev)
        L22, L16 = 2 * T22 + 1, _l16(2 * T22 + 1)
        frames = [_last_frame(c, L22, L16), 0, 1]
        fresh = NativeContext(make_desc(HubertArch.tiny(), VocoderArch.tiny(), 50), dev)
        try:
            want = fresh.cut_pair(x, sr, frames, L22, L16, f22, f16) + fresh.cut_pair(x2, sr, frames, L22, L16, f22, f16, channel=1)
            torch.cuda.synchronize()
            want = [t.cpu() for t in want]
        finally:
            fresh.close()
        with P.poisoned_allocs():
            ctx.quiet_runs(x, 100.0, 3)
            eng.resample(x[None].to(torch.float32), sr, 22050)
            ctx.cut_pair(x, sr, [0], c["N22"], c["lim"], f22, f16)
            got = ctx.cut_pair(x, sr, frames, L22, L16, f22, f16) + ctx.cut_pair(x2, sr, frames, L22, L16, f22, f16, channel=1)
            torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(P.bits(a.cpu()), P.bits(b)) and bool(torch.isfinite(a).all()), sr
        assert torch.equal(P.bits(got[0].cpu()), P.bits(got[2].cpu())) and torch.equal(P.bits(got[1].cpu()), P.bits(got[3].cpu()))
