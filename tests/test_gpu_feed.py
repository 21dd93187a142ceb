"""si_cut_rate alone: the 22.05 kHz context clips cut straight out of a file at its own rate and sample type.  No model.

The reference is tests/feed_ref.py, the definition in numpy float64.  Every output must lie within
    2^-24 |y| + (2 H + 2) 2^-52 A,   A = sum |c x| over the sample's taps, H = taps per wing
of it: the one rounding to fp32, and the float64 sum, which the kernel's fma chain and numpy's separate multiply and add may spend
differently.  The share of outputs that equal fl32(y) bit for bit is reported with the ratios."""
import ctypes as C

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import feed_ref as F
from tests.harness import RatioSummary, build_engine

pytestmark = pytest.mark.gpu

T = native.CUT_RATE_TILE
RATES = [48000, 44100, 32000, 16000, 11025, 8000, 4000, 192000]
SUMMARY = RatioSummary()
SHARES = RatioSummary()                                # per rate: the share of outputs that do NOT equal fl32(y), worst call | mean
_CASES = {}


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", "fp32", key=("patch", "fp32"))


def _case(sr):
    """An int16 file whose 22.05 kHz axis holds a little over 2 T + 1 samples, and the reference of EVERY sample of that axis."""
    if sr not in _CASES:
        P, Q = G.rate_ratio(sr)
        n_file = -(-(2 * T + 300) * Q // P) + 3
        v = np.random.default_rng(sr).integers(-20000, 20001, size=n_file).astype(np.int16)
        N22 = F.n22(n_file, sr)
        y, A, _ = F.samples(v, np.arange(N22), sr)
        _CASES[sr] = dict(v=v, N22=N22, y=y, A=A, P=P, Q=Q)
    return _CASES[sr]


def _off_grid(t, off, dev):
    """t on the device, its first element `off` elements past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=dev)
    v = buf[off:off + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


def _both(v, dev, off32=0, off16=0):
    """The int16 file v on the device as int16 and as the fp32 file that holds v / 32768."""
    x16 = _off_grid(torch.from_numpy(v), off16, dev)
    x32 = _off_grid(torch.from_numpy(v.astype(np.float32) / np.float32(32768.0)), off32, dev)
    return x32, x16


def _check(out, starts, L, y, A, sr, label):
    """out (C, L) host fp32 against the reference of the whole axis.  -> the share of outputs that equal fl32(y)."""
    j = np.asarray(starts, dtype=np.int64)[:, None] + np.arange(L)[None, :]
    ref, E = y[j], F.kernel_bound(y[j], A[j], sr)
    ratio = np.abs(out.astype(np.float64) - ref) / np.maximum(E, 1e-300)
    seam = (np.arange(L) % T == 0) | (np.arange(L) % T == T - 1) | (np.arange(L) == L - 1)
    near = float(ratio[:, seam].max())
    rest = float(ratio[:, ~seam].max()) if (~seam).any() else 0.0
    SUMMARY.note(label, near, rest)
    assert near <= 1.0 and rest <= 1.0, (label, L, near, rest)
    return float(np.mean(out == ref.astype(np.float32)))


@pytest.mark.parametrize("sr", RATES)
def test_bound_sample_types_and_tile_seams(sr):
    """L in {1, T - 1, T, T + 1, 2 T + 1}; starts on and off tile multiples, at the recording's start (left taps before the file) and
    against its end (right taps past the file, and the last sample, which is interpolated: 4.17 (b)), overlapping and unsorted, several
    clips per call; every integer-time output (j a multiple of P) of the axis among them.  The fp32 file that holds v / 32768 and the
    int16 file v give the same bytes, and a repeated call gives them again."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    c = _case(sr)
    N22, P = c["N22"], c["P"]
    x32, x16 = _both(c["v"], dev)
    filt = eng._feed_filter(sr)
    seen = np.zeros(N22, dtype=bool)
    shares = []
    for L in (1, T - 1, T, T + 1, 2 * T + 1):
        starts = [s for s in (N22 - L, 0, T, 77, T + 1, 77, P, 2 * P - 1, N22 - L - 1) if 0 <= s and s + L <= N22]
        assert len(starts) >= 5 and starts[0] + L == N22 and sorted(starts) != starts
        a = ctx.cut_rate(x32, sr, starts, L, filt)
        b = ctx.cut_rate(x16, sr, starts, L, filt)
        again = ctx.cut_rate(x16, sr, starts, L, filt, out=torch.full((len(starts), L), 7.0, device=dev))
        torch.cuda.synchronize()
        out = a.cpu().numpy()
        assert out.shape == (len(starts), L)
        assert np.array_equal(out.view(np.int32), b.cpu().numpy().view(np.int32)), (sr, L, "fp32 | int16")
        assert np.array_equal(out.view(np.int32), again.cpu().numpy().view(np.int32)), (sr, L, "repeated call")
        shares.append(_check(out, starts, L, c["y"], c["A"], sr, f"cut_rate {sr} Hz"))
        for s in starts:
            seen[s:s + L] = True
    assert seen[np.arange(0, N22, P)].all() and seen[N22 - 1] and seen[0]            # every integer-time output, both ends
    assert abs(c["y"][N22 - 1]) > 0 and float(np.abs(c["y"]).max()) > 0.1
    SHARES.note(f"cut_rate {sr} Hz", 1.0 - min(shares), 1.0 - float(np.mean(shares)))


def test_kernel_summary():
    SUMMARY.report()
    SHARES.report(line="   SUMMARY {key}: share of outputs that differ from fl32(y): worst call {near:.4f}, mean {rest:.4f} of its five calls")


@pytest.mark.parametrize("sr", [48000, 16000, 192000])
def test_short_files(sr):
    """A file shorter than one wing, and a file of one sample: every tap count is cut by the file's ends."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    filt = eng._feed_filter(sr)
    for n_file in (F.reach(sr) - 3, 1):
        v = np.random.default_rng(n_file).integers(-20000, 20001, size=n_file).astype(np.int16)
        N22 = F.n22(n_file, sr)
        y, A, _ = F.samples(v, np.arange(N22), sr)
        x32, x16 = _both(v, dev, 1, 1)
        for starts, L in (([0], N22), ([N22 - 1, 0], 1)):
            a = ctx.cut_rate(x32, sr, starts, L, filt)
            b = ctx.cut_rate(x16, sr, starts, L, filt)
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            _check(a.cpu().numpy(), starts, L, y, A, sr, f"cut_rate short {sr} Hz")
        assert np.abs(y).max() > 0
    SUMMARY.report(keys=[f"cut_rate short {sr} Hz"])


def test_base_pointers_off_the_16_byte_grid():
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    for sr in (48000, 8000):
        c = _case(sr)
        filt = eng._feed_filter(sr)
        starts, L = [0, 77, c["N22"] - T - 1], T + 1
        x32, x16 = _both(c["v"], dev)
        want = ctx.cut_rate(x32, sr, starts, L, filt)
        for o32, o16 in ((1, 1), (2, 3), (3, 7)):
            y32, y16 = _both(c["v"], dev, o32, o16)
            assert y32.data_ptr() % 16 == 4 * o32 and y16.data_ptr() % 16 == 2 * o16
            a, b = ctx.cut_rate(y32, sr, starts, L, filt), ctx.cut_rate(y16, sr, starts, L, filt)
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), want.view(torch.int32)) and torch.equal(b.view(torch.int32), want.view(torch.int32)), (sr, o32, o16)
        _check(want.cpu().numpy(), starts, L, c["y"], c["A"], sr, f"cut_rate off-grid {sr} Hz")


@pytest.mark.parametrize("sr", [48000, 192000])
def test_the_time_is_64_bit(sr):
    """An int16 file of 15 M samples: the last clip's j Q lies above 2^31 (and the file index, at 192 kHz, above 2^23: no fp32 time)."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    P, Q = G.rate_ratio(sr)
    n_file = 15_000_000
    v = np.random.default_rng(7).integers(-20000, 20001, size=n_file).astype(np.int16)
    N22 = F.n22(n_file, sr)
    L = T + 1
    starts = [N22 - L, 2 ** 31 // Q - 5]
    assert all(s * Q + 5 * Q > 2 ** 31 or s * Q < 2 ** 31 < (s + L) * Q for s in starts) and starts[1] + L <= N22
    out = ctx.cut_rate(torch.from_numpy(v).to(dev), sr, starts, L, eng._feed_filter(sr))
    torch.cuda.synchronize()
    j = np.concatenate([np.arange(s, s + L) for s in starts])
    y, A, _ = F.samples(v, j, sr)
    got = out.cpu().numpy().reshape(-1).astype(np.float64)
    ratio = float((np.abs(got - y) / F.kernel_bound(y, A, sr)).max())
    SUMMARY.note(f"cut_rate 64-bit {sr} Hz", ratio, ratio)
    SUMMARY.report(keys=[f"cut_rate 64-bit {sr} Hz"])
    assert float(np.abs(y).max()) > 0.1


def test_refusals_launch_nothing():
    """Straight at the C ABI: every malformed call returns an error code and a message naming the entry and the argument, launches
    nothing and leaves the output untouched."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    sr = 48000
    c = _case(sr)
    N22, n_file = c["N22"], c["v"].size
    x = torch.from_numpy(c["v"]).to(dev)
    f0 = eng._feed_filter(sr)
    L0 = 100
    out = torch.full((2, L0), 7.0, device=dev)

    def filt(**kw):
        d = dict(nwin=f0["win"].numel(), num_table=f0["num_table"], step=f0["step"], scale=f0["scale"], win=f0["win"].data_ptr(), dwin=f0["dwin"].data_ptr())
        d.update(kw)
        return native.SincFilter(C.sizeof(native.SincFilter), d["nwin"], d["num_table"], d["step"], 0, 0, d["scale"], 0.0, d["win"], d["dwin"], None)

    def call(starts=(0, 50), f=None, sr_=sr, n=n_file, o=out, x_=x, L=L0, Cn=None, host=True, devt=True):
        h = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
        d = torch.from_numpy(h).to(dev)
        f = filt() if f is None else f
        ctx.profile_start(100)
        rc = ctx.lib.si_cut_rate(ctx._h, native._ptr(x_), 1, n, sr_, h.ctypes.data_as(C.c_void_p) if host else None, native._ptr(d) if devt else None,
                                 len(h) if Cn is None else Cn, L, C.byref(f) if f else None, native._ptr(o), ctx._stream())
        msg = ctx.lib.si_last_error(ctx._h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        torch.cuda.synchronize()
        return rc, msg, launched

    def refused(**kw):
        rc, msg, launched = call(**kw)
        assert rc != 0 and msg.startswith("si_cut_rate: ") and launched == [], (rc, msg, launched)
        assert bool((out == 7.0).all())
        return msg

    assert "x is NULL" in refused(x_=None) and "out is NULL" in refused(o=None)
    assert "host_start is NULL" in refused(host=False) and "start is NULL" in refused(devt=False)
    assert "filt" in refused(f=False)
    assert "sr = 3999" in refused(sr_=3999) and "sr = 192001" in refused(sr_=192001) and "sr = 22050" in refused(sr_=22050)
    assert "n_file = 0" in refused(n=0) and "n_file = -1" in refused(n=-1)
    assert "n_file" in refused(n=2 ** 31 - 1 - 2047) and "at most" in refused(n=2 ** 31 - 1 - 2047)
    assert "at 22050 Hz" in refused(sr_=8000, n=2 ** 30)                                      # 2^30 samples at 8 kHz are 2.96e9 at 22.05 kHz
    bad = filt()
    bad.struct_size -= 8
    assert "si_sinc_filter size mismatch" in refused(f=bad)
    for kw in (dict(nwin=1), dict(num_table=0), dict(step=0), dict(scale=0.0), dict(scale=1.5), dict(win=None), dict(dwin=None)):
        assert "filt: bad filter table" in refused(f=filt(**kw))
    assert "filt: bad filter table" in refused(f=filt(step=2))                                # 16 385 taps per wing: no tile's samples fit
    assert "C = -1" in refused(Cn=-1) and "C = 65536" in refused(Cn=65536)
    assert "L = 0" in refused(L=0) and "L = -3" in refused(L=-3)
    assert "start[1]" in refused(starts=(0, -1)) and "start[0]" in refused(starts=(N22 - L0 + 1, 0))
    assert "start[1]" in refused(starts=(0, 2 ** 31 - 1))                                     # start + L past int32
    # C = 0 launches nothing and succeeds, whatever the pointers; the good call works
    rc, _, launched = call(starts=(), x_=None, o=None, host=False, devt=False)
    assert rc == 0 and launched == [] and bool((out == 7.0).all())
    assert ctx.cut_rate(x, sr, [], L0, f0).shape == (0, L0)
    rc, _, launched = call(starts=(N22 - L0, 0))
    assert rc == 0 and [(e["name"], e["launches"]) for e in launched] == [("cut_rate", 1)] and not bool((out == 7.0).any())
