"""The three kernels of DESIGN.md 4.18 alone: si_quiet_runs_ch, si_cut_rate_ch and si_patch_rate_ch on interleaved (n, ch) files.  No model.

The contract is bytes: whatever a call gives for channel c is what the mono entry point (si_quiet_runs, si_cut_rate, si_patch_rate) gives
on the de-interleaved channel x[:, c].contiguous(), and nothing else is written.  Detection is compared with tests/detect_ref.py as it
stands: fed x[:, c], or for joint detection the 0 / 1 signal "some channel is loud" at threshold 0 (tests/channels_ref.py).  The other
channels hold independent noise at about ten times the amplitude, so a leak between channels cannot hide in a rounding."""
import ctypes as C

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import channels_ref as CH
from tests import detect_ref as D
from tests import feed_ref as F
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

T = native.CUT_RATE_TILE
SENTINEL = -7
DTYPES = [np.float32, np.int16]


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", "fp32", key=("patch", "fp32"))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.int16 else torch.int32)


# ------------------------------------------------------------------------------------------------------------ detection
def _runs(ctx, x, channel, thr, min_len, max_runs=4096, off=0):
    """si_quiet_runs_ch on the host (n, ch) array x -> (total, the rows written, the rows past them)."""
    view = CH.on_device(x, ctx.device, off)
    runs = torch.full((max_runs + 8, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
    _, n_runs = ctx.quiet_runs(view, thr, min_len, max_runs, runs=runs, channel=channel)
    total = int(n_runs.item())
    rows = runs.cpu().numpy()
    k = min(total, max_runs)
    return total, rows[:k], rows[k:]


def _want(x, channel, thr, min_len):
    return CH.joint_runs_ref(x, thr, min_len) if channel < 0 else D.quiet_runs_ref(x[:, channel], thr, min_len)


def _check(ctx, x, channel, thr, min_len, what, **kw):
    want = _want(x, channel, thr, min_len)
    total, rows, rest = _runs(ctx, x, channel, thr, min_len, **kw)
    assert total == len(want), (what, channel, total, len(want))
    assert len(rows) == min(total, kw.get("max_runs", 4096)) and np.array_equal(rows, want[:len(rows)]), (what, channel, rows[:8].tolist(), want[:8].tolist())
    assert np.all(rest == SENTINEL), (what, channel)
    return want


def _seam_file(n, ch, dtype, k):
    """Seam case k of tests/detect_ref.py in channel 0 and other seam cases in the other channels, so that every channel has runs of
    its own on and across the chunk seams.  The masks of channels 2 .. (and of channel 1 for even k) also hold channel 0's quiet
    samples: the joint answer is then channel 0's pattern for even k and its intersection with channel 1's for odd k, never empty
    by accident however many channels there are.  -> (name, x (n, ch), min_len)."""
    cases = D.seam_cases(n)
    name, mask0, min_len = cases[k]
    masks = [mask0]
    for c in range(1, ch):
        other = cases[(k + 5 * c) % len(cases)][1]
        masks.append(other if c == 1 and k % 2 else other | mask0)
    cols = [D.materialize(m, dtype, 10 * k + c) for c, m in enumerate(masks)]
    return name, np.ascontiguousarray(np.stack(cols, axis=1)), min_len


@pytest.mark.parametrize("n", [1, 7, 2047, 2048, 2049, 4101])
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_runs_of_every_channel_and_joint_at_the_chunk_seams(dtype, ch, n):
    ctx = _engine().ctx
    found = joint = 0
    for k in range(len(D.seam_cases(n))):
        name, x, min_len = _seam_file(n, ch, dtype, k)
        for c in range(ch):
            found += len(_check(ctx, x, c, D.THR[dtype], min_len, (n, ch, name)))
        joint += len(_check(ctx, x, -1, D.THR[dtype], min_len, (n, ch, name, "joint")))
    assert found > 0 and joint > 0


def test_a_stretch_quiet_in_one_channel_only_is_no_joint_dropout():
    ctx = _engine().ctx
    for dtype in DTYPES:
        n = 4101
        quiet0 = D.mask_of(n, [(100, 300), (2000, 2100), (4000, 4101)])         # channel 0: three stretches, one across the seam at 2048
        quiet1 = D.mask_of(n, [(150, 200), (2040, 2060)])                       # channel 1: loud through most of them
        x = np.stack([D.materialize(quiet0, dtype, 1), D.materialize(quiet1, dtype, 2)], axis=1)
        assert _check(ctx, x, 0, D.THR[dtype], 1, "ch 0").tolist() == [[100, 200], [2000, 100], [4000, 101]]
        assert _check(ctx, x, 1, D.THR[dtype], 1, "ch 1").tolist() == [[150, 50], [2040, 20]]
        assert _check(ctx, x, -1, D.THR[dtype], 1, "joint").tolist() == [[150, 50], [2040, 20]]
        assert _check(ctx, x, -1, D.THR[dtype], 21, "joint, min_len 21").tolist() == [[150, 50]]


def test_value_edges_per_channel_and_joint():
    ctx = _engine().ctx
    a = np.array([np.nan, -0.0, 1e-40, np.inf, 0.0, 0.25, 0.0, 0.0, 1.0], dtype=np.float32)
    b = np.array([0.0, 0.0, 0.0, 0.0, -0.0, -0.25, np.nan, 0.5, 0.0], dtype=np.float32)
    x = np.stack([a, b], axis=1)
    assert _check(ctx, x, 0, 0.0, 1, "thr 0").tolist() == [[1, 1], [4, 1], [6, 2]]
    assert _check(ctx, x, -1, 0.0, 1, "joint thr 0").tolist() == [[1, 1], [4, 1]]
    assert _check(ctx, x, -1, 0.25, 1, "joint == thr").tolist() == [[1, 2], [4, 2]]              # |x| = thr is quiet, NaN loud in either channel
    p = np.array([[-32768, 0], [3, -3], [-3, 4], [0, -32768], [0, 0]], dtype=np.int16)
    assert _check(ctx, p, 0, 3.0, 1, "pcm").tolist() == [[1, 4]]
    assert _check(ctx, p, -1, 3.0, 1, "pcm joint").tolist() == [[1, 1], [4, 1]]
    assert _check(ctx, p, -1, 32767.0, 1, "pcm joint 32767").tolist() == [[1, 2], [4, 1]]      # |-32768| = 32768, taken in int32
    assert _check(ctx, p, -1, 32768.0, 1, "pcm joint 32768").tolist() == [[0, 5]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_bases_off_the_16_byte_grid(dtype):
    ctx = _engine().ctx
    for ch, n in ((2, 2049), (3, 4101), (8, 2047)):
        for k in (5, 9, len(D.seam_cases(n)) - 3):
            name, x, min_len = _seam_file(n, ch, dtype, k)
            for off in (1, 2, 3):
                for c in (0, ch - 1, -1):
                    _check(ctx, x, c, D.THR[dtype], min_len, (n, ch, name, off), off=off)


def test_the_carry_scan_across_its_tile_seam_with_two_channels():
    """1027 chunks and 5 sample times at ch = 2: channel 0 holds a run across the carry scan's tile seam with whole quiet chunks on both
    sides, channel 1 a run that ends exactly on it; their intersection is the joint answer."""
    ctx = _engine().ctx
    n, seam, q, q2 = D.tile_seam_case()
    assert n // D.CHUNK == 1027 and n % D.CHUNK == 5
    for dtype in DTYPES:
        x = np.stack([D.materialize(q, dtype, 0), D.materialize(q2, dtype, 1)], axis=1)
        w0 = _check(ctx, x, 0, D.THR[dtype], 64, "tile seam ch 0", max_runs=1 << 18)
        w1 = _check(ctx, x, 1, D.THR[dtype], 64, "tile seam ch 1", max_runs=1 << 18)
        wj = _check(ctx, x, -1, D.THR[dtype], 1, "tile seam joint", max_runs=1 << 18)
        assert [seam - D.CHUNK - 1000, 2 * D.CHUNK + 1200] in w0.tolist() and [seam - D.CHUNK - 1000, D.CHUNK + 1000] in w1.tolist()
        assert [seam - D.CHUNK - 1000, D.CHUNK + 1000] in wj.tolist()


def test_max_runs_and_one_channel_bytes():
    eng = _engine()
    ctx = eng.ctx
    col = D.materialize(np.arange(4101) % 2 == 0, np.float32)
    x = CH.around(col, 1, 3)
    want = D.quiet_runs_ref(col, D.THR[np.float32], 1)
    assert len(want) == 2051
    for cap in (100, 2051, 2052, 1):
        total, rows, rest = _runs(ctx, x, 1, D.THR[np.float32], 1, max_runs=cap)
        assert total == 2051 and np.array_equal(rows, want[:cap]) and np.all(rest == SENTINEL), cap
    dev = torch.from_numpy(x).to(eng.device)
    runs, n_runs = ctx.quiet_runs(dev, D.THR[np.float32], 1, 0, channel=1)                       # max_runs = 0 counts only
    assert runs is None and int(n_runs.item()) == 2051
    assert np.array_equal(eng.find_quiet_runs(x, D.THR[np.float32], channel=1).cpu().numpy(), want)
    assert eng.find_quiet_runs(x, D.THR[np.float32], channel=0).shape == (0, 2) and eng.find_quiet_runs(x, D.THR[np.float32], channel=-1).shape == (0, 2)
    with pytest.raises(ValueError, match="needs channel"):
        eng.find_quiet_runs(x, D.THR[np.float32])
    # channels = 1: channel 0 and -1 give si_quiet_runs' bytes, sentinel rows included
    for dtype in DTYPES:
        for n in (7, 2049, 4101):
            for name, mask, min_len in D.seam_cases(n)[4:12]:
                y = D.materialize(mask, dtype, n)
                mono = torch.full((600, 2), SENTINEL, dtype=torch.int32, device=eng.device)
                _, cnt = ctx.quiet_runs(torch.from_numpy(y).to(eng.device), D.THR[dtype], min_len, 592, runs=mono)
                for c in (0, -1):
                    got = torch.full((600, 2), SENTINEL, dtype=torch.int32, device=eng.device)
                    _, cnt_c = ctx.quiet_runs(torch.from_numpy(y[:, None].copy()).to(eng.device), D.THR[dtype], min_len, 592, runs=got, channel=c)
                    assert torch.equal(got, mono) and int(cnt_c.item()) == int(cnt.item()), (n, name, c)


# ------------------------------------------------------------------------------------------------------------ si_cut_rate_ch
def _feed_file(sr, dtype, seed=0):
    """One channel of a file whose 22.05 kHz axis holds a little over 2 T + 1 samples, at a tenth of the neighbours' amplitude."""
    P, Q = G.rate_ratio(sr)
    n_file = -(-(2 * T + 300) * Q // P) + 3
    return CH.noise(n_file, dtype, sr + seed, 0.09 if dtype is np.float32 else 3000)


def _cut_both(eng, x, c, sr, starts, L, off=0):
    """(si_cut_rate_ch on channel c of the interleaved host file x, si_cut_rate on the de-interleaved channel)."""
    filt = eng._feed_filter(sr)
    got = eng.ctx.cut_rate(CH.on_device(x, eng.device, off), sr, starts, L, filt, channel=c)
    want = eng.ctx.cut_rate(torch.from_numpy(np.ascontiguousarray(x[:, c])).to(eng.device), sr, starts, L, filt)
    torch.cuda.synchronize()
    return got, want


@pytest.mark.parametrize("sr", [48000, 44100, 16000, 8000])
@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cut_rate_ch_equals_cut_rate_on_the_channel(dtype, ch, sr):
    """L in {1, T - 1, T, T + 1, 2 T + 1}; starts at the recording's start (left taps before the file: they must read zero, not the
    previous sample time's other channel), against its end (right taps past the file), overlapping and unsorted."""
    eng = _engine()
    N22 = F.n22(_feed_file(sr, dtype).size, sr)
    for c in range(ch):
        col = _feed_file(sr, dtype, c)
        x = CH.around(col, c, ch, sr)
        for L in (1, T - 1, T, T + 1, 2 * T + 1):
            starts = [s for s in (N22 - L, 0, T, 77, T + 1, 77, N22 - L - 1) if 0 <= s and s + L <= N22]
            assert len(starts) >= 5 and starts[0] + L == N22 and sorted(starts) != starts
            got, want = _cut_both(eng, x, c, sr, starts, L)
            assert got.shape == (len(starts), L) and torch.equal(_bits(got), _bits(want)), (sr, ch, c, L, int((_bits(got) != _bits(want)).sum()))
            assert float(want.abs().max()) > 0


@pytest.mark.parametrize("sr", [48000, 16000])
def test_cut_rate_ch_short_files_and_bases_off_the_grid(sr):
    eng = _engine()
    for dtype in DTYPES:
        for n_file in (1, F.reach(sr) - 3):                            # one sample time; shorter than one wing
            N22 = F.n22(n_file, sr)
            for ch in (2, 3):
                col = CH.noise(n_file, dtype, n_file, 0.09 if dtype is np.float32 else 3000)
                x = CH.around(col, ch - 1, ch, n_file)
                for starts, L in (([0], N22), ([N22 - 1, 0], 1)):
                    got, want = _cut_both(eng, x, ch - 1, sr, starts, L, off=1)
                    assert torch.equal(_bits(got), _bits(want)) and float(want.abs().max()) > 0, (sr, n_file, ch)
        col = _feed_file(sr, dtype)
        N22 = F.n22(col.size, sr)
        for ch, c in ((2, 0), (3, 1)):
            x = CH.around(col, c, ch, 3)
            for off in (1, 2, 3):
                got, want = _cut_both(eng, x, c, sr, [0, 77, N22 - T - 1], T + 1, off=off)
                assert torch.equal(_bits(got), _bits(want)), (sr, ch, off)


# ------------------------------------------------------------------------------------------------------------ si_patch_rate_ch
@pytest.mark.parametrize("sr", [48000, 16000])
@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("pcm", [False, True], ids=["fp32", "int16"])
def test_patch_rate_ch_writes_its_channel_as_patch_rate_and_nothing_else(pcm, ch, sr):
    """Fades 0 and the default, gain given and NULL, a table that also names a window and a context no span uses.  `out` pre-filled
    with a copy of orig and with a sentinel pattern: channel c equals si_patch_rate's output on the de-interleaved channel (and its
    pre-fill), every other element what it held before the call."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    filt = eng._rate_filter(sr)
    for fade_f in (0, G.file_fade(5.0, sr)):
        case = CH.rate_case(sr, fade_f)
        o_col = (case["orig"].numpy() * 32767.0).astype(np.int16) if pcm else case["orig"].numpy()
        gen3 = case["gen"].to(dev)
        mono_table = native.RateTable(case["spans"], case["windows"], case["chunks"], 2, fade_f, dev)
        table = native.RateTable(case["spans"], case["windows3"], case["chunks"], 3, fade_f, dev)
        for c in (0, ch - 1):
            x = CH.around(o_col, c, ch, fade_f + c)
            orig = CH.on_device(x, dev, 1 + c)
            rng = np.random.default_rng(c)
            sentinel = rng.integers(-30000, 30000, x.shape).astype(np.int16) if pcm else (rng.random(x.shape).astype(np.float32) + 2.0)
            for gain_host in (None, np.array([0.8, 1.3, 55.0], dtype=np.float32)):
                gain3 = None if gain_host is None else torch.from_numpy(gain_host).to(dev)
                gain2 = None if gain_host is None else gain3[:2].contiguous()
                for fill in (x, sentinel):
                    out = CH.on_device(fill, dev, 3 - c)
                    ctx.patch_rate(orig, sr, table, gen3, filt, out, gain3, channel=c)
                    want = torch.from_numpy(np.ascontiguousarray(fill[:, c])).to(dev)
                    ctx.patch_rate(torch.from_numpy(np.ascontiguousarray(x[:, c])).to(dev), sr, mono_table, gen3[:2].contiguous(), filt, want, gain2)
                    torch.cuda.synchronize()
                    assert torch.equal(_bits(out[:, c]), _bits(want)), (sr, ch, c, fade_f, int((_bits(out[:, c]) != _bits(want)).sum()))
                    others = [k for k in range(ch) if k != c]
                    assert torch.equal(_bits(out[:, others]), _bits(torch.from_numpy(np.ascontiguousarray(fill[:, others])).to(dev))), (sr, ch, c, fade_f)
                    assert int((_bits(want) != _bits(torch.from_numpy(np.ascontiguousarray(fill[:, c])).to(dev))).sum()) > sum(s[1] for s in case["spans"][:4]) // 2


# ------------------------------------------------------------------------------------------------------------ 64-bit element offsets
def test_element_offsets_past_2_to_the_31():
    """One int16 tensor of 2^28 + 5 sample times x 8 channels (4.3 GB, allocated on the device): the elements of its last five sample
    times lie at and past 2^31, where an int32 offset has wrapped.  Those five hold a dropout of channel 7 alone and a joint one, the
    end of a clip and the end of a patched span; the cut and the patch are compared with the mono calls on the last k sample times
    of channel 7, k chosen so that the cut-off front is a whole number of 22.05 kHz samples."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    n, ch, sr, K = 2 ** 28 + 5, 8, 48000, 16384
    P, Q = G.rate_ratio(sr)
    k = n % Q + 25 * Q
    shift22, shift = (n - k) // Q * P, n - k
    assert (n - 5) * ch == 2 ** 31 and (n - k) % Q == 0 and k < K
    x = torch.zeros((n, ch), dtype=torch.int16, device=dev)
    try:
        tail = np.stack([CH.noise(K, np.int16, c, 3000 if c == 7 else 30000) for c in range(ch)], axis=1)
        tail[K - 100:K - 90, 7] = 0                                   # a dropout of channel 7 alone
        tail[K - 50:K - 45, :] = 0                                    # a joint dropout
        tail[K - 5, :] = 0                                            # past 2^31: a joint one of one sample time ...
        tail[K - 3:, 7] = 0                                           # ... and one of channel 7 alone that reaches the file's end
        x[n - K:] = torch.from_numpy(tail).to(dev)
        assert eng.find_quiet_runs(x, 0.0, 1, channel=7).tolist() == [[0, n - K], [n - 100, 10], [n - 50, 5], [n - 5, 1], [n - 3, 3]]
        assert eng.find_quiet_runs(x, 0.0, 1, channel=-1).tolist() == [[0, n - K], [n - 50, 5], [n - 5, 1]]
        assert eng.find_quiet_runs(x, 0.0, 1, channel=0).tolist() == [[0, n - K], [n - 50, 5], [n - 5, 1]]
        col = x[n - k:, 7].contiguous()
        # one clip of T + 1 samples at the end of the 22.05 kHz axis: its last samples read the file's last sample times
        N22, N22s = F.n22(n, sr), F.n22(k, sr)
        assert N22 == shift22 + N22s
        fin = eng._feed_filter(sr)
        got = ctx.cut_rate(x, sr, [N22 - (T + 1)], T + 1, fin, channel=7)
        want = ctx.cut_rate(col, sr, [N22s - (T + 1)], T + 1, fin)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want)) and float(want.abs().max()) > 0.01 and float(want[0, -8:].abs().max()) > 0
        # one span that ends with the file, cross-faded in front, its window on the 22.05 kHz axis: the last chunk is written to its end
        fade_f = G.file_fade(5.0, sr)
        filt = eng._rate_filter(sr)
        s, l = n - 700, 700
        ws = (s - fade_f) * P // Q - filt["reach"] - 2
        wl = N22 - ws
        gen = ((torch.rand(1, wl + 5, generator=torch.Generator().manual_seed(3)) * 2 - 1) * 0.3).to(dev)
        region = lambda a, lim: G.region_chunks(G.file_regions([(a, l)], [lim], fade_f))
        table = native.RateTable([(s, l, 0, n)], [(0, ws, wl, N22)], region(s, n), 1, fade_f, dev)
        mono = native.RateTable([(s - shift, l, 0, k)], [(0, ws - shift22, wl, N22s)], region(s - shift, k), 1, fade_f, dev)
        out = x.clone()
        ctx.patch_rate(x, sr, table, gen, filt, out, None, channel=7)
        want = col.clone()
        ctx.patch_rate(col, sr, mono, gen, filt, want, None)
        torch.cuda.synchronize()
        assert torch.equal(out[n - k:, 7], want) and int((want != col).sum()) > l and int((want[-5:] != col[-5:]).sum()) >= 3
        assert torch.equal(out[n - K:, :7], x[n - K:, :7]) and torch.equal(out[:n - k, 7], x[:n - k, 7])
        del out
    finally:
        del x
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_argument_and_launch_nothing():
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    lib, h = ctx.lib, ctx._h
    sr, fade_f = 48000, 240
    case = CH.rate_case(sr, fade_f)
    n = case["orig"].numel()
    x = torch.from_numpy(CH.around(case["orig"].numpy(), 0, 2)).to(dev)
    out = torch.full((n, 2), 7.0, device=dev)
    runs = torch.full((16, 2), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    clips = torch.full((2, 100), 7.0, device=dev)
    table = native.RateTable(case["spans"], case["windows"], case["chunks"], 2, fade_f, dev)
    gen = case["gen"][:2].contiguous().to(dev)
    host = np.array([0, 50], dtype=np.int32)
    start = torch.from_numpy(host).to(dev)
    P = native._ptr

    def sinc(f):
        return native.SincFilter(C.sizeof(native.SincFilter), f["win"].numel(), int(f["num_table"]), int(f["step"]), 0, 0, float(f["scale"]), 0.0,
                                 f["win"].data_ptr(), f["dwin"].data_ptr(), None)

    f_feed, f_rate, st = sinc(eng._feed_filter(sr)), sinc(eng._rate_filter(sr)), table.struct()

    def detect(channels=2, channel=0, x_=x, n_=n, thr=0.0):
        return lib.si_quiet_runs_ch(h, P(x_), 0, n_, channels, channel, thr, 1, P(runs), 16, P(cnt), ctx._stream())

    def cut(channels=2, channel=0, x_=x, n_=n, sr_=sr, L=100):
        return lib.si_cut_rate_ch(h, P(x_), 0, n_, channels, channel, sr_, host.ctypes.data_as(C.c_void_p), P(start), 2, L, C.byref(f_feed), P(clips),
                                  ctx._stream())

    def patch(channels=2, channel=0, x_=x, n_=n, sr_=sr, o=out):
        return lib.si_patch_rate_ch(h, P(x_), 0, n_, channels, channel, sr_, C.byref(st), P(gen), gen.shape[1], None, C.byref(f_rate), P(o), ctx._stream())

    def refused(call, name, msg, **kw):
        ctx.profile_start(100)
        rc = call(**kw)
        err = lib.si_last_error(h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        assert rc == -1 and launched == [] and err.startswith(name + ": ") and msg in err, (name, kw, rc, err, launched)      # SI_EINVAL

    for call, name, lowest in ((detect, "si_quiet_runs_ch", -1), (cut, "si_cut_rate_ch", 0), (patch, "si_patch_rate_ch", 0)):
        refused(call, name, "channels = 0, outside 1 .. SI_MAX_CHANNELS = 8", channels=0)
        refused(call, name, "channels = 9, outside 1 .. SI_MAX_CHANNELS = 8", channels=9)
        refused(call, name, "channels = -1", channels=-1)
        refused(call, name, f"channel = 2, outside {lowest} .. 1", channel=2)
        refused(call, name, f"channel = {lowest - 1}, outside {lowest} .. 1", channel=lowest - 1)
        refused(call, name, f"channel = 8, outside {lowest} .. 7", channels=8, channel=8)
    # what the mono siblings refuse, under the new names
    refused(detect, "si_quiet_runs_ch", "x is NULL", x_=None)
    refused(detect, "si_quiet_runs_ch", "n = 0 samples", n_=0)
    refused(detect, "si_quiet_runs_ch", "n = 2147481600 samples", n_=2 ** 31 - 1 - 2047)
    refused(detect, "si_quiet_runs_ch", "is negative or NaN", thr=-1.0)
    refused(cut, "si_cut_rate_ch", "x is NULL", x_=None)
    refused(cut, "si_cut_rate_ch", "sr = 22050", sr_=22050)
    refused(cut, "si_cut_rate_ch", "n_file = 0", n_=0)
    refused(cut, "si_cut_rate_ch", "L = 0", L=0)
    refused(cut, "si_cut_rate_ch", "start[0]", n_=100)
    refused(patch, "si_patch_rate_ch", "NULL / empty", o=None)
    refused(patch, "si_patch_rate_ch", "out is orig", o=x)
    refused(patch, "si_patch_rate_ch", "22050", sr_=22050)
    refused(patch, "si_patch_rate_ch", "outside the recording", n_=n - 200)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((clips == 7.0).all()) and bool((runs == SENTINEL).all()) and int(cnt.item()) == SENTINEL
    # the same arguments unchanged are served, under the new family names; the mono calls keep theirs
    ctx.profile_start(100)
    assert detect() == 0 and cut() == 0 and patch() == 0
    prof = {e["name"]: e["launches"] for e in ctx.profile_stop() if e["launches"] > 0}
    assert prof == {"detect_bits_ch": 1, "detect_carry": 1, "detect_count": 1, "detect_offsets": 1, "detect_emit": 1, "cut_rate_ch": 1, "patch_rate_ch": 1}, prof
    torch.cuda.synchronize()
    assert not bool((clips == 7.0).any()) and bool((out[:, 1] == 7.0).all()) and not bool((out[:, 0] == 7.0).all())
    ctx.profile_start(100)
    ctx.quiet_runs(x[:, 0].contiguous(), 0.0, 1, 16)
    ctx.cut_rate(x[:, 0].contiguous(), sr, [0, 50], 100, eng._feed_filter(sr))
    ctx.patch_rate(x[:, 0].contiguous(), sr, table, gen, eng._rate_filter(sr), out[:, 0].contiguous())
    prof = {e["name"] for e in ctx.profile_stop() if e["launches"] > 0}
    assert prof == {"detect_bits", "detect_carry", "detect_count", "detect_offsets", "detect_emit", "cut_rate", "patch_rate"}, prof


def test_every_refusal_of_the_mono_siblings_under_the_new_names():
    """The validation is the mono entry's own (one shared function per pair), so every case that tests/test_gpu_detect.py,
    test_gpu_feed.py and test_gpu_rate.py put to si_quiet_runs, si_cut_rate and si_patch_rate is put to the interleaved entry here,
    on a two-channel file: SI_EINVAL, the message under the new name, nothing launched, no output touched."""
    import re
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    lib, h = ctx.lib, ctx._h
    sr, fade_f = 48000, 240
    case = CH.rate_case(sr, fade_f)
    spans, wins, chunks, lrow = case["spans"], case["windows"], case["chunks"], case["lrow"]
    n = case["orig"].numel()
    P, Q = G.rate_ratio(sr)
    N22 = -(-n * P // Q)
    x = torch.from_numpy(CH.around(case["orig"].numpy(), 0, 2)).to(dev)
    out = torch.full((n, 2), 7.0, device=dev)
    runs = torch.full((16, 2), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    L0 = 100
    clips = torch.full((2, L0), 7.0, device=dev)
    gen = case["gen"][:2].contiguous().to(dev)
    ptr = native._ptr
    keep = []

    def sinc(f0, **kw):
        d = dict(nwin=f0["win"].numel(), num_table=f0["num_table"], step=f0["step"], scale=f0["scale"], win=f0["win"].data_ptr(), dwin=f0["dwin"].data_ptr())
        d.update(kw)
        return native.SincFilter(C.sizeof(native.SincFilter), d["nwin"], d["num_table"], d["step"], 0, 0, d["scale"], 0.0, d["win"], d["dwin"], None)

    def refused(name, rc_of, msg):
        ctx.profile_start(100)
        rc = rc_of()
        err = lib.si_last_error(h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        assert rc == -1 and launched == [] and err.startswith(name + ": ") and re.search(msg, err), (name, msg, rc, err, launched)      # SI_EINVAL

    # ---- si_quiet_runs_ch: tests/test_gpu_detect.py's cases, for one channel and for the joint mode
    good = dict(x=x, n=n, thr=0.0, min_len=1, runs=runs, max_runs=16, cnt=cnt)
    cases = [(dict(x=None), "x is NULL"), (dict(cnt=None), "n_runs is NULL"), (dict(runs=None), "runs is NULL with max_runs = 16"),
             (dict(n=0), "n = 0 samples"), (dict(n=-5), "n = -5 samples"), (dict(n=2 ** 31 - 1 - 2047), "n = 2147481600 samples"),
             (dict(n=2 ** 31 - 1), "n = 2147483647 samples"), (dict(thr=-1e-9), "threshold = -1e-09 is negative or NaN"),
             (dict(thr=float("nan")), "threshold = -?nan is negative or NaN"), (dict(min_len=0), "min_len = 0 samples"),
             (dict(min_len=-3), "min_len = -3 samples"), (dict(max_runs=-1), "max_runs = -1 is negative")]
    for channel in (1, -1):
        for change, msg in cases:
            a = {**good, **change}
            refused("si_quiet_runs_ch", lambda: lib.si_quiet_runs_ch(h, ptr(a["x"]), 0, a["n"], 2, channel, a["thr"], a["min_len"], ptr(a["runs"]), a["max_runs"],
                                                                     ptr(a["cnt"]), ctx._stream()), msg)

    # ---- si_cut_rate_ch: tests/test_gpu_feed.py's cases
    feed = eng._feed_filter(sr)

    def cut(starts=(0, 50), f=None, sr_=sr, n_=n, o=clips, x_=x, L=L0, Cn=None, host=True, devt=True):
        hs = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
        ds = torch.from_numpy(hs).to(dev)
        f = sinc(feed) if f is None else f
        keep.extend([hs, ds, f])
        return lambda: lib.si_cut_rate_ch(h, ptr(x_), 0, n_, 2, 1, sr_, hs.ctypes.data_as(C.c_void_p) if host else None, ptr(ds) if devt else None,
                                          len(hs) if Cn is None else Cn, L, C.byref(f) if f else None, ptr(o), ctx._stream())

    short = sinc(feed)
    short.struct_size -= 8
    cases = [(dict(x_=None), "x is NULL"), (dict(o=None), "out is NULL"), (dict(host=False), "host_start is NULL"), (dict(devt=False), "start is NULL"),
             (dict(f=False), "filt: si_sinc_filter size mismatch"), (dict(f=short), "filt: si_sinc_filter size mismatch"),
             (dict(sr_=3999), "sr = 3999 Hz, outside 4000 .. 192000"), (dict(sr_=192001), "sr = 192001 Hz, outside 4000 .. 192000"),
             (dict(sr_=22050), "sr = 22050"), (dict(n_=0), "n_file = 0"), (dict(n_=-1), "n_file = -1"),
             (dict(n_=2 ** 31 - 1 - 2047), "n_file = 2147481600 samples, at most"), (dict(sr_=8000, n_=2 ** 30), "at 22050 Hz"),
             (dict(f=sinc(feed, step=2)), "filt: bad filter table: .* taps per wing"),      # 16 385 taps per wing: no tile's samples fit
             (dict(Cn=-1), "C = -1"), (dict(Cn=65536), "C = 65536"), (dict(L=0), "L = 0"), (dict(L=-3), "L = -3"),
             (dict(starts=(0, -1)), r"start\[1\]"), (dict(starts=(N22 - L0 + 1, 0)), r"start\[0\]"), (dict(starts=(0, 2 ** 31 - 1)), r"start\[1\]")]
    cases += [(dict(f=sinc(feed, **bad)), "filt: bad filter table") for bad in
              (dict(nwin=1), dict(num_table=0), dict(step=0), dict(scale=0.0), dict(scale=1.5), dict(win=None), dict(dwin=None))]
    for change, msg in cases:
        refused("si_cut_rate_ch", cut(**change), msg)

    # ---- si_patch_rate_ch: tests/test_gpu_rate.py's cases
    rate = eng._rate_filter(sr)

    def table(spans_=spans, wins_=wins, chunks_=chunks, fade_=fade_f, n_ctx=2):
        t = native.RateTable(spans_, wins_, chunks_, n_ctx, max(fade_, 0), dev)
        keep.append(t)
        st = t.struct()
        st.fade = fade_
        return st

    def patch(st=None, f=None, sr_=sr, n_=n, o=out, x_=x, lrow_=lrow):
        st = table() if st is None else st
        f = sinc(rate) if f is None else f
        keep.extend([st, f])
        return lambda: lib.si_patch_rate_ch(h, ptr(x_), 0, n_, 2, 1, sr_, C.byref(st) if st else None, ptr(gen), lrow_, None, C.byref(f) if f else None,
                                            ptr(o), ctx._stream())

    def swap(rows, k, j, v):
        r = list(rows[k])
        r[j] = v
        return rows[:k] + [tuple(r)] + rows[k + 1:]

    small = table()
    small.struct_size -= 8
    cut_row = [(0, 0, wins[0][2] - 6, wins[0][2]), wins[1]]
    cases = [(dict(sr_=3999), "outside 4000 .. 192000"), (dict(sr_=192001), "outside 4000 .. 192000"), (dict(sr_=22050), "22050"),
             (dict(n_=2 ** 31 - 1 - 2047), "at most"), (dict(sr_=8000, n_=2 ** 30), "at 22050 Hz"),
             (dict(o=None), "NULL / empty"), (dict(x_=None), "NULL / empty"), (dict(n_=0), "NULL / empty"), (dict(o=x), "out is orig"),
             (dict(st=False), "si_rate_table size mismatch"), (dict(st=small), "si_rate_table size mismatch"), (dict(f=False), "si_sinc_filter size mismatch"),
             (dict(f=sinc(rate, step=2)), "bad filter table: .* taps per wing"),            # 16 385 taps per wing: no chunk's row fits
             (dict(st=table(fade_=-1)), "fade of -1 samples"),
             (dict(st=table([spans[1], spans[0]] + spans[2:])), "unsorted or overlapping"),
             (dict(st=table(swap(spans, 1, 1, 0))), "span 1 "), (dict(st=table(swap(spans, 0, 0, -5))), "span 0 "),
             (dict(st=table(swap(spans, 4, 3, n + 1))), "lim"), (dict(st=table(swap(spans, 1, 3, spans[1][0]))), "lim"),
             (dict(st=table(swap(spans, 0, 2, 2))), "names window 2 of 2"), (dict(st=table(swap(spans, 0, 2, -1))), "names window -1"),
             (dict(st=table(wins_=swap(wins, 1, 0, 2))), "window 1 names context 2"), (dict(st=table(n_ctx=0)), "names context 0 of 0"),
             (dict(lrow_=wins[0][2] - 1), "outside the recording"), (dict(st=table(wins_=swap(wins, 0, 1, -1))), "outside the recording"),
             (dict(st=table(wins_=swap(wins, 1, 3, wins[1][1]))), "its context's audio ends"),                  # win_lim <= win_start
             (dict(st=table(wins_=swap(wins, 1, 3, 10 ** 6))), "its context's audio ends"),                     # win_lim past the recording
             (dict(st=table(chunks_=[chunks[1], chunks[0]] + chunks[2:])), "not strictly increasing"),
             (dict(st=table(chunks_=chunks + [(4, 5, 5)])), "at or past"), (dict(st=table(chunks_=swap(chunks, 0, 2, 6))), "walks spans"),
             (dict(st=table(chunks_=chunks[:3])), "lacks chunk 3"), (dict(st=table(chunks_=[])), "lacks chunk"),
             (dict(st=table(chunks_=swap(chunks, 0, 2, chunks[0][1]))), "omits span"),
             (dict(st=table(swap(spans, 4, 3, spans[4][3] + 2))), "span 4 writes up to"),                       # lim_f past its context's end
             (dict(st=table(wins_=swap(wins, 1, 1, wins[1][1] + 4))), "span 3 blends"),                         # the row starts 1 tap late
             (dict(st=table(wins_=cut_row)), "span 2 blends"),                                                  # the row ends 1 tap early
             (dict(st=table(swap(spans, 2, 2, 1))), "its window's row holds")]                                  # C in window 1, which starts behind it
    cases += [(dict(f=sinc(rate, **bad)), "bad filter table") for bad in
              (dict(nwin=1), dict(num_table=0), dict(step=0), dict(scale=0.0), dict(scale=1.5), dict(win=None), dict(dwin=None))]
    for change, msg in cases:
        refused("si_patch_rate_ch", patch(**change), msg)
    # NULL arrays behind non-zero counts: the struct of a good table with one pointer taken out
    for field, msg in (("ramp", "NULL ramp"), ("win_len", "NULL window arrays"), ("host_span_lim", "NULL span arrays"), ("k1", "NULL chunk arrays")):
        st = table()
        setattr(st, field, None)
        refused("si_patch_rate_ch", patch(st=st), msg)
    st = table()
    st.num_spans = -1
    refused("si_patch_rate_ch", patch(st=st), "rate table with 2 contexts / 2 windows / -1 spans / 4 chunks")
    refused("si_patch_rate_ch", lambda: lib.si_patch_rate_ch(h, ptr(x), 0, n, 2, 1, sr, C.byref(table()), None, lrow, None, C.byref(sinc(rate)), ptr(out),
                                                             ctx._stream()), "NULL window arrays / generator rows")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((clips == 7.0).all()) and bool((runs == SENTINEL).all()) and int(cnt.item()) == SENTINEL
    # counts of zero launch nothing and succeed, as the mono calls do
    ctx.profile_start(100)
    assert cut(starts=(), x_=None, o=None, host=False, devt=False)() == 0
    ctx.patch_rate(x, sr, native.RateTable([], [], [], 0, 0, dev), None, rate, out, None, channel=1)
    assert [e for e in ctx.profile_stop() if e["launches"] > 0] == []
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
