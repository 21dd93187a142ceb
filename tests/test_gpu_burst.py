"""Corrupted blocks by second-difference level on the device: si_burst_runs against the exact reference of
tests/burst_ref.py -- the total, every (start, len) row and the untouched rows past them, exact integer equality; the effective
threshold bit for bit -- for fp32, int16 and packed 24-bit.  There is no tolerance: every case's builder has asserted that none of its
samples depends on the order in which the squares are added.
Every input lies inside a longer device buffer with sample times planted in front of the base and behind the input, zeros in some
cases and full-scale alternation -- the loudest second difference there is -- in others: neither may be read."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import burst_ref as B
from tests import dead_ref as R
from tests import s24_ref as S
from tests.cases import _patch_engine as _engine

pytestmark = pytest.mark.gpu

TORCH = {np.float32: torch.float32, np.int16: torch.int16}
SENTINEL = -7
DTYPES = list(B.DTYPES)
IDS = ["fp32", "int16", "s24"]
OFFSETS = {np.float32: (4, 8, 12), np.int16: (2, 6, 14), B.S24: (1, 3, 5, 8, 10)}        # bytes past a 16-byte boundary
_SIZE = {}


def _size_cases(n, h, dtype):
    if (n, h, dtype) not in _SIZE:
        _SIZE[n, h, dtype] = B.size_cases(n, h, dtype)
    return _SIZE[n, h, dtype]


def _place(dev, case, off=0):
    """case.x on the device as a view whose first byte lies `off` bytes past a 16-byte boundary, its traps in front of it and behind
    it.  24-bit values go packed: uint8 (n, [ch,] 3)."""
    flat, start = case.memory()
    s24 = flat.dtype.type is B.S24
    raw = S.pack(flat).reshape(-1) if s24 else flat.view(np.uint8)
    item = 3 if s24 else flat.itemsize
    assert s24 or off % item == 0
    first = start * item                                                # x's first byte in raw
    lead = 16 + (off - first) % 16
    buf = torch.zeros(lead + raw.size + 32, dtype=torch.uint8, device=dev)
    buf[lead:lead + raw.size] = torch.from_numpy(raw.copy())
    view = buf[lead + first:lead + first + case.x.size * item]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == off
    return view.view(*case.x.shape, 3) if s24 else view.view(TORCH[flat.dtype.type]).view(case.x.shape)


def _call(ctx, case, off=0, max_runs=4096, x=None):
    """-> (total, the rows written, the rows past them, T) of one si_burst_runs call."""
    x = _place(ctx.device, case, off) if x is None else x
    runs = torch.full((max_runs + 8, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
    T = torch.full((1,), -1.0, dtype=torch.float32, device=ctx.device)
    _, n_runs = ctx.burst_runs(x, case.half, case.thr, case.rel, case.min_len, max_runs, runs=runs, channel=case.channel, threshold_out=T)
    total = int(n_runs.item())
    rows = runs.cpu().numpy()
    k = min(total, max_runs)
    return total, rows[:k], rows[k:], T.cpu().numpy()[0]


def _check(ctx, case, **kw):
    want = case.rows()
    total, rows, rest, T = _call(ctx, case, **kw)
    what = (case.name, case.x.shape, str(case.x.dtype), kw)
    assert total == len(want), (what, total, len(want), rows[:6].tolist(), want[:6].tolist())
    assert len(rows) == min(total, kw.get("max_runs", 4096)) and np.array_equal(rows, want[:len(rows)]), (what, rows[:8].tolist(), want[:8].tolist())
    assert np.all(rest == SENTINEL), what
    assert T.tobytes() == case.threshold().tobytes(), (what, T, case.threshold())
    return want


def _same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("h", B.HALVES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_size_at_every_half_window(dtype, h):
    """The thinned product of n in {1, 2, 3, 4, 2 h + 1, 2 h + 2, 2 h + 3, 2047, 2048, 2049, 2050, 4101, 6144} and the nine half windows:
    garbage blocks on, off and across every chunk seam, at sample 1 and ending at n - 2, at both file ends with truncated windows; at
    h = 1024 the halo is a whole chunk on each side.  n < 3 gives zero runs."""
    ctx = _engine().ctx
    found = 0
    for n in [n for n, g in B.sweep() if g == h]:
        for case in _size_cases(n, h, dtype):
            want = _check(ctx, case)
            assert n >= 3 or len(want) == 0
            found += len(want)
    assert found > 0


@pytest.mark.parametrize("h", B.HALVES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_value_edges(dtype, h):
    """E == lim exactly and one step over T; the full-scale alternation, whose d = 131 070 (2^25 - 2 for 24-bit) must not wrap, and T =
    4 * peak from rel_threshold = 4; blocks at both file ends with truncated counts; NaN and +-inf at, beside and one past a window's edge
    under the three-neighbour rule; hot windows 2 h, 2 h + 1 and 2 h + 2 apart; a D that fp32 cannot form."""
    ctx = _engine().ctx
    for case in B.value_cases(h, dtype):
        _check(ctx, case)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_half_zero_is_the_sample_wise_second_difference(dtype):
    """half = 0: hot(i) <=> |d(i)| >= T for 1 <= i <= n - 2, computed here without the reference's windows."""
    ctx = _engine().ctx
    for n in (3, 9, 2049, 4101):
        for case in _size_cases(n, 0, dtype):
            v = case.x.astype(np.float64)
            d = np.abs(v[:-2] - 2 * v[1:-1] + v[2:])                    # exact: the builders' values are short integers times a power of two
            mask = np.concatenate([[False], d >= float(np.float32(case.thr)), [False]])
            assert np.array_equal(R.runs_of(mask, case.min_len), case.rows()), case.name
            _check(ctx, case)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_base_pointer_off_the_grids(dtype):
    """Bases off the 4-, 8- and 16-byte grids; packed 24-bit at odd bytes too."""
    ctx = _engine().ctx
    for n, h in ((9, 1), (2049, 7), (4101, 48), (4101, 512)):
        for case in _size_cases(n, h, dtype):
            for off in OFFSETS[dtype]:
                _check(ctx, case, off=off)
    for case in B.value_cases(8, dtype)[::3]:
        for off in OFFSETS[dtype]:
            _check(ctx, case, off=off)


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("ch", [2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_interleaved_files(dtype, ch):
    """One channel of (n, ch) and the joint mode: channel c's neighbours are elements (k +- 1) ch + c -- its own block lies where its
    neighbours are clean, and a stretch alternates ACROSS the channels while each is constant --, each channel's peak is its own and
    the joint one is the file's.  channel = c gives the bytes of the mono call on the de-interleaved copy."""
    ctx = _engine().ctx
    for h in (7, 48):
        for case in B.channel_cases(ch, dtype, h):
            for off in (0, OFFSETS[dtype][0]):
                _check(ctx, case, off=off)
            if case.channel >= 0:
                col = np.ascontiguousarray(case.x[:, case.channel])
                mono = B.Case("mono", col, case.half, case.thr, case.rel, case.min_len, None)
                assert _same(_call(ctx, case), _call(ctx, mono)), case.name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_channel_as_an_interleaved_file(dtype):
    """channels = 1 (channel 0 or -1) gives the mono call's bytes."""
    ctx = _engine().ctx
    for case in _size_cases(4101, 48, dtype) + B.value_cases(7, dtype)[:4]:
        want = _call(ctx, case)
        for channel in (0, -1):
            one = B.Case(case.name, case.x.reshape(-1, 1), case.half, case.thr, case.rel, case.min_len, channel, case.before, case.after)
            assert _same(_call(ctx, one), want), (case.name, channel)
            _check(ctx, one)


# ------------------------------------------------------------------------------------------------------------ 3
def test_past_the_tile_seam_of_the_carry():
    """An int16 file of 1027 chunks: a garbage block spans chunks 1023 | 1024 with whole dead chunks on both sides of the carry tile's
    seam, the peak lies in the last chunk, full-scale values lie outside the input."""
    ctx = _engine().ctx
    assert len(_check(ctx, B.long_case())) == 2


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_max_runs_and_repeated_calls(dtype):
    """max_runs from 0 to one past the total; a repeated call; a call after one with a larger n and another h: the bytes of a fresh
    context, whatever the scratch and the LDS request held before."""
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from tests.harness import build_engine
    ctx = _engine().ctx
    case = max(_size_cases(4101, 7, dtype), key=lambda c: len(c.rows()))
    want = _check(ctx, case)
    assert len(want) >= 3
    for cap in (0, 1, len(want) - 1, len(want), len(want) + 1):
        total, rows, rest, T = _call(ctx, case, max_runs=cap)
        assert total == len(want) and np.array_equal(rows, want[:cap]) and np.all(rest == SENTINEL), cap
        assert T.tobytes() == case.threshold().tobytes()
    assert _same(_call(ctx, case), _call(ctx, case))
    big = _size_cases(6144, 1024, dtype)[4]
    small = _size_cases(2049, 48, dtype)[4]
    _check(ctx, big)
    after = _call(ctx, small)
    fresh = build_engine(HubertArch.tiny(), VocoderArch.tiny(), 100).ctx
    assert _same(after, _call(fresh, small)) and len(after[1]) > 0
    _check(fresh, big)


@pytest.mark.parametrize("ch", [0, 3], ids=["mono", "3ch"])
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["fp32", "int16"])
def test_detector_scratch_after_a_long_hot_recording(dtype, ch):
    """ctx->det_scratch by history: first a long recording that is hot from end to end (an alternation at half of full
    scale, |d| = 2 full scales, against T = the peak from rel_threshold = 1) at the largest half window -- three carry tiles, a bitmap of
    all ones, the 139 264-byte LDS request --, under poisoned allocations.  Then short recordings at other half windows on the SAME
    context: each result equals the same call on a fresh context, bit for bit.  The kernel is profiled in the detect_dead family
    (tests/poison.py's lists are closed), whose own account in tests/test_gpu_scratch.py does not reach it: this test does."""
    from tests import poison as P
    from tests import test_gpu_scratch as G
    from tests.harness import tapped_run
    assert "detect_dead" in P.SCRATCH_FAMILIES
    used = G._fresh_ctx()

    def burst(ctx, x, c, h, thr, rel, min_len, max_runs=64):
        T = torch.empty(1, dtype=torch.float32, device=ctx.device)
        runs, n = ctx.burst_runs(x, h, thr, rel, min_len, max_runs, channel=c, threshold_out=T)
        return [runs, n, T]

    try:
        n_long = 2 * 1024 * 2048 + 4101
        A = 0.5 if dtype is np.float32 else 16384
        long = torch.full((n_long, ch) if ch else (n_long,), A, dtype=TORCH[dtype])
        long[1::2] = -A
        long = long.cuda()
        chan = -1 if ch else None
        with P.poisoned_allocs():
            (_, (runs, cnt, T), prof) = tapped_run(used, {}, lambda: burst(used, long, chan, 1024, 0.0, 1.0, 1, 4), profile=True)
            assert {"detect_peak", "detect_peak_final", "detect_dead", "detect_carry", "detect_count", "detect_offsets", "detect_emit"} == set(prof)
            assert int(cnt[0]) == 1 and runs[0].tolist() == [0, n_long] and float(T[0]) == float(A)
            for n, h in ((3, 0), (9, 1), (2047, 7), (2049, 48), (4101, 511), (6144, 22)):
                cols = [_size_cases(n, h, dtype)[4 + k % 3].x for k in range(max(ch, 1))]
                x = torch.from_numpy(R.interleave(cols) if ch else cols[0]).cuda()
                for c in ([0, ch - 1, -1] if ch else [None]):
                    for rel in (0.0, 1.2):
                        call = lambda ctx: burst(ctx, x, c, h, B.THR[dtype], rel, 2)
                        got = [t.cpu() for t in call(used)]
                        G._same(G._written(got), G._written(G._on_fresh(call)), (dtype, ch, n, h, c, rel))
                        assert 0 <= int(got[1][0]) <= n
    finally:
        used.close()


def test_find_burst_runs():
    eng = _engine()
    x = np.float32([0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0])                                  # d = 4, -8, 4 at 4, 5, 6
    assert eng.find_burst_runs(x, half=0, threshold=4.0).tolist() == [[4, 3]] and eng.find_burst_runs(x, half=0, threshold=5.0).tolist() == [[5, 1]]
    assert eng.find_burst_runs(x, win=3, threshold=5.0).tolist() == [[3, 5]]              # W(4), W(5), W(6): 80, 96, 80 >= 75; W(3), W(7): 16; dilated by 1
    runs, T = eng.find_burst_runs(x, half=1, threshold=0.0, rel_threshold=1.25, min_len=2, return_threshold=True)
    assert runs.dtype == torch.int32 and runs.is_cuda and T == 5.0 and runs.tolist() == B.burst_runs_ref(x, 1, 5.0, min_len=2).tolist()
    assert eng.find_burst_runs(x, half=1, threshold=5.0).tolist() == B.burst_runs_ref(x, 1, 5.0).tolist()
    two = np.stack([x, x[::-1]], axis=1)
    assert eng.find_burst_runs(two, half=0, threshold=4.0, channel=1).tolist() == [[5, 3]]
    assert eng.find_burst_runs(two, half=0, threshold=4.0, channel=-1).tolist() == [[5, 2]]
    assert eng.find_burst_runs(np.int16(x * 2).reshape(-1, 1), half=0, threshold=8.0, channel=0).tolist() == [[4, 3]]
    assert eng.find_burst_runs(S.pack(np.int32(x * 1000)), half=0, threshold=4000.0).tolist() == [[4, 3]]
    assert eng.find_burst_runs(np.float32([1, -1]), half=0, threshold=0.0).shape == (0, 2)         # n < 3
    with pytest.raises(ValueError, match=r"3 runs .* more than max_runs = 1"):
        eng.find_burst_runs(np.float32([0, 4, 0, 0, 0, 0, 4, 0, 0, 0, 0, 4, 0]), half=0, threshold=8.0, max_runs=1)
    with pytest.raises(ValueError, match="needs channel"):
        eng.find_burst_runs(two, half=1)
    with pytest.raises(ValueError, match="channel = 1 of a one-channel recording"):
        eng.find_burst_runs(x, half=1, channel=1)
    with pytest.raises(ValueError, match=r"rel_threshold = 4.5 is NaN or outside \[0, 4\]"):
        eng.find_burst_runs(x, half=1, rel_threshold=4.5)


# ------------------------------------------------------------------------------------------------------------ 4
def test_refusals_come_before_any_launch():
    ctx = _engine().ctx
    lib, h, dev = ctx.lib, ctx._h, ctx.device
    x = torch.zeros(4096 * 2, device=dev)
    x[0::4] = 1.0                                                       # channel 0 of (4096, 2): 1, 0, 1, 0 ...: |d| = 2 at every centre
    runs = torch.full((16, 2), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    T = torch.full((1,), -1.0, dtype=torch.float32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(x=x, pcm=0, n=4096, channels=2, channel=0, half=48, thr=0.0, rel=0.5, min_len=1, runs=runs, max_runs=16, cnt=cnt)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(x=None), "x is NULL"), (dict(cnt=None), "n_runs is NULL"), (dict(runs=None), "runs is NULL with max_runs = 16"),
             (dict(n=0), "n = 0 samples"), (dict(n=2 ** 31 - 1 - 2047), "n = 2147481600 samples"), (dict(thr=-1e-9), "threshold = -1e-09 is negative or NaN"),
             (dict(thr=nan), "threshold = -?nan is negative or NaN"), (dict(min_len=0), "min_len = 0 samples"), (dict(max_runs=-1), "max_runs = -1 is negative"),
             (dict(channels=0), "channels = 0, outside 1 .. SI_MAX_CHANNELS = 8"), (dict(channels=9), "channels = 9, outside"),
             (dict(channel=2), "channel = 2, outside -1 .. 1"), (dict(channel=-2), "channel = -2, outside -1 .. 1"),
             (dict(channels=1, channel=1), "channel = 1, outside -1 .. 0"),
             (dict(half=-1), "half = -1 samples, outside 0 .. SI_LEVEL_MAX_HALF = 1024"), (dict(half=1025), "half = 1025 samples, outside 0 .. SI_LEVEL_MAX_HALF = 1024"),
             (dict(thr=inf), "threshold = inf is not finite"),
             (dict(rel=nan), r"rel_threshold = -?nan is NaN or outside \[0, 4\]"), (dict(rel=-0.1), r"rel_threshold = -0.1 is NaN or outside \[0, 4\]"),
             (dict(rel=4.5), r"rel_threshold = 4.5 is NaN or outside \[0, 4\]")]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda a: lib.si_burst_runs(h, P(a["x"]), a["pcm"], a["n"], a["channels"], a["channel"], a["half"], a["thr"], a["rel"], a["min_len"],
                                       P(a["runs"]), a["max_runs"], P(a["cnt"]), P(T), stream)
    for change, msg in cases:
        ctx.profile_start(100)
        rc = call({**good, **change})
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        err = lib.si_last_error(h).decode()
        assert rc == -1 and launched == [], (change, rc, launched)                               # SI_EINVAL
        assert re.search("si_burst_runs: " + msg, err), (change, err)
    torch.cuda.synchronize()
    assert bool((runs == SENTINEL).all()) and int(cnt.item()) == SENTINEL and float(T.item()) == -1.0
    # the same arguments unchanged are served: pass 0 only with rel > 0, a NULL threshold_out is fine, both ends of half and of rel are legal
    names = {"detect_dead": 1, "detect_carry": 1, "detect_count": 1, "detect_offsets": 1, "detect_emit": 1}
    peak = {**names, "detect_peak": 1, "detect_peak_final": 1}
    for change, want in ((dict(), peak), (dict(rel=0.0, thr=2.0), names), (dict(half=0, rel=2.0), peak), (dict(half=1024), peak),
                         (dict(max_runs=0, runs=None), {k: v for k, v in peak.items() if k != "detect_emit"})):
        ctx.profile_start(100)
        rc = call({**good, **change})
        prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
        assert rc == 0 and prof == want, (change, prof)
        first = [1, 4094] if change.get("half") == 0 else [0, 4096]     # without a dilation samples 0 and n - 1 stay out
        assert int(cnt.item()) == 1 and runs[0].tolist() == first, (change, runs[0].tolist())
    assert float(T.item()) == 0.5
    assert call({**good, "rel": 4.0}) == 0 and int(cnt.item()) == 0 and float(T.item()) == 4.0    # |d| = 2 < 4: nothing is hot
    assert lib.si_burst_runs(h, P(x), 0, 4096, 2, 0, 48, 2.0, 0.0, 1, P(runs), 16, P(cnt), C.c_void_p(0), stream) == 0
    # the other routes launch what they launched
    ctx.profile_start(100)
    ctx.quiet_runs(x[:4096], 0.0, 1, 16, runs=runs)
    ctx.quiet_runs(x.view(4096, 2), 0.0, 1, 16, runs=runs, channel=0)
    ctx.dead_runs(x[:4096], 3, 0.0, 0.5, 0.0, 1, 16, runs=runs)
    ctx.dead_runs(x.view(4096, 2), 3, 0.0, 0.0, 0.0, 1, 16, runs=runs, channel=-1)
    ctx.level_runs(x[:4096], 48, 0.0, 0.5, 1, 16, runs=runs)
    ctx.level_runs(x.view(4096, 2), 7, 0.0, 0.0, 1, 16, runs=runs, channel=1)
    prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
    assert prof == {"detect_bits": 1, "detect_bits_ch": 1, "detect_dead": 4, "detect_peak": 2, "detect_peak_final": 2, "detect_carry": 6,
                    "detect_count": 6, "detect_offsets": 6, "detect_emit": 6}, prof
