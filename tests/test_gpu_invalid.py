"""NaN, inf and out-of-range samples on the device: si_invalid_runs against the exact reference of
tests/invalid_ref.py -- the total, every (start, len) row and the untouched rows past them, exact integer equality -- for fp32, int16
and packed 24-bit.  Every input lies inside a longer device buffer with NaN (fp32) or full scale (PCM) planted in front of the base
and behind the input: neither may be judged."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import dead_ref as R
from tests import invalid_ref as V
from tests import s24_ref as S
from tests.cases import _patch_engine as _engine

pytestmark = pytest.mark.gpu

TORCH = {np.float32: torch.float32, np.int16: torch.int16}
SENTINEL = -7
DTYPES = list(V.DTYPES)
IDS = ["fp32", "int16", "s24"]
OFFSETS = {np.float32: (4, 8, 12), np.int16: (2, 6, 14), V.S24: (1, 3, 5, 8, 10)}        # bytes past a 16-byte boundary
_SIZE = {}


def _size_cases(n, dtype):
    if (n, dtype) not in _SIZE:
        _SIZE[n, dtype] = V.size_cases(n, dtype)
    return _SIZE[n, dtype]


def _place(dev, case, off=0):
    """case.x on the device as a view whose first byte lies `off` bytes past a 16-byte boundary, its traps in front of it and behind
    it.  24-bit values go packed: uint8 (n, [ch,] 3)."""
    flat, start = case.memory()
    s24 = flat.dtype.type is V.S24
    raw = S.pack(flat).reshape(-1) if s24 else flat.view(np.uint8)
    item = 3 if s24 else flat.itemsize
    assert s24 or off % item == 0
    first = start * item
    lead = 16 + (off - first) % 16
    buf = torch.zeros(lead + raw.size + 32, dtype=torch.uint8, device=dev)
    buf[lead:lead + raw.size] = torch.from_numpy(raw.copy())
    view = buf[lead + first:lead + first + case.x.size * item]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == off
    return view.view(*case.x.shape, 3) if s24 else view.view(TORCH[flat.dtype.type]).view(case.x.shape)


def _call(ctx, case, off=0, max_runs=4096, x=None):
    """-> (total, the rows written, the rows past them) of one si_invalid_runs call."""
    x = _place(ctx.device, case, off) if x is None else x
    runs = torch.full((max_runs + 8, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
    _, n_runs = ctx.invalid_runs(x, case.ceiling, case.min_len, max_runs, runs=runs, channel=case.channel)
    total = int(n_runs.item())
    rows = runs.cpu().numpy()
    k = min(total, max_runs)
    return total, rows[:k], rows[k:]


def _check(ctx, case, **kw):
    want = case.rows()
    total, rows, rest = _call(ctx, case, **kw)
    what = (case.name, case.x.shape, str(case.x.dtype), kw)
    assert total == len(want), (what, total, len(want), rows[:6].tolist(), want[:6].tolist())
    assert len(rows) == min(total, kw.get("max_runs", 4096)) and np.array_equal(rows, want[:len(rows)]), (what, rows[:8].tolist(), want[:8].tolist())
    assert np.all(rest == SENTINEL), what
    return want


def _same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_size_and_seam(dtype):
    """n in {1, 2, 7, 8, 9, 2047, 2048, 2049, 4101}: invalid samples at 0 and n - 1, on both sides of thread seams (8) and chunk seams
    (2048), runs across the chunk seams, nothing invalid, everything invalid; c in {inf, 1.0, FLT_MAX} for fp32, {32766, 32767} for
    int16, 2^23 - 2 for 24-bit; NaN / full scale in front of the base and past n."""
    ctx = _engine().ctx
    found = 0
    for n in V.SIZES:
        for case in _size_cases(n, dtype):
            found += len(_check(ctx, case))
    assert found > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_value_of_the_table(dtype):
    """The hand-checked values -- four NaN patterns, +-inf, +-FLT_MAX, one step on either side of a finite ceiling, |v| == c, -0.0, a
    subnormal; -32768 and -2^23 against both ceilings around them -- at every ceiling of the table."""
    ctx = _engine().ctx
    for case in V.table_cases(dtype):
        _check(ctx, case)
        for off in OFFSETS[dtype][:2]:
            _check(ctx, case, off=off)
    for name, d, v, c, want in V.value_table():                        # and one by one: a file of one sample
        if d is dtype:
            case = V.Case(name, np.asarray(v).astype(d) if d is not np.float32 else np.asarray(v), c, 1, None, V.trap(3, d), V.trap(3, d))
            total, rows, _ = _call(ctx, case)
            assert (total, rows.tolist()) == ((1, [[0, 1]]) if want else (0, [])), name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_base_pointer_off_the_grids(dtype):
    """Bases off the 4-, 8- and 16-byte grids; packed 24-bit at odd bytes too: both routes of dt_load_eight."""
    ctx = _engine().ctx
    for n in (9, 2049, 4101):
        for case in _size_cases(n, dtype):
            for off in OFFSETS[dtype]:
                _check(ctx, case, off=off)


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("ch", [2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_interleaved_files(dtype, ch):
    """One channel of (n, ch) and the joint mode, with an invalid element in ONE channel only: channel = c gives the bytes of the mono
    call on the de-interleaved copy; joint is dead only where every channel is."""
    ctx = _engine().ctx
    for case in V.channel_cases(ch, dtype):
        for off in (0, OFFSETS[dtype][0]):
            _check(ctx, case, off=off)
        if case.channel >= 0:
            mono = V.Case("mono", np.ascontiguousarray(case.x[:, case.channel]), case.ceiling, case.min_len, None)
            assert _same(_call(ctx, case), _call(ctx, mono)), case.name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_channel_as_an_interleaved_file(dtype):
    """channels = 1 (channel 0 or -1) gives the mono call's bytes."""
    ctx = _engine().ctx
    for case in _size_cases(4101, dtype)[:3]:
        want = _call(ctx, case)
        for channel in (0, -1):
            one = V.Case(case.name, case.x.reshape(-1, 1), case.ceiling, case.min_len, channel, case.before, case.after)
            assert _same(_call(ctx, one), want), (case.name, channel)
            _check(ctx, one)


# ------------------------------------------------------------------------------------------------------------ 3
def test_past_the_tile_seam_of_the_carry():
    """An fp32 file of 1027 chunks: an inf run spans chunks 1023 | 1024 with whole dead chunks on both sides of the carry tile's seam."""
    ctx = _engine().ctx
    assert len(_check(ctx, V.long_case())) == 2


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_min_len_max_runs_and_repeated_calls(dtype):
    """min_len from 1 up, max_runs from 0 to one past the total; a repeated call; a call after one with a larger n: the bytes of a
    fresh context."""
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from tests.harness import build_engine
    ctx = _engine().ctx
    case = _size_cases(4101, dtype)[0]
    want = _check(ctx, case)
    assert len(want) >= 8
    for min_len in (1, 2, 3, 8, 9):
        c = V.Case(case.name, case.x, case.ceiling, min_len, None, case.before, case.after)
        assert np.array_equal(c.rows(), R.runs_of(case.mask(), min_len))
        _check(ctx, c)
    for cap in (0, 1, len(want) - 1, len(want), len(want) + 1):
        total, rows, rest = _call(ctx, case, max_runs=cap)
        assert total == len(want) and np.array_equal(rows, want[:cap]) and np.all(rest == SENTINEL), cap
    assert _same(_call(ctx, case), _call(ctx, case))
    big, small = _size_cases(4101, dtype)[2], _size_cases(2049, dtype)[0]              # all invalid, then the seams
    _check(ctx, big)
    after = _call(ctx, small)
    fresh = build_engine(HubertArch.tiny(), VocoderArch.tiny(), 100).ctx
    assert _same(after, _call(fresh, small)) and len(after[1]) > 0


@pytest.mark.parametrize("ch", [0, 3], ids=["mono", "3ch"])
def test_detector_scratch_after_a_long_all_invalid_recording(ch):
    """ctx->det_scratch by history: first a long recording that is NaN from end to end -- three carry tiles, a bitmap
    of all ones --, under poisoned allocations; then short recordings on the SAME context: each result equals the same call on a fresh
    context, bit for bit.  The kernels are profiled as detect_bits / detect_bits_ch (tests/poison.py's lists are closed)."""
    from tests import poison as P
    from tests import test_gpu_scratch as G
    from tests.harness import tapped_run
    assert "detect_bits" in P.SCRATCH_FAMILIES and "detect_bits_ch" in P.SCRATCH_FAMILIES
    used = G._fresh_ctx()

    def invalid(ctx, x, c, ceiling, min_len, max_runs=64):
        runs, n = ctx.invalid_runs(x, ceiling, min_len, max_runs, channel=c)
        return [runs, n]

    try:
        n_long = 2 * 1024 * 2048 + 4101
        long = torch.full((n_long, ch) if ch else (n_long,), float("nan"), dtype=torch.float32).cuda()
        chan = -1 if ch else None
        with P.poisoned_allocs():
            (_, (runs, cnt), prof) = tapped_run(used, {}, lambda: invalid(used, long, chan, float("inf"), 1, 4), profile=True)
            assert {"detect_bits_ch" if ch else "detect_bits", "detect_carry", "detect_count", "detect_offsets", "detect_emit"} == set(prof)
            assert int(cnt[0]) == 1 and runs[0].tolist() == [0, n_long]
            for n in (1, 9, 2047, 2049, 4101):
                cols = [_size_cases(n, np.float32)[3 * (k % 3)].x for k in range(max(ch, 1))]
                x = torch.from_numpy(R.interleave(cols) if ch else cols[0]).cuda()
                for c in ([0, ch - 1, -1] if ch else [None]):
                    for ceiling in (float("inf"), 1.0):
                        call = lambda ctx: invalid(ctx, x, c, ceiling, 2)
                        got = [t.cpu() for t in call(used)]
                        G._same(G._written(got), G._written(G._on_fresh(call)), (ch, n, c, ceiling))
                        assert 0 <= int(got[1][0]) <= n
    finally:
        used.close()


def test_find_invalid_runs():
    eng = _engine()
    nan, inf = float("nan"), float("inf")
    x = np.float32([0, nan, 0, 0, inf, -inf, 3e38, 0, -0.0, 2.0, 0, nan])
    assert eng.find_invalid_runs(x).tolist() == [[1, 1], [4, 2], [11, 1]]
    assert eng.find_invalid_runs(x, ceiling=2.0).tolist() == [[1, 1], [4, 3], [11, 1]] and eng.find_invalid_runs(x, ceiling=1.0).tolist() == [[1, 1], [4, 3], [9, 1], [11, 1]]
    runs = eng.find_invalid_runs(x, min_len=2)
    assert runs.dtype == torch.int32 and runs.is_cuda and runs.tolist() == [[4, 2]]
    two = np.stack([x, x[::-1]], axis=1)
    assert eng.find_invalid_runs(two, channel=1).tolist() == V.invalid_runs_ref(two, channel=1).tolist() == [[0, 1], [6, 2], [10, 1]]   # 3e38 is finite
    assert eng.find_invalid_runs(two, channel=-1).shape == (0, 2)                                       # no time is non-finite in both
    assert eng.find_invalid_runs(two, ceiling=1.0, channel=-1).tolist() == V.invalid_runs_ref(two, 1.0, channel=-1).tolist() == [[5, 2]]
    assert eng.find_invalid_runs(np.int16([0, 32767, -32768, 5]).reshape(-1, 1), ceiling=32766.0, channel=0).tolist() == [[1, 2]]
    assert eng.find_invalid_runs(np.int16([0, 32767, -32768, 5])).shape == (0, 2)                   # PCM: nothing without a finite ceiling
    assert eng.find_invalid_runs(S.pack(np.int32([1, V.LO24, V.HI24, 7])), ceiling=float(V.HI24 - 1)).tolist() == [[1, 2]]
    with pytest.raises(ValueError, match=r"3 runs .* more than max_runs = 1"):
        eng.find_invalid_runs(x, max_runs=1)
    with pytest.raises(ValueError, match="needs channel"):
        eng.find_invalid_runs(two)
    with pytest.raises(ValueError, match="channel = 1 of a one-channel recording"):
        eng.find_invalid_runs(x, channel=1)


# ------------------------------------------------------------------------------------------------------------ 4
def test_refusals_come_before_any_launch():
    ctx = _engine().ctx
    lib, h, dev = ctx.lib, ctx._h, ctx.device
    x = torch.zeros(4096 * 2, device=dev)
    x[0::2] = float("nan")                                              # channel 0 of (4096, 2) is NaN throughout
    runs = torch.full((16, 2), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(x=x, pcm=0, n=4096, channels=2, channel=0, ceiling=float("inf"), min_len=1, runs=runs, max_runs=16, cnt=cnt)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(x=None), "x is NULL"), (dict(cnt=None), "n_runs is NULL"), (dict(runs=None), "runs is NULL with max_runs = 16"),
             (dict(n=0), "n = 0 samples"), (dict(n=2 ** 31 - 1 - 2047), "n = 2147481600 samples"), (dict(min_len=0), "min_len = 0 samples"),
             (dict(max_runs=-1), "max_runs = -1 is negative"), (dict(channels=0), "channels = 0, outside 1 .. SI_MAX_CHANNELS = 8"),
             (dict(channels=9), "channels = 9, outside"), (dict(channel=2), "channel = 2, outside -1 .. 1"), (dict(channel=-2), "channel = -2, outside -1 .. 1"),
             (dict(channels=1, channel=1), "channel = 1, outside -1 .. 0"),
             (dict(ceiling=0.0), "ceiling = 0 is not above 0, or is NaN"), (dict(ceiling=-1.0), "ceiling = -1 is not above 0, or is NaN"),
             (dict(ceiling=-inf), "ceiling = -inf is not above 0, or is NaN"), (dict(ceiling=nan), "ceiling = -?nan is not above 0, or is NaN")]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda a: lib.si_invalid_runs(h, P(a["x"]), a["pcm"], a["n"], a["channels"], a["channel"], a["ceiling"], a["min_len"], P(a["runs"]),
                                         a["max_runs"], P(a["cnt"]), stream)
    for change, msg in cases:
        ctx.profile_start(100)
        rc = call({**good, **change})
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        err = lib.si_last_error(h).decode()
        assert rc == -1 and launched == [], (change, rc, launched)                               # SI_EINVAL
        assert re.search("si_invalid_runs: " + msg, err), (change, err)
    torch.cuda.synchronize()
    assert bool((runs == SENTINEL).all()) and int(cnt.item()) == SENTINEL
    # the same arguments unchanged are served: never a pass 0; the smallest and the largest ceilings are legal
    names = {"detect_bits_ch": 1, "detect_carry": 1, "detect_count": 1, "detect_offsets": 1, "detect_emit": 1}
    for change, want in ((dict(), names), (dict(ceiling=1e-45), names), (dict(ceiling=3.4028234663852886e38), names),
                         (dict(max_runs=0, runs=None), {k: v for k, v in names.items() if k != "detect_emit"})):
        ctx.profile_start(100)
        rc = call({**good, **change})
        prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
        assert rc == 0 and prof == want, (change, prof)
        assert int(cnt.item()) == 1 and runs[0].tolist() == [0, 4096], (change, runs[0].tolist())
    assert call({**good, "channel": 1}) == 0 and int(cnt.item()) == 0
    assert call({**good, "channel": -1}) == 0 and int(cnt.item()) == 0
    ctx.profile_start(100)
    ctx.invalid_runs(x[:4096], inf, 1, 16, runs=runs)
    ctx.invalid_runs(x[:4096].view(4096, 1), inf, 1, 16, runs=runs, channel=0)              # channels = 1: the mono kernel
    prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
    assert prof == {"detect_bits": 2, "detect_carry": 2, "detect_count": 2, "detect_offsets": 2, "detect_emit": 2}, prof
    # the other routes launch what they launched
    z = torch.zeros(4096 * 2, device=dev)
    z[0::4] = 1.0
    ctx.profile_start(100)
    ctx.quiet_runs(z[:4096], 0.0, 1, 16, runs=runs)
    ctx.quiet_runs(z.view(4096, 2), 0.0, 1, 16, runs=runs, channel=0)
    ctx.dead_runs(z[:4096], 3, 0.0, 0.5, 0.0, 1, 16, runs=runs)
    ctx.dead_runs(z.view(4096, 2), 3, 0.0, 0.0, 0.0, 1, 16, runs=runs, channel=-1)
    ctx.level_runs(z[:4096], 48, 0.0, 0.5, 1, 16, runs=runs)
    ctx.level_runs(z.view(4096, 2), 7, 0.0, 0.0, 1, 16, runs=runs, channel=1)
    ctx.burst_runs(z[:4096], 48, 0.0, 0.5, 1, 16, runs=runs)
    ctx.burst_runs(z.view(4096, 2), 7, 2.0, 0.0, 1, 16, runs=runs, channel=1)
    prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
    assert prof == {"detect_bits": 1, "detect_bits_ch": 1, "detect_dead": 6, "detect_peak": 3, "detect_peak_final": 3, "detect_carry": 8,
                    "detect_count": 8, "detect_offsets": 8, "detect_emit": 8}, prof
