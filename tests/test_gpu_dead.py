"""Held-sample and peak-relative dropouts on the device: si_dead_runs against the numpy reference of tests/dead_ref.py --
the total, every (start, len) row and the untouched rows past them, exact integer equality; the effective threshold bit for bit.
Every input lies inside a longer device buffer with one sample time planted in front of the base and one behind the input: copies of
x[0] and x[n - 1] (a link to either would lengthen a run) or a magnitude above the peak."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import dead_ref as R
from tests import detect_ref as D
from tests.cases import _patch_engine as _engine

pytestmark = pytest.mark.gpu

TORCH = {np.float32: torch.float32, np.int16: torch.int16}
SENTINEL = -7


def _place(dev, case, off=0):
    """case.x on the device as a view that starts `off` elements past a 16-byte boundary, its traps in front of it and behind it."""
    flat, ch = case.memory()
    start = 16 + off                                                    # elements; 16 elements are a multiple of 16 bytes
    buf = torch.zeros(start + flat.size + 16, dtype=TORCH[flat.dtype.type], device=dev)
    buf[start - ch:start - ch + flat.size] = torch.from_numpy(flat)
    view = buf[start:start + case.x.size]
    assert view.data_ptr() % 16 == (off * flat.itemsize) % 16
    return view.view(case.x.shape)


def _call(ctx, case, off=0, max_runs=4096, x=None):
    """-> (total, the rows written, the rows past them, T) of one si_dead_runs call."""
    x = _place(ctx.device, case, off) if x is None else x
    runs = torch.full((max_runs + 8, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
    T = torch.full((1,), -1.0, dtype=torch.float32, device=ctx.device)
    _, n_runs = ctx.dead_runs(x, case.kind, case.thr, case.rel, case.tol, case.min_len, max_runs, runs=runs, channel=case.channel, threshold_out=T)
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


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n", R.SEAM_N)
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_runs_at_the_thread_wave_and_chunk_seams(dtype, n):
    """tests/dead_ref.py::seam_masks for kinds 1, 2 and 3: held pairs across every multiple of 8, runs ending on, starting on and
    crossing the wave and chunk seams, whole held chunks inside a run, lengths min_len - 1 / min_len / min_len + 1, pairs at both
    ends; x[-1] == x[0] and x[n] == x[n - 1] lie in memory and must not link."""
    ctx = _engine().ctx
    found = 0
    for case in R.seam_cases(n, dtype):
        found += len(_check(ctx, case))
    assert found > 0


@pytest.mark.parametrize("dtype,offsets", [(np.float32, (1, 2, 3)), (np.int16, (1, 3, 7))])
def test_a_base_pointer_off_the_16_byte_grid(dtype, offsets):
    """Views 1 - 3 floats / 1, 3, 7 int16 off the grid take the staged loads, in the peak's pass too; the traps are still there."""
    ctx = _engine().ctx
    for n in (9, 2049, 4101):
        for case in R.seam_cases(n, dtype):
            for off in offsets:
                _check(ctx, case, off=off)
    for case in R.peak_position_cases(dtype):
        for off in offsets:
            _check(ctx, case, off=off)


def test_value_edges():
    """|diff| == tol and the float above it, 0.0 | -0.0, NaN, inf - inf, 32767 | -32768, subnormal steps; T bit-equal to the fp32
    product at rel = 1e-3, the peak over the finite samples only, all NaN, rel = 1, |-32768|."""
    ctx = _engine().ctx
    for case in R.value_cases():
        _check(ctx, case)


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_the_peak_wherever_it_lies(dtype):
    """The peak at the first sample, the last one, in a partial last chunk; a larger magnitude in front of the base and behind the
    input does not count.  The mute at 1 / 64 of the noise floor is found through the peak, and not at threshold 0."""
    ctx = _engine().ctx
    for case in R.peak_position_cases(dtype):
        assert _check(ctx, case).tolist() == [[100, 60]]
        assert len(_check(ctx, R.Case(case.name + ", no rel", case.x, R.QUIET, 0.0, 0.0, 0.0, 8, None, case.before, case.after))) == 0


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("ch", [2, 3, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_interleaved_files(dtype, ch):
    """One channel of (n, ch) and the joint mode: neighbours are (i +- 1) ch + c -- equal values in adjacent channels of one time and
    across the time seam do not link --, each channel's peak is its own and the joint one is the file's.  channel = c gives the
    bytes of the mono call on the de-interleaved copy."""
    ctx = _engine().ctx
    for case in R.channel_cases(ch, dtype):
        for off in (0, 1):
            _check(ctx, case, off=off)
        if case.channel >= 0:
            col = np.ascontiguousarray(case.x[:, case.channel])
            mono = R.Case("mono", col, case.kind, case.thr, case.rel, case.tol, case.min_len, None)
            a, b = _call(ctx, case), _call(ctx, mono)
            assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes(), case.name


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_one_channel_as_an_interleaved_file(dtype):
    """channels = 1 (channel 0 or -1) gives the mono call's bytes."""
    ctx = _engine().ctx
    cases = R.seam_cases(4101, dtype)[::7] + R.peak_position_cases(dtype)[:2]
    for case in cases:
        want = _call(ctx, case)
        for channel in (0, -1):
            one = R.Case(case.name, case.x.reshape(-1, 1), case.kind, case.thr, case.rel, case.tol, case.min_len, channel, case.before, case.after)
            got = _call(ctx, one)
            assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[3].tobytes() == want[3].tobytes(), (case.name, channel)
            _check(ctx, one)


# ------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_equivalences(dtype):
    """kind = QUIET with rel = 0 gives si_quiet_runs' bytes on tests/detect_ref.py::seam_cases; a repeated call gives the same bytes."""
    ctx = _engine().ctx
    for n in (7, 2049, 6144):
        for name, q, min_len in D.seam_cases(n):
            x = D.materialize(q, dtype, n)
            case = R.Case(name, x, R.QUIET, D.THR[dtype], 0.0, 0.0, min_len)
            dev = _place(ctx.device, case)
            total, rows, rest, T = _call(ctx, case, x=dev)
            runs = torch.full((4096 + 8, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
            _, n_runs = ctx.quiet_runs(dev, D.THR[dtype], min_len, 4096, runs=runs)
            assert total == int(n_runs.item()) and np.array_equal(np.concatenate([rows, rest]), runs.cpu().numpy()), (n, name)
            assert T == np.float32(D.THR[dtype])
    case = R.seam_cases(6144, dtype)[-4]
    case = R.Case(case.name, case.x, R.ANY, case.thr, 2.0 ** -9, 0.0, 1)
    a, b = _call(ctx, case), _call(ctx, case)
    assert a[0] == b[0] > 0 and a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes()
    _check(ctx, case)
    want = case.rows()
    for cap in (1, len(want) - 1, len(want), len(want) + 1):
        total, rows, rest, _ = _call(ctx, case, max_runs=cap)
        assert total == len(want) and np.array_equal(rows, want[:cap]) and np.all(rest == SENTINEL), cap


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_past_the_tile_seam_of_the_final_reduce_and_of_the_carry(dtype):
    """1027 workgroups: the peak's final reduce and the carry scan take two tiles.  A held run spans chunks 1023 | 1024 with whole
    held chunks inside it, the peak lies in the last chunk, larger values lie outside the input."""
    ctx = _engine().ctx
    case = R.long_case(dtype)
    seam = R.TILE * R.CHUNK
    assert _check(ctx, case).tolist() == [[5000, 400], [seam - R.CHUNK - 1000, 2 * R.CHUNK + 1200]]
    assert len(_check(ctx, R.Case("held only", case.x, R.HELD, 0.0, 0.0, 0.0, 64, None, case.before, case.after))) == 1


# ------------------------------------------------------------------------------------------------------------ 4
def test_find_dead_runs():
    eng = _engine()
    case = R.peak_position_cases(np.float32)[2]
    runs, T = eng.find_dead_runs(case.x, "quiet", rel_threshold=case.rel, min_len=8, return_threshold=True)
    assert runs.dtype == torch.int32 and runs.is_cuda and runs.tolist() == [[100, 60]] and np.float32(T).tobytes() == case.threshold().tobytes()
    x = np.float32([1, 2, 2, 2, 0, 5, 0, 0, 7])
    assert eng.find_dead_runs(x, "held").tolist() == [[1, 3], [6, 2]]
    assert eng.find_dead_runs(x).tolist() == [[1, 4], [6, 2]] and eng.find_dead_runs(x, "quiet").tolist() == [[4, 1], [6, 2]]
    assert eng.find_dead_runs(x, "held", min_len=3).tolist() == [[1, 3]] and eng.find_dead_runs(x, "held", min_len=4).shape == (0, 2)
    two = np.stack([x, np.float32([3, 3, 3, 1, 0, 1, 2, 2, 2])], axis=1)
    assert eng.find_dead_runs(two, "held", channel=1).tolist() == [[0, 3], [6, 3]]
    assert eng.find_dead_runs(two, "held", channel=-1).tolist() == [[1, 2], [6, 2]]
    assert eng.find_dead_runs(x.reshape(-1, 1), "held", channel=0).tolist() == [[1, 3], [6, 2]]
    with pytest.raises(ValueError, match=r"2 runs .* more than max_runs = 1"):
        eng.find_dead_runs(x, "held", max_runs=1)
    with pytest.raises(ValueError, match="kind = 'loud'"):
        eng.find_dead_runs(x, "loud")
    with pytest.raises(ValueError, match="needs channel"):
        eng.find_dead_runs(two, "held")
    with pytest.raises(ValueError, match="channel = 1 of a one-channel recording"):
        eng.find_dead_runs(x, "held", channel=1)


# ------------------------------------------------------------------------------------------------------------ 5
def test_refusals_come_before_any_launch():
    ctx = _engine().ctx
    lib, h, dev = ctx.lib, ctx._h, ctx.device
    x = torch.zeros(4096 * 2, device=dev)
    runs = torch.full((16, 2), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    T = torch.full((1,), -1.0, dtype=torch.float32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(x=x, pcm=0, n=4096, channels=2, channel=0, kind=3, thr=0.0, rel=0.5, tol=0.0, min_len=1, runs=runs, max_runs=16, cnt=cnt)
    nan = float("nan")
    cases = [(dict(x=None), "x is NULL"), (dict(cnt=None), "n_runs is NULL"), (dict(runs=None), "runs is NULL with max_runs = 16"),
             (dict(n=0), "n = 0 samples"), (dict(n=2 ** 31 - 1 - 2047), "n = 2147481600 samples"), (dict(thr=-1e-9), "threshold = -1e-09 is negative or NaN"),
             (dict(thr=nan), "threshold = -?nan is negative or NaN"), (dict(min_len=0), "min_len = 0 samples"), (dict(max_runs=-1), "max_runs = -1 is negative"),
             (dict(channels=0), "channels = 0, outside 1 .. SI_MAX_CHANNELS = 8"), (dict(channels=9), "channels = 9, outside"),
             (dict(channel=2), "channel = 2, outside -1 .. 1"), (dict(channel=-2), "channel = -2, outside -1 .. 1"),
             (dict(channels=1, channel=1), "channel = 1, outside -1 .. 0"),
             (dict(kind=0), "kind = 0, outside 1 .. 3"), (dict(kind=4), "kind = 4, outside 1 .. 3"), (dict(kind=-1), "kind = -1, outside 1 .. 3"),
             (dict(rel=nan), "rel_threshold = -?nan is NaN or outside"), (dict(rel=-0.1), "rel_threshold = -0.1 is NaN or outside"),
             (dict(rel=1.5), "rel_threshold = 1.5 is NaN or outside"),
             (dict(tol=-1.0), "held_tol = -1 is negative or NaN"), (dict(tol=nan), "held_tol = -?nan is negative or NaN"),
             (dict(tol=-1.0, kind=1), "held_tol = -1 is negative or NaN")]        # validated even when kind lacks HELD
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda a: lib.si_dead_runs(h, P(a["x"]), a["pcm"], a["n"], a["channels"], a["channel"], a["kind"], a["thr"], a["rel"], a["tol"], a["min_len"],
                                      P(a["runs"]), a["max_runs"], P(a["cnt"]), P(T), stream)
    for change, msg in cases:
        ctx.profile_start(100)
        rc = call({**good, **change})
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        err = lib.si_last_error(h).decode()
        assert rc == -1 and launched == [], (change, rc, launched)                               # SI_EINVAL
        assert re.search("si_dead_runs: " + msg, err), (change, err)
    torch.cuda.synchronize()
    assert bool((runs == SENTINEL).all()) and int(cnt.item()) == SENTINEL and float(T.item()) == -1.0
    # the same arguments unchanged are served: pass 0 only with rel > 0, and a NULL threshold_out is fine
    names = {"detect_dead": 1, "detect_carry": 1, "detect_count": 1, "detect_offsets": 1, "detect_emit": 1}
    for change, want in ((dict(), {**names, "detect_peak": 1, "detect_peak_final": 1}), (dict(rel=0.0), names), (dict(channels=1), {**names, "detect_peak": 1, "detect_peak_final": 1})):
        ctx.profile_start(100)
        rc = call({**good, **change})
        prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
        assert rc == 0 and prof == want, (change, prof)
        assert int(cnt.item()) == 1 and runs[0].tolist() == [0, 4096]
    assert float(T.item()) == 0.0
    assert lib.si_dead_runs(h, P(x), 0, 4096, 2, 0, 3, 0.0, 0.0, 0.0, 1, P(runs), 16, P(cnt), C.c_void_p(0), stream) == 0
    # the quiet routes launch what they launched
    ctx.profile_start(100)
    ctx.quiet_runs(x[:4096], 0.0, 1, 16, runs=runs)
    ctx.quiet_runs(x.view(4096, 2), 0.0, 1, 16, runs=runs, channel=0)
    prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
    assert prof == {"detect_bits": 1, "detect_bits_ch": 1, "detect_carry": 2, "detect_count": 2, "detect_offsets": 2, "detect_emit": 2}, prof
