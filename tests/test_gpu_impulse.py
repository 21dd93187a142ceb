"""Clicks and pops by locally scaled AR prediction error on the device: si_impulse_runs and si_impulse_residual against
the float64 reference of tests/impulse_ref.py, for fp32, int16 and packed 24-bit.
    rows, the total, the untouched rows past them and T: exact equality.  Every case's builder has asserted E_p / r[0] > 1e-6 for every
        fitted block and that no comparison of a candidate sample lies within 2^-20 of equality (a seed that violates it is replaced), so no
        decision depends on the order in which the device adds a window's squares.  The float64 decisions themselves are held to the
        60-digit ones on the CPU (tests/test_impulse_ref.py); here the reference runs in float64 alone, which keeps a case at milliseconds.
    the residual tap: |e_gpu - e_ref| <= C_DEVICE * A(t), A(t) = sum |a_j| |x[t - j]|, C_DEVICE = 16 * the worst float64-against-exact ratio
        measured on the CPU cases (2^-46 -> 2^-42), under the cap 2^-24 at which a model formed in fp32 fails; NaN and 0.0 where stated.
Every input lies inside a longer device buffer with full-scale alternation planted in front of the base and behind the input: neither
may be read."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import dead_ref as R
from tests import impulse_ref as I
from tests import s24_ref as S
from tests.cases import _patch_engine as _engine

pytestmark = pytest.mark.gpu

TORCH = {np.float32: torch.float32, np.int16: torch.int16}
SENTINEL = -7
DTYPES = list(I.DTYPES)
IDS = ["fp32", "int16", "s24"]
OFFSETS = {np.float32: (4, 8, 12), np.int16: (2, 6, 14), I.S24: (1, 2, 3, 4, 5, 6, 7)}        # bytes past a 16-byte boundary
SIZES = (1, "p", "p+1", "4p", 255, 256, 257, 511, 512, 513, 767, 768, 769, 2047, 2048, 2049, 2305, 4101, 6144)
PAD, GUARD = 2, 4
HALVES = (GUARD + 1, 8, 254, 512, 1024 - PAD)
ORDERS = (2, 16, 32)
_REF = {}


def _trap(dtype, k, ch):
    """k sample times of full-scale alternation: the loudest thing there is, in front of the base and behind the input."""
    full = {np.float32: 1.0, np.int16: 32767, I.S24: 8388607}[dtype]
    v = np.resize(np.array([full, -full]), k).astype(dtype)
    return v if ch is None else np.repeat(v[:, None], ch, axis=1)


def _place(dev, case, off=0):
    """case.x on the device as a view whose first byte lies `off` bytes past a 16-byte boundary, loud samples in front of it and behind
    it (the case's own `after` when it has one).  24-bit values go packed: uint8 (n, [ch,] 3)."""
    x = case.x
    dtype, ch = x.dtype.type, (None if x.ndim == 1 else x.shape[1])
    behind = _trap(dtype, 1024, ch) if case.after is None else np.asarray(case.after, dtype)
    flat = np.concatenate([_trap(dtype, 64, ch), x, behind]).reshape(-1)
    start = 64 * (ch or 1)
    s24 = dtype is I.S24
    raw = S.pack(flat).reshape(-1) if s24 else flat.view(np.uint8)
    item = 3 if s24 else flat.itemsize
    assert s24 or off % item == 0
    first = start * item
    lead = 16 + (off - first) % 16
    buf = torch.zeros(lead + raw.size + 32, dtype=torch.uint8, device=dev)
    buf[lead:lead + raw.size] = torch.from_numpy(raw.copy())
    view = buf[lead + first:lead + first + x.size * item]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == off
    return view.view(*x.shape, 3) if s24 else view.view(TORCH[dtype]).view(x.shape)


def _args(case):
    k = case.kw
    return (k["order"], k["half"], k["guard"], k["pad"], k["ratio"], k["thr"], k["rel"], k["min_len"])


def _call(ctx, case, off=0, max_runs=4096, x=None):
    """-> (total, the rows written, the rows past them, T) of one si_impulse_runs call."""
    x = _place(ctx.device, case, off) if x is None else x
    runs = torch.full((max_runs + 8, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
    T = torch.full((1,), -1.0, dtype=torch.float32, device=ctx.device)
    _, n_runs = ctx.impulse_runs(x, *_args(case), max_runs, runs=runs, channel=case.kw["channel"], threshold_out=T)
    total = int(n_runs.item())
    rows = runs.cpu().numpy()
    k = min(total, max_runs)
    return total, rows[:k], rows[k:], T.cpu().numpy()[0]


def _want(case):
    """The reference's (rows, T, results) of a case, computed once, the builders' conditions asserted."""
    if id(case) not in _REF:
        _REF[id(case)] = (case, I.check(case))
    return _REF[id(case)][1]


def _check(ctx, case, **kw):
    want, T_ref, _ = _want(case)
    total, rows, rest, T = _call(ctx, case, **kw)
    what = (case.name, case.x.shape, str(case.x.dtype), kw)
    assert total == len(want), (what, total, len(want), rows[:6].tolist(), want[:6].tolist())
    assert len(rows) == min(total, kw.get("max_runs", 4096)) and np.array_equal(rows, want[:len(rows)]), (what, rows[:8].tolist(), want[:8].tolist())
    assert np.all(rest == SENTINEL), what
    assert T.tobytes() == np.float32(T_ref).tobytes(), (what, T, T_ref)
    return want


def _same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


def _decided(build):
    """build(seed) -> Case for the first seed of 0 .. 7 whose case passes the builders' conditions (a seed that puts a comparison within
    2^-20 of equality, or an ill-conditioned block, is replaced, as the conditions ask)."""
    for seed in range(8):
        case = build(seed)
        try:
            _want(case)
            return case
        except AssertionError:
            continue
    raise AssertionError("no seed of 0 .. 7 gives a decided case")


def _n_of(n, p):
    return {"p": p, "p+1": p + 1, "4p": 4 * p}.get(n, n)


def _spread(n, p):
    """Click positions of a size case: t = p, n - 1, and one on, before or after every block and chunk seam in turn, 300 apart at least."""
    at, last = [], -10 ** 9
    for k, s in enumerate(range(512, n, 512)):
        t = s + (k % 3) - 1
        if t - last >= 300 and t < n:
            at.append(t)
            last = t
    return sorted(set([t for t in (p, n - 1) if 0 <= t < n and all(abs(t - u) >= 40 for u in at)] + at))


def _sweep():
    out = []
    for n in SIZES:
        for h in HALVES:
            for p in ORDERS:
                if (h == 254 and p == 16) or n in (2049, 4101) or (h in (GUARD + 1, 1024 - PAD) and p == 32 and n in (1, "p", "p+1", "4p", 513, 6144)):
                    out.append((n, h, p))
    return out


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("p", ORDERS)
@pytest.mark.parametrize("h", HALVES)
def test_every_size_at_every_window_and_order(h, p):
    """n in {1, p, p + 1, 4 p, 255 .. 257, 511 .. 513, 767 .. 769, 2047 .. 2049, 2305, 4101, 6144} crossed with the five half windows and the
    three orders, thinned as DESIGN.md 4.28's grid is: every n meets (254, 16), every (h, p) meets 2049 and 4101, the extremes meet the
    smallest sizes and 6144.  Clicks at t = p, at n - 1 and on, before and after the seams; the sample type rotates."""
    ctx = _engine().ctx
    found = 0
    for k, (n, hh, pp) in enumerate(s for s in _sweep() if s[1] == h and s[2] == p):
        n = _n_of(n, p)
        dtype = DTYPES[k % 3]
        case = _decided(lambda seed: I.clicked(n, dtype, 10 * k + seed, _spread(n, p), "voiced" if k % 2 == 0 else "ar2", amp=0.9, order=p, half=h, guard=GUARD,
                                               pad=PAD))
        want = _check(ctx, case)
        assert n > p + 1 or len(want) == 0
        found += len(want)
    assert found > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_click_positions(dtype):
    """A click on, one before and one after every block seam and the chunk seams; two clicks 2 pad, 2 pad + 1 and 2 pad + 2 apart (one
    run, one run, two runs); a click in digital silence; a click at t = p and at n - 1."""
    ctx = _engine().ctx
    for s in (512, 1024, 1536, 2048, 2560, 4096):
        for d in (-1, 0, 1):
            # order = guard = 8: the click's own tail a_j * click, j = 1 .. 8, lies inside the guard, so the neighbourhood is the signal's alone
            case = _decided(lambda seed: I.clicked(4700, dtype, 100 + seed, (s + d,), amp=0.9, half=254, order=8, guard=8))
            want = _check(ctx, case)
            assert len(want) == 1 and want[0][0] <= s + d < want[0][0] + want[0][1] <= s + d + 9 + PAD, (s, d, want.tolist())
    for gap, runs in ((2 * PAD, 1), (2 * PAD + 1, 1), (2 * PAD + 2, 2)):
        x = np.zeros(3000, dtype)
        I.plant(x, 2040)
        I.plant(x, 2040 + gap)
        # order 2 sees no correlation at lags 4 .. 6: the model is the delta, e = x, and each click outweighs the other in its window
        want = _check(ctx, I.Case(f"two clicks {gap} apart", x, I.base_kw(half=100, order=2)))
        assert len(want) == runs, (gap, want.tolist())
    quiet = I.signal(4200, dtype, 7)
    quiet[1500:3300] = 0
    I.plant(quiet, 2300, amp=0.01)
    want = _check(ctx, I.Case("silence", quiet, I.base_kw(half=254)))
    assert any(r[0] <= 2300 < r[0] + r[1] for r in want.tolist())
    for p in ORDERS:
        for t in (p, 2999):
            x = np.zeros(3000, dtype)
            I.plant(x, t)
            assert _check(ctx, I.Case(f"click at {t}", x, I.base_kw(order=p, half=64))).tolist() == [[max(t - PAD, 0), min(t + PAD, 2999) - max(t - PAD, 0) + 1]]


def test_non_finite_samples():
    """NaN and +-inf at a fit window's first sample, its last sample and one past it: block 1's window is [256, 1280)."""
    ctx = _engine().ctx
    for v in (np.nan, np.inf, -np.inf):
        for at in (255, 256, 1279, 1280):
            x = I.signal(2600, np.float32, 21)
            for t in (300, 700, 1100, 1700, 2400):
                I.plant(x, t)
            x[at] = v
            case = I.Case(f"{v} at {at}", x, I.base_kw(half=64))
            _check(ctx, case)
            e = ctx.impulse_residual(_place(ctx.device, case), 16).cpu().numpy()
            ref = I.residual_ref(x).e
            assert np.array_equal(np.isnan(e), np.isnan(ref)), (v, at)
            assert np.isnan(e[512:1024]).all() == (256 <= at < 1280)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_residual_tap(dtype):
    """si_impulse_residual against the float64 reference sample by sample: |e - ref| <= C_DEVICE * A(t); 0.0 below p."""
    ctx = _engine().ctx
    worst = 0.0
    for k, (n, p) in enumerate(((1, 2), (2, 2), (33, 32), (700, 16), (2049, 2), (4101, 16), (4101, 32), (6144, 8))):
        for kind in ("voiced", "ar2"):
            case = I.clicked(n, dtype, 40 + k, _spread(n, p), kind, order=p)
            ref = I.residual_ref(case.x, order=p)
            assert all(rt is None or rt > 1e-6 for rt in ref.ratios)
            for off in (0, OFFSETS[dtype][k % len(OFFSETS[dtype])]):
                e = ctx.impulse_residual(_place(ctx.device, case, off), p).cpu().numpy()
                assert e.shape == (n,) and np.all(e[:p] == 0.0)
                err, bound = np.abs(e - ref.e), I.C_DEVICE * ref.A
                assert np.all(err <= bound), (case.name, float(np.max(err / np.maximum(ref.A, 1e-300))))
                worst = max(worst, float(np.max(np.where(ref.A > 0, err / np.maximum(ref.A, 1e-300), 0.0))))
    print(f"worst |e_gpu - e_ref| / A = {worst:.3e} against C_DEVICE = {I.C_DEVICE:.3e}")
    # one channel of an interleaved file: that channel's elements, never the adjacent ones
    st = I.stereo_case(dtype)
    for c in (0, 1):
        e = ctx.impulse_residual(_place(ctx.device, st), 16, channel=c).cpu().numpy()
        ref = I.residual_ref(st.x, 16, channel=c)
        assert np.all(np.abs(e - ref.e) <= I.C_DEVICE * ref.A), c


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_base_pointer_off_the_grids(dtype):
    """Bases off the 4-, 8- and 16-byte grids; packed 24-bit at every byte offset 0 .. 7."""
    ctx = _engine().ctx
    for n, h, p in ((700, 8, 2), (2049, 254, 16), (4101, 512, 32)):
        case = _decided(lambda seed: I.clicked(n, dtype, 60 + seed, _spread(n, p), amp=0.9, order=p, half=h))
        first = _call(ctx, case)
        for off in OFFSETS[dtype]:
            _check(ctx, case, off=off)
            assert _same(_call(ctx, case, off=off), first)


def test_packed_24_bit_equals_its_fp32_image():
    """Each s24 result equals the call on the fp32 image v / 2^23 (exact) with the threshold scaled: every float64 step scales by a
    power of two."""
    ctx = _engine().ctx
    for thr in (0.0, 0.2):
        case = _decided(lambda seed: I.clicked(4101, I.S24, 70 + seed, (600, 2047, 3000), amp=0.9, order=8, guard=8, half=254, thr=thr * 8388608.0))
        img = I.Case("image", (case.x.astype(np.float64) / 8388608.0).astype(np.float32), {**case.kw, "thr": thr})
        a, b = _call(ctx, case), _call(ctx, img)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and float(a[3]) == float(b[3]) * 8388608.0 and a[0] > 0
        _check(ctx, case)


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("ch", [2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_interleaved_files(dtype, ch):
    """One channel of (n, ch) and the joint mode: each channel has clicks of its own and one all share.  channel = c gives the bytes of
    the mono call on the de-interleaved copy; joint = every channel's dead_c, against one T from the peak over all elements."""
    ctx = _engine().ctx

    def build(seed):
        cols = []
        for c in range(ch):
            x = I.signal(2500, dtype, 200 + 10 * seed + c, "voiced" if c % 2 == 0 else "ar2")
            I.plant(x, 300 + 250 * c, amp=0.9)
            I.plant(x, 2300, amp=0.9)
            cols.append(x)
        return np.stack(cols, axis=1)

    for channel in list(range(ch)) + [-1]:
        for rel in (0.0, 0.5):
            case = _decided(lambda seed: I.Case(f"{ch} channels, channel {channel}", build(seed), I.base_kw(half=100, order=8, guard=8, channel=channel, rel=rel)))
            want = _check(ctx, case)
            _check(ctx, case, off=OFFSETS[dtype][0])
            assert any(r[0] <= 2300 < r[0] + r[1] for r in want.tolist()) or rel > 0
            if channel >= 0:
                mono = I.Case("mono", np.ascontiguousarray(case.x[:, channel]), {**case.kw, "channel": None})
                assert _same(_call(ctx, case), _call(ctx, mono)), case.name
            elif rel == 0.0:
                assert len(want) == 1


def test_one_channel_as_an_interleaved_file():
    ctx = _engine().ctx
    case = _decided(lambda seed: I.clicked(2500, np.int16, 80 + seed, (511, 1400), amp=0.9, half=100))
    want = _call(ctx, case)
    for channel in (0, -1):
        one = I.Case(case.name, case.x.reshape(-1, 1), {**case.kw, "channel": channel})
        assert _same(_call(ctx, one), want), channel


# ------------------------------------------------------------------------------------------------------------ 3
def test_past_the_tile_seam_of_the_carry():
    """An int16 file of 1027 chunks, silent but for two stretches of signal: clicks on both sides of the carry tile's seam (chunk 1023 |
    1024), in the first chunk and in the last, partial one; the peak lies in the last chunk."""
    ctx = _engine().ctx
    n = 1026 * 2048 + 900
    x = np.zeros(n, np.int16)
    seam = 1024 * 2048
    x[seam - 3000:seam + 3000] = I.signal(6000, np.int16, 31)
    x[n - 800:] = I.signal(800, np.int16, 32)
    x[n - 5] = 30000
    clicks = (100, seam - 1, seam + 700, n - 300)
    for t in clicks:
        I.plant(x, t, amp=0.9)
    want = _check(ctx, I.Case("1027 chunks", x, I.base_kw(half=64, order=8, guard=8, rel=0.05)))
    assert all(any(r[0] <= t < r[0] + r[1] for r in want.tolist()) for t in clicks)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_max_runs_repeated_calls_and_a_fresh_context(dtype):
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from tests.harness import build_engine
    ctx = _engine().ctx
    case = _decided(lambda seed: I.clicked(4101, dtype, 90 + seed, (300, 1023, 2048, 3500), amp=0.9, half=64, order=8, guard=8))
    want = _check(ctx, case)
    assert len(want) >= 3
    for cap in (0, 1, len(want) - 1, len(want), len(want) + 1):
        total, rows, rest, T = _call(ctx, case, max_runs=cap)
        assert total == len(want) and np.array_equal(rows, want[:cap]) and np.all(rest == SENTINEL), cap
    assert _same(_call(ctx, case), _call(ctx, case))
    big = _decided(lambda seed: I.clicked(6144, dtype, 95 + seed, (2047, 4000), amp=0.9, half=1022, order=32))
    small = _decided(lambda seed: I.clicked(2049, dtype, 97 + seed, (1024,), amp=0.9, half=8, order=2))
    _check(ctx, big)
    after = _call(ctx, small)
    e_after = ctx.impulse_residual(_place(ctx.device, small), 2).cpu()
    fresh = build_engine(HubertArch.tiny(), VocoderArch.tiny(), 100).ctx
    assert _same(after, _call(fresh, small)) and len(after[1]) > 0
    assert torch.equal(e_after.view(torch.int64), fresh.impulse_residual(_place(fresh.device, small), 2).cpu().view(torch.int64))
    _check(fresh, big)


def test_poisoned_workspace_and_guard_bands():
    """under poisoned allocations, after a long hot call, a result equals a fresh context's bit for bit; with
    runs, n_runs and e between guard bands of either fill, no byte outside them is written."""
    from tests import extent as X
    from tests import poison as P
    from tests import test_gpu_scratch as G
    assert "detect_dead" in P.SCRATCH_FAMILIES
    used = G._fresh_ctx()

    def run(ctx, x, c, kw, max_runs=64):
        T = torch.empty(1, dtype=torch.float32, device=ctx.device)
        runs, n = ctx.impulse_runs(x, kw["order"], kw["half"], kw["guard"], kw["pad"], kw["ratio"], kw["thr"], kw["rel"], kw["min_len"], max_runs,
                                   channel=c, threshold_out=T)
        return [runs, n, T]

    try:
        long = torch.zeros(2 * 1024 * 2048 + 4101, dtype=torch.int16)
        long[::3] = 20000                                              # a click every third sample of digital silence
        long = long.cuda()
        with P.poisoned_allocs():
            out = run(used, long, None, I.base_kw(order=2, half=5, guard=4, pad=16, rel=0.5), 4)
            assert int(out[1][0]) >= 0
            for dtype in (np.float32, np.int16):
                for n, h, p in ((700, 8, 2), (2049, 254, 16), (4101, 1008, 32)):
                    case = _decided(lambda seed: I.clicked(n, dtype, 300 + seed, _spread(n, p), amp=0.9, order=p, half=h, pad=16 if h == 1008 else 2, rel=0.1))
                    x = torch.from_numpy(case.x).cuda()
                    call = lambda ctx: run(ctx, x, None, case.kw)
                    got = [t.cpu() for t in call(used)]
                    G._same(G._written(got), G._written(G._on_fresh(call)), (dtype, n, h, p))
                    assert got[0][:int(got[1][0])].tolist() == _want(case)[0].tolist()
        case = _decided(lambda seed: I.clicked(4101, np.float32, 310 + seed, _spread(4101, 16), amp=0.9, half=254))
        x = torch.from_numpy(case.x).cuda()
        for fill in X.FILLS:
            snap = X.unchanged({"x": x})
            with X.guarded_allocs(fill) as rec:
                runs, cnt = used.impulse_runs(x, *_args(case), 5)
                e = used.impulse_residual(x, 16)
                torch.cuda.synchronize()
            assert len(rec.allocs) >= 3 and int(cnt[0]) == len(_want(case)[0]) and bool(torch.isfinite(e).all())
            rec.check()
            snap.check()
    finally:
        used.close()


def test_find_impulse_runs_and_the_engine_tap():
    eng = _engine()
    x = np.zeros(3000, np.float32)
    x[1500] = 0.5
    assert eng.find_impulse_runs(x, half=64).tolist() == [[1498, 5]] and eng.find_impulse_runs(x, win=129, pad=0).tolist() == [[1500, 1]]
    runs, T = eng.find_impulse_runs(x, half=64, rel_threshold=0.5, return_threshold=True)
    assert runs.dtype == torch.int32 and runs.is_cuda and T == 0.25 and runs.tolist() == [[1498, 5]]
    assert eng.find_impulse_runs(x, half=64, threshold=0.6).shape == (0, 2)
    two = np.stack([x, np.roll(x, 100)], axis=1)
    assert eng.find_impulse_runs(two, half=64, channel=1).tolist() == [[1598, 5]] and eng.find_impulse_runs(two, half=64, channel=-1).shape == (0, 2)
    assert eng.find_impulse_runs(S.pack(np.int32(x * 8388608 * 0.999)), half=64).tolist() == [[1498, 5]]
    e = eng.impulse_residual(x)
    assert e.dtype == torch.float64 and e.is_cuda and e.shape == (3000,) and float(e[1500]) == 0.5 and int((e != 0).sum()) == 1
    assert float(eng.impulse_residual(two, channel=1)[1600]) == 0.5
    with pytest.raises(ValueError, match="needs channel"):
        eng.find_impulse_runs(two, half=64)
    with pytest.raises(ValueError, match=r"half = 4 samples is under guard \+ 1 = 5"):
        eng.find_impulse_runs(x, half=4)
    with pytest.raises(ValueError, match=r"half \+ pad = 1026 samples, above 1024"):
        eng.find_impulse_runs(x, half=1024)
    with pytest.raises(ValueError, match=r"ratio = 0.5 is NaN or outside \[1, 1e6\]"):
        eng.find_impulse_runs(x, half=64, ratio=0.5)


# ------------------------------------------------------------------------------------------------------------ 4
def test_refusals_come_before_any_launch():
    ctx = _engine().ctx
    lib, h, dev = ctx.lib, ctx._h, ctx.device
    x = torch.zeros(4096 * 2, device=dev)
    x[2 * 2000] = 0.5                                                   # channel 0 of (4096, 2): one click at time 2000
    runs = torch.full((16, 2), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    T = torch.full((1,), -1.0, dtype=torch.float32, device=dev)
    e = torch.full((4096,), -3.0, dtype=torch.float64, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(x=x, pcm=0, n=4096, channels=2, channel=0, order=16, half=256, guard=4, pad=2, ratio=10.0, thr=0.0, rel=0.5, min_len=1, runs=runs,
                max_runs=16, cnt=cnt)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(x=None), "x is NULL"), (dict(cnt=None), "n_runs is NULL"), (dict(runs=None), "runs is NULL with max_runs = 16"),
             (dict(n=0), "n = 0 samples"), (dict(n=2 ** 31 - 1 - 2047), "n = 2147481600 samples"), (dict(thr=-1e-9), "threshold = -1e-09 is negative or NaN"),
             (dict(thr=nan), "threshold = -?nan is negative or NaN"), (dict(min_len=0), "min_len = 0 samples"), (dict(max_runs=-1), "max_runs = -1 is negative"),
             (dict(channels=0), "channels = 0, outside 1 .. SI_MAX_CHANNELS = 8"), (dict(channels=9), "channels = 9, outside"),
             (dict(channel=2), "channel = 2, outside -1 .. 1"), (dict(channel=-2), "channel = -2, outside -1 .. 1"),
             (dict(order=1), "order = 1, outside 2 .. SI_IMPULSE_MAX_ORDER = 32"), (dict(order=33), "order = 33, outside 2 .. SI_IMPULSE_MAX_ORDER = 32"),
             (dict(guard=-1), "guard = -1 samples, outside 0 .. SI_IMPULSE_MAX_GUARD = 64"), (dict(guard=65), "guard = 65 samples, outside 0 .. SI_IMPULSE_MAX_GUARD = 64"),
             (dict(half=4), r"half = 4 samples, outside guard \+ 1 = 5 .. SI_IMPULSE_MAX_HALF = 1024"),
             (dict(half=1025, pad=0), r"half = 1025 samples, outside guard \+ 1 = 5 .. SI_IMPULSE_MAX_HALF = 1024"),
             (dict(pad=-1), "pad = -1 samples, outside 0 .. SI_IMPULSE_MAX_PAD = 16"), (dict(pad=17), "pad = 17 samples, outside 0 .. SI_IMPULSE_MAX_PAD = 16"),
             (dict(half=1023), r"half \+ pad = 1025 samples, above SI_IMPULSE_MAX_HALF = 1024"),
             (dict(ratio=nan), r"ratio = -?nan is NaN or outside \[1, 1e6\]"), (dict(ratio=0.99), r"ratio = 0.99 is NaN or outside \[1, 1e6\]"),
             (dict(ratio=2e6), r"ratio = 2e\+06 is NaN or outside \[1, 1e6\]"), (dict(thr=inf), "threshold = inf is not finite"),
             (dict(rel=nan), r"rel_threshold = -?nan is NaN or outside \[0, 4\]"), (dict(rel=-0.1), r"rel_threshold = -0.1 is NaN or outside \[0, 4\]"),
             (dict(rel=4.5), r"rel_threshold = 4.5 is NaN or outside \[0, 4\]")]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda a: lib.si_impulse_runs(h, P(a["x"]), a["pcm"], a["n"], a["channels"], a["channel"], a["order"], a["half"], a["guard"], a["pad"],
                                         a["ratio"], a["thr"], a["rel"], a["min_len"], P(a["runs"]), a["max_runs"], P(a["cnt"]), P(T), stream)
    for change, msg in cases:
        ctx.profile_start(100)
        rc = call({**good, **change})
        launched = [q for q in ctx.profile_stop() if q["launches"] > 0]
        err = lib.si_last_error(h).decode()
        assert rc == -1 and launched == [], (change, rc, launched)
        assert re.search("si_impulse_runs: " + msg, err), (change, err)
    tap = lambda a: lib.si_impulse_residual(h, P(a["x"]), 0, a["n"], a["channels"], a["channel"], a["order"], P(a.get("e", e)), stream)
    for change, msg in ((dict(x=None), "x is NULL"), (dict(e=None), "e is NULL"), (dict(n=0), "n = 0 samples"), (dict(channel=-1), "channel = -1, outside 0 .. 1"),
                        (dict(channels=9), "channels = 9, outside"), (dict(order=1), "order = 1, outside 2 .. SI_IMPULSE_MAX_ORDER = 32"),
                        (dict(order=33), "order = 33, outside")):
        ctx.profile_start(100)
        rc = tap({**good, **change})
        launched = [q for q in ctx.profile_stop() if q["launches"] > 0]
        assert rc == -1 and launched == [] and re.search("si_impulse_residual: " + msg, lib.si_last_error(h).decode()), change
    torch.cuda.synchronize()
    assert bool((runs == SENTINEL).all()) and int(cnt.item()) == SENTINEL and float(T.item()) == -1.0 and bool((e == -3.0).all())
    # the same arguments unchanged are served: one launch in pass 1's family, pass 0 only with rel > 0, both ends of every range are legal
    names = {"detect_dead": 1, "detect_carry": 1, "detect_count": 1, "detect_offsets": 1, "detect_emit": 1}
    peak = {**names, "detect_peak": 1, "detect_peak_final": 1}
    for change, want in ((dict(), peak), (dict(rel=0.0), names), (dict(order=2, guard=0, half=1, pad=0, rel=0.9, thr=0.3), peak),
                         (dict(order=32, guard=64, half=1008, pad=16, ratio=1.0), peak), (dict(ratio=1e6), peak),
                         (dict(max_runs=0, runs=None), {k: v for k, v in peak.items() if k != "detect_emit"})):
        ctx.profile_start(100)
        rc = call({**good, **change})
        prof = {q["name"]: q["launches"] for q in ctx.profile_stop()}
        assert rc == 0 and prof == want, (change, prof)
        pad = change.get("pad", 2)
        assert int(cnt.item()) == 1 and runs[0].tolist() == [2000 - pad, 2 * pad + 1], (change, runs[0].tolist())
    assert call({**good, "rel": 4.0}) == 0 and int(cnt.item()) == 0 and float(T.item()) == 2.0     # |e| = 0.5 < T: nothing is hot
    ctx.profile_start(100)
    assert tap(good) == 0
    assert {q["name"]: q["launches"] for q in ctx.profile_stop()} == {"detect_dead": 1} and float(e[2000]) == 0.5 and float(e[0]) == 0.0
    assert lib.si_impulse_runs(h, P(x), 0, 4096, 2, 0, 16, 256, 4, 2, 10.0, 0.0, 0.0, 1, P(runs), 16, P(cnt), C.c_void_p(0), stream) == 0
    # the five existing detectors launch what they launched
    ctx.profile_start(100)
    ctx.quiet_runs(x[:4096], 0.0, 1, 16, runs=runs)
    ctx.quiet_runs(x.view(4096, 2), 0.0, 1, 16, runs=runs, channel=0)
    ctx.dead_runs(x[:4096], 3, 0.0, 0.5, 0.0, 1, 16, runs=runs)
    ctx.dead_runs(x.view(4096, 2), 3, 0.0, 0.0, 0.0, 1, 16, runs=runs, channel=-1)
    ctx.level_runs(x[:4096], 48, 0.0, 0.5, 1, 16, runs=runs)
    ctx.level_runs(x.view(4096, 2), 7, 0.0, 0.0, 1, 16, runs=runs, channel=1)
    ctx.burst_runs(x[:4096], 44, 1.15, 0.0, 1, 16, runs=runs)
    ctx.burst_runs(x.view(4096, 2), 7, 0.0, 0.5, 1, 16, runs=runs, channel=1)
    ctx.invalid_runs(x[:4096], float("inf"), 1, 16, runs=runs)
    ctx.invalid_runs(x.view(4096, 2), 0.4, 1, 16, runs=runs, channel=-1)
    prof = {q["name"]: q["launches"] for q in ctx.profile_stop()}
    assert prof == {"detect_bits": 2, "detect_bits_ch": 2, "detect_dead": 6, "detect_peak": 3, "detect_peak_final": 3, "detect_carry": 10,
                    "detect_count": 10, "detect_offsets": 10, "detect_emit": 10}, prof
