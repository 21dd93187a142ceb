"""si_mend_runs on the device against tests/mend_ref.py: statuses equal, fp32 within one rounding of the float64
reference, PCM equal (+-1 step only where the unrounded reference lies within 2^-30 P of a half-integer), for every sample type, an
s24 view at every byte offset and interleaved files; the status boundaries one sample on either side; and the invariants: guard
bands around x and status, every sample outside a filled run keeps its bits, a row alone equals the row in a table, repeated and
fresh-context calls give the same bits, refusals and an empty table launch nothing.

Every case is first held to the condition under which the bounds are stated, on the CPU: E_p / r[0] > 1e-6 (or r[0] == 0) in the
reference, and |float64 reference - 60-digit evaluation| < 2^-34 P with P = max |window|."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import extent
from tests import mend_ref as M
from tests import s24_ref as S

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = [np.float32, np.int16, M.S24]
IDS = ["fp32", "int16", "s24"]
TORCH = {np.float32: torch.float32, np.int16: torch.int16}
LENS = (1, 2, 3, 16, 63, 64, 65)
FILLED = (M.AR, M.LINE)
WORST = {}                                             # sample type -> the worst observed |gpu - ref| / bound (fp32) or exception count (PCM)
_CTX = []


def _ctx():
    if not _CTX:
        from speech_inpainting_amd import native
        from speech_inpainting_amd.arch import HubertArch, VocoderArch
        _CTX.append(native.NativeContext(native.make_desc(HubertArch.tiny(), VocoderArch.tiny(), 50), torch.device("cuda:0")))
    return _CTX[0]


def _fresh_ctx():
    from speech_inpainting_amd import native
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return native.NativeContext(native.make_desc(HubertArch.tiny(), VocoderArch.tiny(), 50), torch.device("cuda:0"))


# ------------------------------------------------------------------------------------------------------------ placing a file on the device
def _raw(x):
    """The file's bytes as they lie in memory: packed 3-byte samples for S24."""
    return S.pack(x).reshape(-1) if x.dtype.type is M.S24 else np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _unraw(raw, like):
    if like.dtype.type is M.S24:
        return S.unpack(raw.reshape(*like.shape, 3)).astype(M.S24)
    return raw.view(like.dtype).reshape(like.shape)


class Placed:
    """x on the device inside a longer byte buffer filled with `fill` (0xFF: a NaN for fp32, -1 for PCM) in front of it and behind it,
    its first byte `off` bytes past a 16-byte boundary."""
    def __init__(self, x, dev, off=0, fill=0xFF, band=4096):
        self.x, self.fill, self.raw = x, fill, _raw(x)
        s24 = x.dtype.type is M.S24
        assert s24 or off % x.itemsize == 0
        self.lead = band + off
        self.buf = torch.full((self.lead + self.raw.size + band,), fill, dtype=torch.uint8, device=dev)
        self.buf[self.lead:self.lead + self.raw.size] = torch.from_numpy(self.raw.copy())
        view = self.buf[self.lead:self.lead + self.raw.size]
        assert self.buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == off % 16
        self.view = view.view(*x.shape, 3) if s24 else view.view(TORCH[x.dtype.type]).view(x.shape)

    def result(self):
        """The file after the call; the bands are checked to hold the fill."""
        host = self.buf.cpu().numpy()
        assert np.all(host[:self.lead] == self.fill) and np.all(host[self.lead + self.raw.size:] == self.fill), "a byte outside x was written"
        return _unraw(host[self.lead:self.lead + self.raw.size].copy(), self.x)


def _call(ctx, x, runs, max_len, p, K, channel=None, off=0, fill=0xFF):
    """One si_mend_runs call -> (y, status) on the host, with guard bands around x (Placed) and around status (tests/extent.py)."""
    pl = Placed(x, ctx.device, off, fill)
    table = torch.tensor(np.asarray(runs, dtype=np.int32).reshape(-1, 2), device=ctx.device)
    keep = extent.unchanged({"runs": table})
    with extent.guarded_allocs(fill, band=4096) as rec:
        status = ctx.mend_runs(pl.view, table, max_len, p, K, channel=channel)
    torch.cuda.synchronize()
    rec.check()
    keep.check()
    return pl.result(), status.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ the comparison
def _hold_condition(name, ref, exact):
    """The condition on a case, asserted on the CPU side: a well-posed fit, and a float64 reference that is its own exact value."""
    assert ref.status.tolist() == exact.status.tolist(), name
    for i, (u, ux, ratio, P) in enumerate(zip(ref.u, exact.u, ref.ratio, ref.peak)):
        if u is None:
            continue
        assert (ratio is not None and ratio > 1e-6) or P == 0.0, (name, i, ratio, P)
        gap = max(abs(float(a) - float(b)) for a, b in zip(u, ux))
        assert gap < 2.0 ** -34 * P or (P == 0.0 and gap == 0.0), (name, i, gap, 2.0 ** -34 * P)


def _compare(name, x, runs, ref, y, status, channel=None, quiet=False):
    dtype = x.dtype.type
    assert status.tolist() == ref.status.tolist(), (name, [M.NAMES[s] for s in status], [M.NAMES[s] for s in ref.status])
    col = (lambda a: a) if x.ndim == 1 else (lambda a: a[:, channel])
    untouched = np.ones(x.shape, bool)
    checked = odd = 0
    for (s, m), st, u, P in zip(runs, ref.status, ref.u, ref.peak):
        if st not in FILLED:
            continue
        col(untouched)[s:s + m] = False
        got, want = col(y)[s:s + m], np.array([float(v) for v in u])
        if dtype is np.float32:
            bound = 2.0 ** -23 * np.maximum(P, np.abs(want))
            err = np.abs(got.astype(np.float64) - want)
            worst = float(np.max(err / np.where(bound > 0, bound, 1.0))) if np.any(bound > 0) else 0.0
            if not quiet:
                print(f"   {name} row ({s}, {m}): fp32 err / bound {worst:.4f}")
            WORST["fp32"] = max(WORST.get("fp32", 0.0), worst)
            assert np.all(err <= bound), (name, s, m, float(np.max(err)), float(np.min(bound)))
        else:
            stored = np.array([int(M.store(float(v), dtype)) for v in want])
            diff = got.astype(np.int64) - stored
            tie = np.abs(np.abs(want - np.floor(want)) - 0.5) <= 2.0 ** -30 * P
            assert np.all((diff == 0) | (tie & (np.abs(diff) == 1))), (name, s, m, diff.tolist(), want.tolist())
            odd += int(np.count_nonzero(diff))
            key = "int16" if dtype is np.int16 else "s24"
            WORST[key] = WORST.get(key, 0) + int(np.count_nonzero(diff))
        checked += m
    assert odd * 100 <= checked, (name, odd, checked)
    keep = np.repeat(untouched.reshape(-1), 3 if dtype is M.S24 else x.itemsize)
    assert np.array_equal(_raw(y)[keep], _raw(x)[keep]), (name, "a sample outside the filled runs changed")
    return checked


@functools.lru_cache(maxsize=None)
def _case(dtype, p, K, lens, seed, ch=None, channel=None):
    """A file with one run per entry of `lens`, each exactly K + 2 samples clear of the next, NaN (fp32) or full scale (PCM) in the damaged
    samples -> (name, x, runs, float64 reference, exact reference); references are computed once and shared."""
    gap = K + 2
    n = K + 1 + sum(m + gap for m in lens) + K - gap + 3
    cols = []
    for c in range(ch or 1):
        sig = (M.voiced if (seed + c) % 2 == 0 else M.ar2)(n, seed + 7 * c)
        cols.append(M.as_type(sig, dtype))
    x = cols[0] if ch is None else np.stack(cols, axis=1)
    runs, s = [], K + 1
    for m in lens:
        runs.append((s, m))
        target = x if ch is None else x[:, channel]
        target[s:s + m] = np.nan if dtype is np.float32 else M.RANGE[dtype][1]
        s += m + gap
    name = f"{np.dtype(dtype).name} p={p} K={K} seed={seed}" + ("" if ch is None else f" ch={ch}/{channel}")
    ref = M.mend(x, runs, 64, p, K, channel=channel)
    exact = M.mend(x, runs, 64, p, K, channel=channel, exact=True)
    _hold_condition(name, ref, exact)
    return name, x, runs, ref, exact


# ------------------------------------------------------------------------------------------------------------ 1: shapes
@pytest.mark.parametrize("p,K", [(2, 8), (8, 32), (32, 128)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_run_length_against_the_reference(dtype, p, K):
    """m in {1, 2, 3, 16, 63, 64} filled, 65 LONG, in one table."""
    ctx = _ctx()
    name, x, runs, ref, _ = _case(dtype, p, K, LENS, 10 + p + (p == 8))
    assert ref.status.tolist() == [M.AR] * 6 + [M.LONG]
    y, status = _call(ctx, x, runs, 64, p, K)
    assert _compare(name, x, runs, ref, y, status) == sum(LENS[:-1])


@pytest.mark.parametrize("dtype,K,lens", [(np.float32, 512, (1, 16, 64)), (np.int16, 512, (3, 64)), (np.float32, 1024, (2, 63)), (M.S24, 1024, (64,))],
                         ids=["fp32-512", "int16-512", "fp32-1024", "s24-1024"])
def test_the_long_contexts(dtype, K, lens):
    ctx = _ctx()
    name, x, runs, ref, _ = _case(dtype, 32, K, lens, 5)
    y, status = _call(ctx, x, runs, 64, 32, K)
    assert ref.status.tolist() == [M.AR] * len(lens) and _compare(name, x, runs, ref, y, status) == sum(lens)


def test_an_s24_view_at_every_byte_offset():
    ctx = _ctx()
    name, x, runs, ref, _ = _case(M.S24, 8, 32, (1, 3, 16), 21)
    first = None
    for off in range(8):
        y, status = _call(ctx, x, runs, 64, 8, 32, off=off)
        _compare(f"{name} off={off}", x, runs, ref, y, status)
        first = first if first is not None else y
        assert np.array_equal(y, first), off
    for dtype, offs in ((np.float32, (4, 8, 12)), (np.int16, (2, 6, 14))):
        name, x, runs, ref, _ = _case(dtype, 8, 32, (1, 3, 16), 21)
        for off in offs:
            y, status = _call(ctx, x, runs, 64, 8, 32, off=off)
            _compare(f"{name} off={off}", x, runs, ref, y, status)


@pytest.mark.parametrize("ch", [2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_channel_of_an_interleaved_file(dtype, ch):
    """Channel first and last: the samples of the mono call on the de-interleaved channel, and no other channel touched."""
    ctx = _ctx()
    for channel in (0, ch - 1):
        name, x, runs, ref, _ = _case(dtype, 8, 32, (1, 2, 16), 30 + ch, ch, channel)
        y, status = _call(ctx, x, runs, 64, 8, 32, channel=channel)
        _compare(name, x, runs, ref, y, status, channel)
        mono, mstatus = _call(ctx, np.ascontiguousarray(x[:, channel]), runs, 64, 8, 32)
        assert np.array_equal(mstatus, status) and _raw(np.ascontiguousarray(y[:, channel])).tobytes() == _raw(mono).tobytes()
    one, ostatus = _call(ctx, np.ascontiguousarray(x[:, channel]).reshape(-1, 1), runs, 64, 8, 32, channel=0)      # channels = 1 is the mono call
    assert np.array_equal(ostatus, status) and _raw(one.reshape(-1)).tobytes() == _raw(mono).tobytes()


# ------------------------------------------------------------------------------------------------------------ 2: status boundaries
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_status_boundaries(dtype):
    ctx = _ctx()
    p, K, n = 2, 8, 96
    x = M.as_type(M.voiced(n, 3), dtype)

    def both(runs, max_len=4, file=x):
        ref = M.mend(file, runs, max_len, p, K)
        _hold_condition(str(runs), ref, M.mend(file, runs, max_len, p, K, exact=True))
        y, status = _call(ctx, file, runs, max_len, p, K)
        _compare(f"{np.dtype(dtype).name} {runs}", file, runs, ref, y, status)
        return status.tolist()

    assert both([(8, 2)]) == [M.AR] and both([(7, 2)]) == [M.EDGE]                                 # s - K = 0 against -1
    assert both([(n - 10, 2)]) == [M.AR] and both([(n - 9, 2)]) == [M.EDGE]                        # e + K = n against n + 1
    assert both([(20, 4)]) == [M.AR] and both([(20, 5)]) == [M.LONG]
    assert both([(10, 2), (20, 2)]) == [M.AR, M.AR]                                                # a neighbour at distance exactly K is filled
    assert both([(10, 2), (19, 2)]) == [M.NEAR, M.NEAR]                                            # at K - 1 both rows are NEAR
    assert both([(10, 2), (19, 30), (60, 3)]) == [M.NEAR, M.LONG, M.AR]
    assert both([(-1, 2), (20, 0), (40, 2), (n - 1, 2), (n - 2, 2)]) == [M.BADROW, M.BADROW, M.AR, M.BADROW, M.EDGE]    # a bad row is written as 6
    zero = np.zeros(40, dtype)
    zero[16:19] = 5
    assert both([(16, 3)], file=zero) == [M.LINE]                                                 # an all-zero context: the line
    if dtype is np.float32:
        for where, runs, want in ((12, [(20, 2)], M.NONFINITE), (12, [(21, 2)], M.AR), (30, [(20, 3)], M.NONFINITE), (30, [(20, 2)], M.AR)):
            y = x.copy()                                                # a NaN at s - K against s - K - 1, an inf at e + K - 1 against e + K
            y[where] = np.nan if where == 12 else np.inf
            assert both(runs, file=y) == [want], (where, runs)
        # a NaN planted outside the input (Placed's 0xFF bands are NaN words) is never read: rows that reach the file's first and last sample
        assert both([(8, 1), (n - 9, 1)]) == [M.AR, M.AR]


# ------------------------------------------------------------------------------------------------------------ 3: invariants
def test_a_row_alone_equals_the_row_in_a_table_and_calls_repeat():
    ctx = _ctx()
    for dtype in DTYPES:
        name, x, runs, ref, _ = _case(dtype, 8, 32, LENS, 18)
        results = [_call(ctx, x, runs, 64, 8, 32, fill=fill) for fill in extent.FILLS + extent.FILLS[:1]]
        for y, status in results[1:]:
            assert _raw(y).tobytes() == _raw(results[0][0]).tobytes() and np.array_equal(status, results[0][1])
        table = results[0][0]
        for i, (s, m) in enumerate(runs):
            y, status = _call(ctx, x, [(s, m)], 64, 8, 32)
            assert status.tolist() == [int(results[0][1][i])] and _raw(y[s:s + m]).tobytes() == _raw(table[s:s + m]).tobytes(), (name, s, m)
            keep = np.ones(len(x), bool)
            keep[s:s + m] = False
            assert _raw(y[keep]).tobytes() == _raw(x[keep]).tobytes()
        fresh = _fresh_ctx()
        try:
            y, status = _call(fresh, x, runs, 64, 8, 32)
        finally:
            fresh.close()
        assert _raw(y).tobytes() == _raw(table).tobytes() and np.array_equal(status, results[0][1])


def test_five_thousand_one_sample_rows():
    """(p, K) = (2, 8), the rows exactly K apart: every workgroup's context ends where its neighbours' runs begin."""
    ctx = _ctx()
    R, K = 5000, 8
    n = K + 9 * R + K
    x = M.as_type(M.voiced(n, 8, noise=0.05), f32)
    runs = [(K + 9 * i, 1) for i in range(R)]
    for s, _ in runs:
        x[s] = np.nan
    ref = M.mend(x, runs, 1, 2, K)
    _hold_condition("5000 rows", ref, M.mend(x, runs, 1, 2, K, exact=True))
    assert ref.status.tolist() == [M.AR] * R
    y, status = _call(ctx, x, runs, 1, 2, K)
    assert _compare("5000 rows", x, runs, ref, y, status, quiet=True) == R and np.all(np.isfinite(y))


def test_refusals_and_an_empty_table_launch_nothing():
    ctx = _ctx()
    dev = ctx.device
    x = torch.full((256,), 7.0, device=dev)
    runs = torch.tensor([[100, 2]], dtype=torch.int32, device=dev)
    status = torch.full((4,), -7, dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(x_=x, fmt=0, n=256, channels=1, channel=0, runs_=runs, n_runs=1, max_len=64, order=8, context=32, status_=status):
        ctx.profile_start(100)
        rc = ctx.lib.si_mend_runs(ctx._h, P(x_), fmt, n, channels, channel, P(runs_), n_runs, max_len, order, context, P(status_), ctx._stream())
        msg = ctx.lib.si_last_error(ctx._h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        torch.cuda.synchronize()
        return rc, msg, launched

    for kw, text in ((dict(max_len=0), "max_len = 0"), (dict(max_len=65), "max_len = 65"), (dict(order=1), "order = 1"), (dict(order=33), "order = 33"),
                     (dict(context=31), "context = 31"), (dict(context=1025, order=32), "context = 1025"), (dict(n_runs=65537), "n_runs = 65537"),
                     (dict(n_runs=-1), "n_runs = -1"), (dict(channels=9), "channels = 9"), (dict(channels=2, channel=2), "channel = 2"),
                     (dict(channel=-1), "channel = -1"), (dict(x_=None), "x is NULL"), (dict(runs_=None), "runs is NULL"),
                     (dict(status_=None), "status is NULL"), (dict(n=0), "n = 0")):
        rc, msg, launched = call(**kw)
        assert rc != 0 and msg.startswith("si_mend_runs: ") and text in msg and launched == [], (kw, rc, msg, launched)
    rc, msg, launched = call(n_runs=0)
    assert rc == 0 and launched == []
    assert bool((x == 7.0).all()) and bool((status == -7).all())
    rc, msg, launched = call()                                          # and the call itself: one launch in the family patch_rate
    assert rc == 0 and [(e["name"], e["launches"]) for e in launched] == [("patch_rate", 1)]
    ref = M.mend(np.full(256, 7.0, f32), [(100, 2)], 64, 8, 32)          # a constant context, through the model
    got = x.cpu().numpy()
    assert status.tolist() == [int(ref.status[0]), -7, -7, -7] and bool((x[:100] == 7.0).all()) and bool((x[102:] == 7.0).all())
    assert np.all(np.abs(got[100:102].astype(np.float64) - np.array(ref.u[0])) <= 2.0 ** -23 * 7.0)


def test_zz_the_worst_ratios():
    """Printed for DESIGN.md 4.31: the worst |gpu - ref| / bound over the fp32 checks of this file, and the PCM samples that took the
    half-integer exception."""
    print("   SUMMARY mend_runs:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in sorted(WORST.items())})
    assert WORST.get("fp32", 0.0) <= 1.0
