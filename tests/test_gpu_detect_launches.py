"""What the detection launcher does per route, in one place: for each of the seven run-list entry points and
si_impulse_residual, on one file of 2 * 2048 + 5 sample times in four layouts -- (n,), (n, 1) with channel 0, (n, 2) with channel 1 and
(n, 2) joint -- in fp32, and once each in int16 and packed 24-bit on (n,):
    the rows, the count and T equal the float64 references' (tests/detect_ref.py, channels_ref.py, dead_ref.py, level_ref.py, burst_ref.py,
        invalid_ref.py, impulse_ref.py), exactly; the file is rebuilt from another seed until no windowed decision is within an
        addition order of its limit (the references' own conditions), so nothing depends on the order of the device's sums;
    the profile is exactly the route's families, one launch each: detect_peak and detect_peak_final only with rel_threshold > 0,
        detect_emit only with max_runs > 0, no other name;
    each family's bytes equal the launcher's traffic model, written out here from n, the channel count, the element size and
        chunks = ceil(n / 2048).
The file: low-level noise with a held stretch, two stretches of zeros (one across the seam of chunks 0 | 1), three clicks, full-scale garbage (one block across the seam of chunks 1 | 2 that ends on the last sample) and, in fp32, a
NaN and an inf.
The refusals: for each entry point and each pair of consecutive refusals in its order, one call wrong in both is refused with the
EARLIER one's text, and launches nothing."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import burst_ref as B
from tests import channels_ref as CH
from tests import dead_ref as R
from tests import detect_ref as D
from tests import impulse_ref as I
from tests import invalid_ref as V
from tests import level_ref as L
from tests import s24_ref as S

pytestmark = pytest.mark.gpu

N = 2 * 2048 + 5
S24 = I.S24
FULL = I.FULL
ESZ = {np.float32: 4, np.int16: 2, S24: 3}
TORCH = {np.float32: torch.float32, np.int16: torch.int16}
SENTINEL = -7
MIN_LEN = 3
HALF = 7                                                # level and burst
IMP = dict(order=8, half=64, guard=8, pad=2, ratio=10.0)
REL = {"dead": 0.25, "level": 0.25, "burst": 0.5, "impulse": 0.25}
ROUTES = ("quiet", "dead", "level", "burst", "invalid", "impulse")
LAYOUTS = {"mono": (1, None), "one": (1, 0), "two": (2, 1), "joint": (2, -1)}       # name -> (columns of the file, channel)
_FILES = {}


# ------------------------------------------------------------------------------------------------------------ the file
def _column(dtype, seed, shift):
    """One channel: noise of 0.002 .. 0.01 of full scale, never zero, and the defects; `shift` moves the stretches that joint detection
    intersects."""
    rng = np.random.default_rng(seed)
    fs = FULL[dtype]
    x = rng.uniform(0.002, 0.01, N) * rng.choice([-1.0, 1.0], N)
    x[300 + shift:330 + shift] = 0.004                                 # held
    x[2040 + shift:2060 + shift] = 0.0                                 # zeros across the seam of chunks 0 | 1
    x[2900 + shift:3100 + shift] = 0.0                                 # zeros, longer than the level window
    for a, b in ((1200 + shift, 1240 + shift), (4085, N)):             # garbage above 0.96 of full scale; the second block ends with the file
        x[a:b] = rng.uniform(0.96, 0.999, b - a) * rng.choice([-1.0, 1.0], b - a)
    for t in (700, 2030, 3500):                                        # clicks
        x[t] = 0.9
    if dtype is np.float32:
        x = x.astype(np.float32)
        x[3700], x[3701] = np.nan, np.inf
        return x
    return np.rint(x * fs).astype(dtype)


def _thr(route, dtype):
    return float(np.float32({"quiet": 2.0 ** -10, "dead": 2.0 ** -10, "level": 2.0 ** -10, "burst": 0.25, "impulse": 0.0}[route] * FULL[dtype]))


def _ceiling(dtype):
    return float(np.float32(0.95 * FULL[dtype]))


def _expected(x, route, channel, rel):
    """(rows, T or None) of one call from the float64 reference; the windowed references' own conditions asserted."""
    dtype = x.dtype.type
    if route == "quiet":
        thr = _thr(route, dtype)
        if x.ndim == 1:
            return D.quiet_runs_ref(x, thr, MIN_LEN), None
        return (CH.joint_runs_ref(x, thr, MIN_LEN) if channel < 0 else D.quiet_runs_ref(x[:, channel], thr, MIN_LEN)), None
    if route == "invalid":
        return V.invalid_runs_ref(x, _ceiling(dtype), MIN_LEN, channel), None
    thr = _thr(route, dtype)
    if route == "dead":
        return R.dead_runs_ref(x, R.ANY, thr, rel, 0.0, MIN_LEN, channel), R.threshold_ref(x, thr, rel, channel)
    if route in ("level", "burst"):
        undecided = []
        mask = (L.level_mask if route == "level" else B.burst_mask)(x, HALF, thr, rel, channel, report=undecided)
        assert not undecided, (route, undecided[:4])
        return R.runs_of(mask, MIN_LEN), R.threshold_ref(x, thr, rel, channel)
    rows, T, _ = I.check(I.Case("launches", x, dict(IMP, thr=thr, rel=rel, channel=channel, min_len=MIN_LEN)))
    return rows, T


def _files():
    """{(dtype, columns): host array} and {(dtype, layout, route, rel): (rows, T)}, from the first seed at which every reference decides."""
    if _FILES:
        return _FILES["x"], _FILES["want"]
    for seed in range(8):
        x = {(np.float32, 1): _column(np.float32, 10 * seed, 0), (np.int16, 1): _column(np.int16, 10 * seed + 1, 0),
             (S24, 1): _column(S24, 10 * seed + 2, 0),
             (np.float32, 2): np.stack([_column(np.float32, 10 * seed + 3, 0), _column(np.float32, 10 * seed + 4, 5)], axis=1)}
        want = {}
        try:
            for dtype, layout in _cases():
                cols, channel = LAYOUTS[layout]
                file = x[(dtype, cols)]
                file = file.reshape(N, 1) if layout == "one" else file
                for route in ROUTES:
                    for rel in ((0.0, REL[route]) if route in REL else (0.0,)):
                        want[(dtype, layout, route, rel)] = _expected(file, route, channel, rel)
        except AssertionError:
            continue
        _FILES["x"], _FILES["want"] = x, want
        return x, want
    raise AssertionError("no seed of 0 .. 7 gives a file that every reference decides")


def _cases():
    return [(np.float32, k) for k in LAYOUTS] + [(np.int16, "mono"), (S24, "mono")]


def _on_device(x, layout, dev):
    """The host file as the call takes it: (n,), (n, 1) or (n, 2); packed 24-bit with its trailing 3 bytes."""
    x = x.reshape(N, 1) if layout == "one" else x
    return torch.from_numpy(S.pack(x) if x.dtype == np.int32 else np.ascontiguousarray(x)).to(dev)


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from tests.harness import build_engine
    return build_engine(HubertArch.tiny(), VocoderArch.tiny(), 100, key=("test_gpu_detect_launches",))


def _profiled(ctx, call):
    """call() -> (its result, {family: (launches, bytes)} of the families that launched)."""
    ctx.profile_start(100)
    try:
        out = call()
    finally:
        prof = {q["name"]: (q["launches"], q["bytes"]) for q in ctx.profile_stop() if q["launches"] > 0}
    return out, prof


# ------------------------------------------------------------------------------------------------------------ the traffic model
def _traffic(route, entry_channels, esz, rel, max_runs):
    """{family: (1, bytes)} of one call as the launcher counts them.  entry_channels: what the C entry point is handed -- None for
    si_quiet_runs, which has no channels."""
    chunks = -(-N // 2048)
    bits, sums = chunks * 256.0, chunks * 4.0
    want = {}
    if route == "quiet":
        ch = entry_channels                                            # si_quiet_runs_ch keeps channels = 1 interleaved
        want["detect_bits" if ch is None else "detect_bits_ch"] = float(N) * (ch or 1) * esz + bits + 2.0 * sums
    else:
        ch = entry_channels if entry_channels >= 2 else 0              # the descriptor routes: channels = 1 is the one-channel file
        samples = float(N) * (ch or 1) * esz
        if route in REL and rel > 0:
            want["detect_peak"] = samples + sums
            want["detect_peak_final"] = sums + 8.0
        family = "detect_dead" if route != "invalid" else "detect_bits" if ch == 0 else "detect_bits_ch"
        want[family] = samples + bits + 2.0 * sums
    want["detect_carry"] = 3.0 * sums
    want["detect_count"] = bits + 3.0 * sums
    want["detect_offsets"] = 2.0 * sums
    if max_runs > 0:
        want["detect_emit"] = bits + 3.0 * sums
    return {k: (1, v) for k, v in want.items()}


def _call(ctx, route, x, channel, rel, max_runs, runs, cnt, T):
    dtype = S24 if x.dtype == torch.uint8 else {torch.float32: np.float32, torch.int16: np.int16}[x.dtype]
    kw = dict(min_len=MIN_LEN, max_runs=max_runs, runs=runs if max_runs > 0 else None, n_runs=cnt, channel=channel)
    if route == "quiet":
        return ctx.quiet_runs(x, _thr(route, dtype), **kw)
    if route == "invalid":
        return ctx.invalid_runs(x, _ceiling(dtype), **kw)
    kw.update(threshold=_thr(route, dtype), rel_threshold=rel, threshold_out=T)
    if route == "dead":
        return ctx.dead_runs(x, R.ANY, held_tol=0.0, **kw)
    if route == "level":
        return ctx.level_runs(x, HALF, **kw)
    if route == "burst":
        return ctx.burst_runs(x, HALF, **kw)
    return ctx.impulse_runs(x, **IMP, **kw)


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("route", ROUTES)
def test_rows_profile_and_bytes_of_every_route(route):
    ctx = _engine().ctx
    files, wants = _files()
    seam = last = False
    for dtype, layout in _cases():
        cols, channel = LAYOUTS[layout]
        x = _on_device(files[(dtype, cols)], layout, ctx.device)
        for rel in ((0.0, REL[route]) if route in REL else (0.0,)):
            rows_ref, T_ref = wants[(dtype, layout, route, rel)]
            for max_runs in (0, 8):
                what = (route, np.dtype(dtype).name, layout, rel, max_runs)
                runs = torch.full((12, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
                cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=ctx.device)
                T = torch.full((1,), -1.0, dtype=torch.float32, device=ctx.device)
                _, prof = _profiled(ctx, lambda: _call(ctx, route, x, channel, rel, max_runs, runs, cnt, T))
                got = runs.cpu().numpy()
                k = min(len(rows_ref), max_runs)
                assert int(cnt.item()) == len(rows_ref), (what, int(cnt.item()), len(rows_ref), got[:6].tolist(), rows_ref[:6].tolist())
                assert np.array_equal(got[:k], rows_ref[:k]) and np.all(got[k:] == SENTINEL), (what, got.tolist(), rows_ref[:8].tolist())
                if T_ref is None:
                    assert float(T.item()) == -1.0, what
                else:
                    assert T.cpu().numpy()[0].tobytes() == np.float32(T_ref).tobytes(), (what, float(T.item()), T_ref)
                entry = None if (route == "quiet" and channel is None) else (cols if channel is not None else 1)
                assert prof == _traffic(route, entry, ESZ[dtype], rel, max_runs), (what, prof)
            assert len(rows_ref) > 0 or rel > 0, (route, layout)
            seam |= any(a < c0 < a + m for a, m in rows_ref.tolist() for c0 in (2048, 4096))
            last |= any(a + m == N for a, m in rows_ref.tolist())
    # the two seams go to the zeros and to the garbage, so a click has none: its runs are held to the reference's all the same
    assert (seam or route == "impulse") and (last or route not in ("burst", "invalid")), (route, seam, last)


def test_the_residual_tap_of_every_layout():
    """si_impulse_residual on (n,), (n, 1) channel 0 and (n, 2) channel 1, and int16 and packed 24-bit once: tests/test_gpu_impulse.py's
    bound |e - ref| <= C_DEVICE * A(t) (NaN where the reference has NaN), one launch in detect_dead, n samples in and n float64 out."""
    ctx = _engine().ctx
    files, _ = _files()
    for dtype, layout in _cases():
        cols, channel = LAYOUTS[layout]
        if channel == -1:
            continue
        host = files[(dtype, cols)].reshape(N, 1) if layout == "one" else files[(dtype, cols)]
        x = _on_device(files[(dtype, cols)], layout, ctx.device)
        e, prof = _profiled(ctx, lambda: ctx.impulse_residual(x, IMP["order"], channel=channel))
        ref = I.residual_ref(host, IMP["order"], channel=channel)
        e = e.cpu().numpy()
        assert e.shape == (N,) and np.array_equal(np.isnan(e), np.isnan(ref.e)), (dtype, layout)
        ok = ~np.isnan(ref.e)
        assert np.all(np.abs(e[ok] - ref.e[ok]) <= I.C_DEVICE * ref.A[ok]), (dtype, layout)
        assert prof == {"detect_dead": (1, float(N) * cols * ESZ[dtype] + float(N) * 8.0)}, (dtype, layout, prof)


def test_the_engine_finds_the_same_rows():
    """InpaintingEngine.find_*_runs on the same files: rows and T.  An (n, 1) file is flattened there, so its quiet and invalid routes are
    the one-channel kernels'; the (n, 2) layouts keep the interleaved ones."""
    from tests.harness import tapped_run
    eng = _engine()
    files, wants = _files()
    for dtype, layout in _cases():
        cols, channel = LAYOUTS[layout]
        x = _on_device(files[(dtype, cols)], layout, eng.device)
        thr = {r: _thr(r, dtype) for r in ROUTES if r != "invalid"}
        calls = {"quiet": lambda: (eng.find_quiet_runs(x, thr["quiet"], MIN_LEN, channel=channel), None),
                 "dead": lambda: eng.find_dead_runs(x, "any", thr["dead"], REL["dead"], 0.0, MIN_LEN, channel=channel, return_threshold=True),
                 "level": lambda: eng.find_level_runs(x, half=HALF, threshold=thr["level"], rel_threshold=REL["level"], min_len=MIN_LEN, channel=channel,
                                                      return_threshold=True),
                 "burst": lambda: eng.find_burst_runs(x, win=2 * HALF + 1, threshold=thr["burst"], rel_threshold=REL["burst"], min_len=MIN_LEN,
                                                      channel=channel, return_threshold=True),
                 "invalid": lambda: (eng.find_invalid_runs(x, _ceiling(dtype), MIN_LEN, channel=channel), None),
                 "impulse": lambda: eng.find_impulse_runs(x, half=IMP["half"], order=IMP["order"], guard=IMP["guard"], pad=IMP["pad"], ratio=IMP["ratio"],
                                                          threshold=thr["impulse"], rel_threshold=REL["impulse"], min_len=MIN_LEN, channel=channel,
                                                          return_threshold=True)}
        for route in ROUTES:
            rows_ref, T_ref = wants[(dtype, layout, route, REL.get(route, 0.0))]
            _, (rows, T), prof = tapped_run(eng.ctx, {}, calls[route])
            assert rows.dtype == torch.int32 and rows.is_cuda and rows.cpu().numpy().tolist() == rows_ref.tolist(), (route, dtype, layout)
            assert T_ref is None or np.float32(T).tobytes() == np.float32(T_ref).tobytes(), (route, dtype, layout, T, T_ref)
            entry = None if (route == "quiet" and cols == 1) else cols
            assert prof == {k: v[0] for k, v in _traffic(route, entry, ESZ[dtype], REL.get(route, 0.0), 1).items()}, (route, dtype, layout, prof)
    x = _on_device(files[(np.float32, 1)], "mono", eng.device)           # the overflow names both numbers, and the route's noun
    for noun, call in (("quiet", lambda: eng.find_quiet_runs(x, _thr("quiet", np.float32), 1, max_runs=1)),
                       ("dead", lambda: eng.find_dead_runs(x, "any", _thr("dead", np.float32), min_len=1, max_runs=1)),
                       ("invalid", lambda: eng.find_invalid_runs(x, _ceiling(np.float32), 1, max_runs=1))):
        with pytest.raises(ValueError, match=f"find_{noun}_runs: [0-9]+ runs of at least 1 {noun} samples, more than max_runs = 1"):
            call()


# ------------------------------------------------------------------------------------------------------------ 2
NAN, INF = float("nan"), float("inf")
HEAD = [(dict(channels=9), "channels = 9, outside 1 .. SI_MAX_CHANNELS = 8"), (dict(x=None), "x is NULL"), (dict(cnt=None), "n_runs is NULL"),
        (dict(max_runs=-1), "max_runs = -1 is negative"), (dict(runs=None), "runs is NULL with max_runs = 8"), (dict(n=0), "n = 0 samples, outside 1 .. "),
        (dict(thr=-1.0), "threshold = -1 is negative or NaN"), (dict(min_len=0), "min_len = 0 samples, at least 1")]
ORDER = {
    "si_quiet_runs": HEAD[1:],
    "si_quiet_runs_ch": HEAD,
    "si_dead_runs": HEAD + [(dict(kind=4), "kind = 4, outside 1 .. 3"), (dict(rel=1.5), r"rel_threshold = 1.5 is NaN or outside \[0, 1\]"),
                            (dict(tol=-1.0), "held_tol = -1 is negative or NaN")],
    "si_level_runs": HEAD + [(dict(half=1025), "half = 1025 samples, outside 0 .. SI_LEVEL_MAX_HALF = 1024"), (dict(thr=INF), "threshold = inf is not finite"),
                             (dict(rel=1.5), r"rel_threshold = 1.5 is NaN or outside \[0, 1\]")],
    "si_burst_runs": HEAD + [(dict(half=-1), "half = -1 samples, outside 0 .. SI_LEVEL_MAX_HALF = 1024"), (dict(thr=INF), "threshold = inf is not finite"),
                             (dict(rel=4.5), r"rel_threshold = 4.5 is NaN or outside \[0, 4\]")],
    "si_invalid_runs": HEAD[:6] + HEAD[7:] + [(dict(ceiling=0.0), "ceiling = 0 is not above 0, or is NaN")],
    "si_impulse_runs": HEAD + [(dict(order=1), "order = 1, outside 2 .. SI_IMPULSE_MAX_ORDER = 32"),
                               (dict(guard=65), "guard = 65 samples, outside 0 .. SI_IMPULSE_MAX_GUARD = 64"),
                               (dict(half=1025), r"half = 1025 samples, outside guard \+ 1 = [0-9]+ .. SI_IMPULSE_MAX_HALF = 1024"),
                               (dict(pad=17), "pad = 17 samples, outside 0 .. SI_IMPULSE_MAX_PAD = 16"),
                               (dict(half=1023, pad=2), r"half \+ pad = 1025 samples, above SI_IMPULSE_MAX_HALF = 1024"),
                               (dict(ratio=0.5), r"ratio = 0.5 is NaN or outside \[1, 1e6\]"), (dict(thr=INF), "threshold = inf is not finite"),
                               (dict(rel=4.5), r"rel_threshold = 4.5 is NaN or outside \[0, 4\]")],
    "si_impulse_residual": [HEAD[0], HEAD[1], (dict(e=None), "e is NULL"), HEAD[5], (dict(order=33), "order = 33, outside 2 .. SI_IMPULSE_MAX_ORDER = 32")],
}


def test_the_earlier_refusal_wins():
    """One call wrong in two consecutive places of the entry point's order: SI_EINVAL, the earlier text, nothing launched, nothing
    written.  (max_runs cannot be negative and positive at once: that pair is runs = NULL at max_runs = -1.)"""
    ctx = _engine().ctx
    lib, h, dev = ctx.lib, ctx._h, ctx.device
    x = torch.zeros(4096 * 2, device=dev)
    runs = torch.full((8, 2), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    T = torch.full((1,), -1.0, dtype=torch.float32, device=dev)
    e = torch.full((4096,), -3.0, dtype=torch.float64, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    good = dict(x=x, n=4096, channels=2, channel=0, thr=0.0, rel=0.5, min_len=1, runs=runs, max_runs=8, cnt=cnt, kind=3, tol=0.0, half=16, ceiling=1.0,
                order=16, guard=4, pad=2, ratio=10.0, e=e)
    tail = lambda a: (a["min_len"], P(a["runs"]), a["max_runs"], P(a["cnt"]))
    file = lambda a: (h, P(a["x"]), 0, a["n"], a["channels"], a["channel"])
    entry = {
        "si_quiet_runs": lambda a: lib.si_quiet_runs(h, P(a["x"]), 0, a["n"], a["thr"], *tail(a), st),
        "si_quiet_runs_ch": lambda a: lib.si_quiet_runs_ch(*file(a), a["thr"], *tail(a), st),
        "si_dead_runs": lambda a: lib.si_dead_runs(*file(a), a["kind"], a["thr"], a["rel"], a["tol"], *tail(a), P(T), st),
        "si_level_runs": lambda a: lib.si_level_runs(*file(a), a["half"], a["thr"], a["rel"], *tail(a), P(T), st),
        "si_burst_runs": lambda a: lib.si_burst_runs(*file(a), a["half"], a["thr"], a["rel"], *tail(a), P(T), st),
        "si_invalid_runs": lambda a: lib.si_invalid_runs(*file(a), a["ceiling"], *tail(a), st),
        "si_impulse_runs": lambda a: lib.si_impulse_runs(*file(a), a["order"], a["half"], a["guard"], a["pad"], a["ratio"], a["thr"], a["rel"], *tail(a), P(T), st),
        "si_impulse_residual": lambda a: lib.si_impulse_residual(*file(a), a["order"], P(a["e"]), st),
    }
    pairs = 0
    for fn, order in ORDER.items():
        for (first, msg), (second, _) in zip(order, order[1:]):
            args = {**good, **second, **first}
            (rc, prof) = _profiled(ctx, lambda: entry[fn](args))
            err = lib.si_last_error(h).decode()
            assert rc == -1 and prof == {}, (fn, first, second, rc, prof)
            assert re.search(re.escape(fn) + ": " + msg, err), (fn, first, second, err)
            pairs += 1
        torch.cuda.synchronize()
        assert bool((runs == SENTINEL).all()) and int(cnt.item()) == SENTINEL and float(T.item()) == -1.0 and bool((e == -3.0).all()), fn
        assert entry[fn](good) == 0, (fn, lib.si_last_error(h).decode())      # the same arguments, none of them wrong, are served
        torch.cuda.synchronize()
        runs.fill_(SENTINEL), cnt.fill_(SENTINEL), T.fill_(-1.0), e.fill_(-3.0)
    assert pairs == 6 + 7 + 3 * 10 + 7 + 15 + 4
