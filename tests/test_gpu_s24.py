"""Packed 24-bit PCM at the kernels, through `native`: detection, both cutters and the patch on uint8 (n, [ch,] 3)
views.  No tolerance of its own (tests/s24_ref.py): detection rows equal the existing references' rows on the fp32 image F = V 2^-23,
the cutters give the bytes of the fp32 call on F and stay inside feed_ref / pair_ref's bounds as the fp32 tests state them, and a
patched sample is the store rule applied to the fp32 the fp32 call writes for F -- and lies, independently, in
[trunc((ref - E) 2^23), trunc((ref + E) 2^23)] with ref and E from rate_ref.blend(F, ...)."""
import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import dead_ref as R
from tests import detect_ref as D
from tests import feed_ref as F
from tests import pair_ref as PR
from tests import rate_ref as RR
from tests import s24_ref as S
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

SENTINEL = -7
_CACHE = {}


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", "fp32", key=("patch", "fp32"))


def _cases(name):
    if name not in _CACHE:
        _CACHE[name] = getattr(S, name)()
    return _CACHE[name]


def _view(v, dev, off=0, before=None, after=None, front=0x7F, back=0x80):
    """The 24-bit file v (int32 (n,) or (n, ch)) as a device uint8 view (n, [ch,] 3) whose first byte lies `off` bytes past a 16-byte
    boundary.  The bytes in front of it are `before`'s samples (else `front`) and those behind it `after`'s (else `back`), 48 of each at
    the least.  -> (view, the whole buffer, the view's first byte in it)."""
    v = np.asarray(v)
    body = S.pack(v).reshape(-1)
    pre = np.full(48, front, np.uint8) if before is None else np.concatenate([np.full(48, front, np.uint8), S.pack(before).reshape(-1)])
    post = np.full(48, back, np.uint8) if after is None else np.concatenate([S.pack(after).reshape(-1), np.full(48, back, np.uint8)])
    pad = (off - pre.size) % 16
    host = np.concatenate([np.full(pad, front, np.uint8), pre, body, post])
    buf = torch.from_numpy(host).to(dev)
    a = pad + pre.size
    view = buf[a:a + body.size].view(*v.shape, 3)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == off and view.is_contiguous()
    return view, buf, a


def _detect(ctx, c, off=0, guards=True, max_runs=8192):
    """Case c through its call -> (rows, T or None); rows past the total keep the sentinel."""
    x, _, _ = _view(c.v, ctx.device, off, c.before if guards else None, c.after if guards else None)
    runs = torch.full((max_runs + 4, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
    chan = c.channel if c.v.ndim == 2 else None
    T = None
    if c.family == "quiet":
        _, cnt = ctx.quiet_runs(x, c.thr, c.min_len, max_runs, runs=runs, channel=chan)
    else:
        word = torch.full((1,), -1.0, device=ctx.device)
        if c.family == "dead":
            _, cnt = ctx.dead_runs(x, c.kind, c.thr, c.rel, c.tol, c.min_len, max_runs, runs=runs, channel=chan, threshold_out=word)
        else:
            _, cnt = ctx.level_runs(x, c.half, c.thr, c.rel, c.min_len, max_runs, runs=runs, channel=chan, threshold_out=word)
        T = np.float32(word.item())
    total = int(cnt.item())
    rows = runs.cpu().numpy()
    assert total <= max_runs and np.all(rows[total:] == SENTINEL), c.name
    return rows[:total], T


def _check(ctx, c, off=0):
    rows, T = _detect(ctx, c, off)
    want, wantT = S.expected(c)
    assert np.array_equal(rows, want), (c.name, off, rows[:6].tolist(), want[:6].tolist())
    if c.rows is not None:                                             # a lifted case: the int16 case's own rows
        assert np.array_equal(rows, c.rows), (c.name, off)
    if T is not None:
        assert T.tobytes() == np.float32(wantT).tobytes(), (c.name, T, wantT)
        assert c.T is None or T.tobytes() == np.float32(c.T).tobytes(), (c.name, T, c.T)
    return len(rows)


# ------------------------------------------------------------------------------------------------------------ detection
@pytest.mark.parametrize("table", ["lifted_quiet_cases", "lifted_dead_cases", "lifted_level_cases", "value_cases", "channel_value_cases"])
def test_detection_on_the_case_tables(table):
    """All three families: the int16 tables times 256 (held links across the 8-sample, 64-lane and 2048-sample seams among them), the
    values only 24 bits hold, and ch in {2, 3, 8}, one channel and joint.  The aligned route at offset 0, the staged one at 5."""
    ctx = _engine().ctx
    found = 0
    for k, c in enumerate(_cases(table)):
        found += _check(ctx, c, 0)
        if c.v.ndim == 1 and k % 3 == 0:
            _check(ctx, c, 5)
    assert found > 0


@pytest.mark.parametrize("off", range(16))
def test_quiet_runs_at_every_base_alignment(off):
    """n = 2 * 2048 + 77 at every byte offset 0 .. 15 from the 16-byte grid: offsets 0 and 8 take the wide loads, the others the staged
    route; 0x7F bytes in front of the view and 0x80 behind it (full-scale samples, whichever way they are cut) change nothing."""
    ctx = _engine().ctx
    n = 2 * D.CHUNK + 77
    tight = None
    for name, q, min_len in D.seam_cases(n)[::2]:
        x = D.materialize(q, np.int16, n)
        c = S.Case("quiet", name, S._lift(x), 256.0 * D.THR[np.int16], min_len, rows=D.quiet_runs_ref(x, D.THR[np.int16], min_len))
        _check(ctx, c, off)
        tight = c
    v = torch.from_numpy(S.pack(tight.v)).to(ctx.device)              # a tight copy: an allocation of its own, nothing around it
    runs, cnt = ctx.quiet_runs(v, tight.thr, tight.min_len, 64)
    assert runs[:int(cnt.item())].cpu().numpy().tolist() == _detect(ctx, tight, off)[0].tolist()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049])
def test_quiet_and_dead_runs_at_the_small_sizes(n):
    ctx = _engine().ctx
    for c in S.lifted_quiet_cases((n,)):
        for off in (0, 3, 8):
            _check(ctx, c, off)
    rng = np.random.default_rng(n)
    v = rng.integers(S.LO, S.HI + 1, n).astype(np.int32)
    v[rng.random(n) < 0.5] = 0x012345
    for off in (0, 1):
        _check(ctx, S.Case("quiet", f"random, n {n}", v, float(0x012345), 1), off)
        _check(ctx, S.Case("dead", f"random held, n {n}", v, 0.0, 1, None, R.ANY, 2.0 ** -12, 0.0), off)
        _check(ctx, S.Case("level", f"random level, n {n}", v, float(0x012345), 1, half=min(7, n)), off)


def test_the_guard_bytes_are_never_read():
    """Value cases whose answer a byte from outside would change: -1 | 0 boundaries, the peak, a held link to the neighbour outside."""
    ctx = _engine().ctx
    n = D.CHUNK + 9
    v = np.full(n, 0x7F7F7F, np.int32)                                 # the file equals what lies in front of it
    v[n // 2:] = S.unpack(np.full((1, 3), 0x80, np.uint8))[0]         # ... and behind it
    for off in range(0, 16, 3):
        for c in (S.Case("dead", "held to the outside", v, 0.0, 1, None, R.HELD, 0.0, 0.0),
                  S.Case("dead", "the peak outside", v // 2, 0.0, 1, None, R.QUIET, 0.75, 0.0),
                  S.Case("level", "windows to the outside", v, float(0x7F7F7F), 1, half=48)):
            rows, T = _detect(ctx, c, off, guards=False)
            want, wantT = S.expected(c)
            assert np.array_equal(rows, want) and T.tobytes() == np.float32(wantT).tobytes(), (c.name, off)


# ------------------------------------------------------------------------------------------------------------ cutters
T = native.CUT_RATE_TILE
T22 = 441 * native.CUT_PAIR_FRAMES
CUT_RATES = [48000, 44100, 16000, 8000]


def _cut_case(sr):
    """A 24-bit file whose 22.05 kHz axis holds a little over two si_cut_rate tiles and two si_cut_pair tiles and whose L16 rule allows
    one 16 kHz sample past N16 where the rate has such a length; 3 channels, channel 1 the file under test, the others full scale."""
    if ("cut", sr) not in _CACHE:
        P, Q = G.rate_ratio(sr)
        first = -(-(2 * T22 + 5 * 441 + 300) * Q // P) + 3
        n_file = next((n for n in range(first, first + 2000) if PR.lim16(n, sr) == PR.n_axis(n, sr, 16000) + 1), first)
        rng = np.random.default_rng(sr)
        v = rng.integers(-5_000_000, 5_000_001, size=n_file).astype(np.int32)
        v[:4] = [S.LO, S.HI, -1, 255]
        v[-3:] = [S.HI, S.LO, 0x00FF00]
        three = np.stack([np.where(np.arange(n_file) % 2 == 0, S.HI, S.LO).astype(np.int32), v, np.full(n_file, S.LO, np.int32)], axis=1)
        _CACHE["cut", sr] = dict(v=v, three=three, N22=F.n22(n_file, sr), lim=PR.lim16(n_file, sr), img=S.image(v))
    return _CACHE["cut", sr]


def _bounded(out, y, A, E, label):
    exact = A == 0
    assert np.array_equal(out[exact].view(np.int32), y[exact].astype(np.float32).view(np.int32)), label
    ratio = np.where(exact, 0.0, np.abs(out.astype(np.float64) - y) / np.maximum(E, 1e-300))
    assert float(ratio.max()) <= 1.0, (label, float(ratio.max()))


@pytest.mark.parametrize("sr", CUT_RATES)
def test_cut_rate_gives_the_fp32_image_s_bytes(sr):
    """Clips touching the file's first and last sample, on and off tile multiples; bases 0, 1, 2, 3 and 13 bytes off the 16-byte grid;
    mono and channel 1 of 3: the bytes of the fp32 call on F, inside feed_ref's bound."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    c = _cut_case(sr)
    filt = eng._feed_filter(sr)
    L = T + 1
    starts = [c["N22"] - L, 0, 77, T]
    want = ctx.cut_rate(torch.from_numpy(c["img"]).to(dev), sr, starts, L, filt)
    torch.cuda.synchronize()
    host = want.cpu().numpy()
    y, A, _ = F.clips(c["img"], sr, starts, L)
    _bounded(host, y, A, F.kernel_bound(y, A, sr), f"cut_rate {sr}")
    assert float(np.abs(y).max()) > 0.1
    for off in (0, 1, 2, 3, 13):
        mono = ctx.cut_rate(_view(c["v"], dev, off)[0], sr, starts, L, filt)
        chan = ctx.cut_rate(_view(c["three"], dev, off)[0], sr, starts, L, filt, channel=1)
        torch.cuda.synchronize()
        assert torch.equal(mono.view(torch.int32), want.view(torch.int32)), (sr, off, "mono")
        assert torch.equal(chan.view(torch.int32), want.view(torch.int32)), (sr, off, "channel 1 of 3")


@pytest.mark.parametrize("sr", CUT_RATES)
def test_cut_pair_gives_the_fp32_image_s_bytes(sr):
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    c = _cut_case(sr)
    f22, f16 = eng._feed_filter(sr), eng._feed_filter16(sr)
    L22 = T22 + 1
    L16 = -(-L22 * 320 // 441)
    last = min((c["N22"] - L22) // 441, (c["lim"] - L16) // 320)
    frames = [last, 0, 2]
    w22, w16 = ctx.cut_pair(torch.from_numpy(c["img"]).to(dev), sr, frames, L22, L16, f22, f16)
    whole22, whole16 = ctx.cut_pair(torch.from_numpy(c["img"]).to(dev), sr, [0], c["N22"], c["lim"], f22, f16)    # the file's last sample, and past N16
    torch.cuda.synchronize()
    ref = PR.clips(c["img"], sr, frames, L22, L16)
    _bounded(w22.cpu().numpy(), ref["y22"], ref["A22"], PR.kernel_bound(ref["y22"], ref["A22"], sr, 22050), f"cut_pair 22 {sr}")
    _bounded(w16.cpu().numpy(), ref["y16"], ref["A16"], PR.kernel_bound(ref["y16"], ref["A16"], sr), f"cut_pair 16 {sr}")
    for off in (0, 1, 2, 3, 13):
        m22, m16 = ctx.cut_pair(_view(c["v"], dev, off)[0], sr, frames, L22, L16, f22, f16)
        c22, c16 = ctx.cut_pair(_view(c["three"], dev, off)[0], sr, frames, L22, L16, f22, f16, channel=1)
        a22, a16 = ctx.cut_pair(_view(c["v"], dev, off)[0], sr, [0], c["N22"], c["lim"], f22, f16)
        torch.cuda.synchronize()
        for got, exp in ((m22, w22), (m16, w16), (c22, w22), (c16, w16), (a22, whole22), (a16, whole16)):
            assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (sr, off)


# ------------------------------------------------------------------------------------------------------------ patch
PATCH_RATES = [48000, 44100, 16000, 8000]
FILL = 0x5A


@pytest.mark.parametrize("sr", PATCH_RATES)
def test_patch_rate_writes_the_store_rule_of_the_fp32_call(sr):
    """tests/test_gpu_rate.py's case (s24_ref.patch_case) at fades 0, 7 and 5 ms, mono and as channel 1 of 3, with and without gain, at
    odd byte offsets: unwritten samples, the other channels and the guard bytes keep their sentinel bytes; a written sample is the
    store rule of the fp32 call's fp32 and lies inside the definition's bound; a chunk list that walks every span gives the same bytes."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    filt = eng._rate_filter(sr)
    off = 1 + PATCH_RATES.index(sr) * 4                                # 1, 5, 9, 13
    for fade_f in (0, 7, G.file_fade(5.0, sr)):
        c = S.patch_case(sr, fade_f)
        n, v = S.N_FILE, c["v"]
        img = S.image(v)
        it = RR.interpolate(sr, c["spans"], c["windows"], [c["gen"][0].numpy(), c["gen"][1].numpy()], fade_f, n)
        gen = c["gen"].to(dev)
        table = native.RateTable(c["spans"], c["windows"], c["chunks"], 2, fade_f, dev)
        wide = native.RateTable(c["spans"], c["windows"], [(q, 0, 5) for q in range(4)], 2, fade_f, dev)
        orig, _, _ = _view(v, dev, off)
        three = np.stack([np.full(n, S.HI, np.int32), v, np.full(n, S.LO, np.int32)], axis=1)
        orig3, _, _ = _view(three, dev, (off + 2) % 16)
        for gain_host in (None, np.array([0.8, 1.3], dtype=np.float32)):
            gain = None if gain_host is None else torch.from_numpy(gain_host).to(dev)
            ref, E, written = RR.blend(img, it, gain_host)
            assert written.sum() >= sum(l for _, l, _, _ in c["spans"][:4]) and not written[c["spans"][4][3]:].any()
            f32out = torch.full((n,), 7.25, device=dev)
            ctx.patch_rate(torch.from_numpy(img).to(dev), sr, table, gen, filt, f32out, gain)
            want = S.store(f32out.cpu().numpy())
            outs = []
            for tab, shape, o, chan in ((table, (n, 3), orig, None), (wide, (n, 3), orig, None), (table, (n, 3, 3), orig3, 1)):
                buf = torch.full((int(np.prod(shape)) + 96 + 16,), FILL, dtype=torch.uint8, device=dev)
                a = 48 + (off + len(outs) - buf.data_ptr()) % 16
                out = buf[a:a + int(np.prod(shape))].view(shape)
                assert out.data_ptr() % 16 == (off + len(outs)) % 16
                ctx.patch_rate(o, sr, tab, gen, filt, out, gain, channel=chan)
                torch.cuda.synchronize()
                whole = buf.cpu().numpy()
                assert np.all(whole[:a] == FILL) and np.all(whole[a + out.numel():] == FILL), (sr, fade_f, "guard bytes")
                got = whole[a:a + out.numel()].reshape(shape)
                if chan is not None:
                    assert np.all(got[:, 0] == FILL) and np.all(got[:, 2] == FILL), (sr, fade_f, "the other channels")
                    got = got[:, 1]
                outs.append(got)
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (sr, fade_f)
            got = outs[0]
            assert np.all(got[~written] == FILL), (sr, fade_f, "unwritten samples")
            val = S.unpack(got[written])
            assert np.array_equal(val, want[written]), (sr, fade_f, int((val != want[written]).sum()))
            lo, hi = S.store_f64(ref[written] - E[written]), S.store_f64(ref[written] + E[written])
            assert np.all((lo <= val) & (val <= hi)), (sr, fade_f, int(((val < lo) | (val > hi)).sum()))
            assert float(np.abs(ref[written]).max()) > 0.1 and int(np.abs(val).max()) > (1 << 20)


def test_the_store_rule_at_its_edges():
    """One span of weight 1 over a generator row that holds +-1.5, NaN, +-inf and 3e38, far enough apart to stay apart: values at and
    past full scale are clamped to 2^23 - 1 and -2^23, NaN is 0, and every written sample is the store rule of the fp32 call's fp32."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    sr = 44100
    n = 4 * 2048 + 77
    filt = eng._rate_filter(sr)
    H = RR.reach(sr)
    row = np.zeros(3000 + 2 * H, np.float32)
    spans, windows = [(200, 5800, 0, 6100)], [(0, 0, row.size, row.size)]
    chunks = G.region_chunks(G.file_regions([(200, 5800)], [6100], 0))
    special = np.array([1.5, -1.5, np.nan, np.inf, -np.inf, 0.99999994, -0.99999994, 2.0 ** -23, -(2.0 ** -23), 2.0 ** -24, 3e38, -3e38, 1.0], np.float32)
    row[300:300 + 200 * special.size:200] = special
    gen = torch.from_numpy(row)[None].contiguous().to(dev)
    table = native.RateTable(spans, windows, chunks, 1, 0, dev)
    f32out = torch.full((n,), 7.25, device=dev)
    ctx.patch_rate(torch.zeros(n, device=dev), sr, table, gen, filt, f32out)
    out = torch.full((n, 3), FILL, dtype=torch.uint8, device=dev)
    ctx.patch_rate(_view(np.zeros(n, np.int32), dev, 7)[0], sr, table, gen, filt, out)
    torch.cuda.synchronize()
    w, raw = f32out.cpu().numpy()[200:6000], out.cpu().numpy()
    got = S.unpack(raw)[200:6000]
    assert np.all(raw[:200] == FILL) and np.all(raw[6000:] == FILL)
    assert np.array_equal(got, S.store(w))
    assert np.isnan(w).any() and (w >= 1.0).any() and (w <= -1.0).any() and np.isinf(w).any()
    assert got.max() == S.HI and got.min() == S.LO and np.all(got[np.isnan(w)] == 0)
