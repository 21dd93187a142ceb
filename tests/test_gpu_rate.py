"""Repair at the file's own sample rate: si_patch_rate alone on synthetic generator rows, then the route --
engine.patch_file, engine.conceal_file and `long: {rate: file}` of predict.yaml -- on test_gpu_long.py's shapes.

The reference is tests/rate_ref.py, the definition in numpy float64.  A written fp32 sample must lie within
    E = 7 * 2^-24 * (|orig| + |gain| A),   A = sum |c x| over the sample's taps
of it: the roundings of the composition (the fp32 rounding of the sum, gain * y, (1 - w) * orig, the fma: one more than DESIGN.md 4.13
counts, each at most 2^-24 of |orig| + |gain| A) plus the float64 sum's 2 H 2^-53 A, which the kernel's fma order and numpy's separate
multiply-add may spend differently.  An int16 sample must equal trunc(ref * 32768); +-1 is accepted only where ref * 32768 lies within
E * 32768 of an integer, for at most 10 % of the written samples (2 E 32768 is under 2 % at amplitude 0.3; the reference alone is
counted under 5 %).  Samples of weight 0 keep the bits of a sentinel-filled output."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from tests import rate_ref as R
from tests.cases import _patch_engine as _engine
from tests.harness import RatioSummary

pytestmark = pytest.mark.gpu

N_FILE = 3 * 2048 + 77
RATES = [48000, 44100, 16000, 8000]
AMP = 0.3
SUMMARY = RatioSummary()
_CASES, _REFS = {}, {}


def _i32(t):
    return t.contiguous().view(torch.int32)


def _case(sr, fade_f):
    """Five spans over two windows of two contexts (file samples; see the comments), their windows, rows and the canonical chunk list."""
    if (sr, fade_f) in _CASES:
        return _CASES[sr, fade_f]
    P, Q = G.rate_ratio(sr)
    H = R.reach(sr)
    n22 = -(-N_FILE * P // Q)
    gap = 3 + fade_f // 2
    raw = [(30, 100, 0),                    # A: its taps (at the default fade its ramp too) reach in front of recording sample 0
           (2048 - 60, 150, 0),             # B: across the seam of chunks 0 | 1
           (2700, 80, 0),                   # C
           (2780 + gap, 90, 1),             # D: closer to C than two fades -- the ramps overlap -- and served by ANOTHER window
           (3 * 2048 - 100, 150, 1)]        # E: across the seam of chunks 2 | 3 and cut by lim_f
    reg = lambda s, l: (max(s - fade_f, 0), s + l + fade_f)
    len0 = (reg(*raw[2][:2])[1] - 1) * P // Q + 1 + H + 5
    ws1 = reg(*raw[3][:2])[0] * P // Q - H - 3
    lim1 = (3 * 2048 + 6) * P // Q                                   # window 1's context ends inside E
    windows = [(0, 0, len0, len0), (1, ws1, lim1 + 10 - ws1, lim1)]  # row 1 runs 10 samples PAST its context's end: they must read as zero
    assert ws1 > 0 and lim1 + 10 <= n22
    lims = [min(G.file_lim(w[3], sr), N_FILE) for w in windows]
    spans = [(s, l, w, lims[w]) for s, l, w in raw]
    assert raw[4][0] < lims[1] < raw[4][0] + raw[4][1] and lims[0] > reg(*raw[2][:2])[1]
    regions = G.file_regions([(s, l) for s, l, _, _ in spans], [sp[3] for sp in spans], fade_f)
    chunks = G.region_chunks(regions)
    assert [c for c, _, _ in chunks] == [0, 1, 2, 3]
    g = torch.Generator().manual_seed(sr + fade_f)
    lrow = max(w[2] for w in windows) + 3
    gen = ((torch.rand(2, lrow, generator=g) * 2 - 1) * AMP).contiguous()
    orig = ((torch.rand(N_FILE, generator=g) * 2 - 1) * AMP).contiguous()
    _CASES[sr, fade_f] = dict(spans=spans, windows=windows, chunks=chunks, regions=regions, gen=gen, orig=orig, lrow=lrow, H=H)
    return _CASES[sr, fade_f]


def _interp(sr, fade_f):
    if (sr, fade_f) not in _REFS:
        c = _case(sr, fade_f)
        _REFS[sr, fade_f] = R.interpolate(sr, c["spans"], c["windows"], [c["gen"][0].numpy(), c["gen"][1].numpy()], fade_f, N_FILE)
    return _REFS[sr, fade_f]


def _filt(eng, sr):
    return eng._rate_filter(sr)


def _off_grid(t, off, dev):
    """t on the device, its first element `off` elements past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
    v = buf[off:off + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16 != 0
    return v.view(t.shape)


def _check(got, ref, E, written, fill, pcm, label):
    """got / fill: host arrays of the file's type; ref, E: `blend`'s.  -> asserts, notes the worst ratio."""
    assert np.array_equal(got[~written].view(np.int32 if not pcm else np.int16), fill[~written].view(np.int32 if not pcm else np.int16)), label
    if not pcm:
        err = np.abs(got[written].astype(np.float64) - ref[written])
        ratio = float((err / E[written]).max())
        SUMMARY.note(label, ratio, ratio)
        assert ratio <= 1.0, (label, ratio)
        return
    v = ref[written] * 32768.0
    want = np.trunc(v)
    d = got[written].astype(np.float64) - want
    near = np.abs(v - np.round(v)) <= E[written] * 32768.0
    assert np.all((d == 0) | ((np.abs(d) == 1) & near)), (label, int(np.sum((d != 0) & ~near)))
    assert np.mean(d != 0) <= 0.10 and np.mean(near) < 0.05, (label, float(np.mean(d != 0)), float(np.mean(near)))
    SUMMARY.note(label + " (int16: fraction off by one / 0.10)", float(np.mean(d != 0)) / 0.10, float(np.mean(near)) / 0.05)


# ------------------------------------------------------------------------------------------------------------ kernel alone
@pytest.mark.parametrize("pcm", [False, True], ids=["fp32", "int16"])
@pytest.mark.parametrize("sr", RATES)
def test_kernel_against_the_definition(sr, pcm):
    from speech_inpainting_amd import native
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    off = 1 + RATES.index(sr) % 3
    for fade_f in (0, 7, G.file_fade(5.0, sr)):
        c = _case(sr, fade_f)
        it = _interp(sr, fade_f)
        o_host = (c["orig"].numpy() * 32767.0).astype(np.int16) if pcm else c["orig"].numpy()
        orig = _off_grid(torch.from_numpy(o_host), off, dev)
        gen = _off_grid(c["gen"], 4 - off, dev)
        fill_host = np.full(N_FILE, 77, dtype=np.int16) if pcm else np.full(N_FILE, 7.25, dtype=np.float32)
        if not pcm:                                                   # -0.0 and a NaN payload where nothing is written
            unwritten = np.flatnonzero(it["owner"] < 0)
            fill_host.view(np.int32)[unwritten[::97]] = -2 ** 31
            fill_host.view(np.int32)[unwritten[5::97]] = 0x7fc12345
        for gain_host in (None, np.array([0.8, 1.3], dtype=np.float32)):
            gain = None if gain_host is None else torch.from_numpy(gain_host).to(dev)
            ref, E, written = R.blend(o_host, it, gain_host)
            assert written.sum() >= sum(l for _, l, _, _ in c["spans"][:4]) and not written[c["spans"][4][3]:].any()
            table = native.RateTable(c["spans"], c["windows"], c["chunks"], 2, fade_f, dev)
            out = _off_grid(torch.from_numpy(fill_host), off, dev)
            ctx.patch_rate(orig, sr, table, gen, _filt(eng, sr), out, gain)
            # the same table, every chunk walking every span: the same bytes
            wide = native.RateTable(c["spans"], c["windows"], [(q, 0, 5) for q in range(4)], 2, fade_f, dev)
            out2 = _off_grid(torch.from_numpy(fill_host), (off % 3) + 1, dev)
            ctx.patch_rate(orig, sr, wide, gen, _filt(eng, sr), out2, gain)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got.view(np.int16 if pcm else np.int32), out2.cpu().numpy().view(np.int16 if pcm else np.int32))
            _check(got, ref, E, written, fill_host, pcm, f"patch_rate {sr} Hz")
            if not pcm:                                               # every sample the definition writes was written (7.25 is no sample's value)
                assert np.all(got[written] != np.float32(7.25)) and float(np.abs(ref[written]).max()) > 0.1
            if fade_f == 7 and not pcm:                               # the overlapping ramps of C and D belong to two windows
                s_d = c["spans"][3][0]
                assert {int(k) for k in it["owner"][s_d - 7:s_d]} == {2, 3} and 0 < it["w"][s_d - 4] < 1


def test_kernel_summary():
    SUMMARY.report(line="   SUMMARY {key}: max err/E {near:.4f} (second figure {rest:.4f}) over {checks} checks")


def test_the_reference_alone_rarely_sits_on_an_integer():
    """CPU count behind the int16 rule: the share of written reference samples within E * 32768 of an integer stays under 5 %."""
    for sr in RATES:
        it = _interp(sr, 7)
        c = _case(sr, 7)
        ref, E, written = R.blend((c["orig"].numpy() * 32767.0).astype(np.int16), it, None)
        v = ref[written] * 32768.0
        assert np.mean(np.abs(v - np.round(v)) <= E[written] * 32768.0) < 0.05


def test_refusals_launch_nothing():
    """Straight at the C ABI: every malformed call returns an error code and a message naming the entry, launches nothing and leaves
    the output untouched."""
    from speech_inpainting_amd import native
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    sr, fade_f = 48000, 240
    c = _case(sr, fade_f)
    spans, wins, chunks, lrow = c["spans"], c["windows"], c["chunks"], c["lrow"]
    orig, gen = c["orig"].to(dev), c["gen"].to(dev)
    out = torch.full((N_FILE,), 7.0, device=dev)
    f0 = _filt(eng, sr)
    keep = []

    def table(spans_=spans, wins_=wins, chunks_=chunks, fade_=fade_f, n_ctx=2):
        t = native.RateTable(spans_, wins_, chunks_, n_ctx, max(fade_, 0), dev)
        keep.append(t)
        st = t.struct()
        st.fade = fade_
        return st

    def filt(**kw):
        d = dict(nwin=f0["win"].numel(), num_table=f0["num_table"], step=f0["step"], scale=f0["scale"], win=f0["win"].data_ptr(), dwin=f0["dwin"].data_ptr())
        d.update(kw)
        return native.SincFilter(C.sizeof(native.SincFilter), d["nwin"], d["num_table"], d["step"], 0, 0, d["scale"], 0.0, d["win"], d["dwin"], None)

    def refused(st=None, f=None, sr_=sr, n=N_FILE, o=out, x=orig, lrow_=lrow):
        st = table() if st is None else st
        f = filt() if f is None else f
        ctx.profile_start(100)
        rc = ctx.lib.si_patch_rate(ctx._h, native._ptr(x), 0, n, sr_, C.byref(st) if st else None, native._ptr(gen), lrow_, None, C.byref(f) if f else None,
                                   native._ptr(o), ctx._stream())
        msg = ctx.lib.si_last_error(ctx._h).decode()
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        torch.cuda.synchronize()
        assert rc != 0 and msg.startswith("si_patch_rate: ") and launched == [], (rc, msg, launched)
        assert bool((out == 7.0).all())
        return msg

    def swap(rows, k, j, v):
        r = list(rows[k])
        r[j] = v
        return rows[:k] + [tuple(r)] + rows[k + 1:]

    assert "outside 4000 .. 192000" in refused(sr_=3999) and "outside 4000 .. 192000" in refused(sr_=192001)
    assert "22050" in refused(sr_=22050)
    assert "at most" in refused(n=2 ** 31 - 1 - 2047)
    assert "at 22050 Hz" in refused(sr_=8000, n=2 ** 30)                                      # 2^30 samples at 8 kHz are 2.96e9 at 22.05 kHz
    assert "NULL / empty" in refused(o=None) and "NULL / empty" in refused(n=0)
    assert "out is orig" in refused(o=orig)
    assert "size mismatch" in refused(st=False) and "si_sinc_filter size mismatch" in refused(f=False)
    st = table()
    st.struct_size -= 8
    assert "si_rate_table size mismatch" in refused(st)
    for bad in (dict(nwin=1), dict(num_table=0), dict(step=0), dict(scale=0.0), dict(scale=1.5), dict(win=None), dict(dwin=None)):
        assert "bad filter table" in refused(f=filt(**bad))
    assert "bad filter table" in refused(f=filt(step=2))                                      # 16 385 taps per wing: no chunk's row fits
    assert "fade" in refused(table(fade_=-1))
    # si_patch_regions' refusals, on the file axis
    assert "unsorted or overlapping" in refused(table([spans[1], spans[0]] + spans[2:]))
    assert "span 1" in refused(table(swap(spans, 1, 1, 0))) and "span 0" in refused(table(swap(spans, 0, 0, -5)))
    assert "lim" in refused(table(swap(spans, 4, 3, N_FILE + 1))) and "lim" in refused(table(swap(spans, 1, 3, spans[1][0])))
    assert "names window 2 of 2" in refused(table(swap(spans, 0, 2, 2))) and "names window -1" in refused(table(swap(spans, 0, 2, -1)))
    assert "window 1 names context 2" in refused(table(wins_=swap(wins, 1, 0, 2))) and "names context 0 of 0" in refused(table(n_ctx=0))
    assert "outside the recording" in refused(lrow_=wins[0][2] - 1) and "outside the recording" in refused(table(wins_=swap(wins, 0, 1, -1)))
    assert "its context's audio ends" in refused(table(wins_=swap(wins, 1, 3, wins[1][1])))                  # win_lim <= win_start
    assert "its context's audio ends" in refused(table(wins_=swap(wins, 1, 3, 10 ** 6)))                     # win_lim past the recording
    assert "not strictly increasing" in refused(table(chunks_=[chunks[1], chunks[0]] + chunks[2:]))
    assert "at or past" in refused(table(chunks_=chunks + [(4, 5, 5)]))
    assert "walks spans" in refused(table(chunks_=swap(chunks, 0, 2, 6)))
    assert "lacks chunk 3" in refused(table(chunks_=chunks[:3])) and "lacks chunk" in refused(table(chunks_=[]))
    assert "omits span" in refused(table(chunks_=swap(chunks, 0, 2, chunks[0][1])))
    # the span table on the file axis against the windows on the 22.05 kHz axis
    assert "span 4 writes up to" in refused(table(swap(spans, 4, 3, spans[4][3] + 2)))                         # lim_f past its context's end
    assert "span 3 blends" in refused(table(wins_=swap(wins, 1, 1, wins[1][1] + 4)))                           # the row starts 1 tap late
    assert "span 2 blends" in refused(table(wins_=[(0, 0, wins[0][2] - 6, wins[0][2]), wins[1]]))             # the row ends 1 tap early
    assert "span 0 blends" not in refused(table(wins_=[(0, 0, wins[0][2] - 6, wins[0][2]), wins[1]]))         # (A reaches below sample 0: allowed)
    assert "its window's row holds" in refused(table(swap(spans, 2, 2, 1)))                                    # C in window 1, which starts behind it
    # num_chunks = 0 launches nothing and succeeds; the good table works
    ctx.profile_start(100)
    ctx.patch_rate(orig, sr, native.RateTable([], [], [], 0, 0, dev), None, f0, out, None)
    assert [e for e in ctx.profile_stop() if e["launches"] > 0] == [] and bool((out == 7.0).all())
    ctx.profile_start(100)
    ctx.patch_rate(orig, sr, native.RateTable(spans, wins, chunks, 2, fade_f, dev), gen, f0, out, None)
    prof = {e["name"]: e["launches"] for e in ctx.profile_stop() if e["launches"] > 0}
    torch.cuda.synchronize()
    assert prof == {"patch_rate": 1} and float(out[N_FILE - 1]) == 7.0 and not bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ the route
N_REC, CLIP, CTX = 300, 75, 15
GAPS = [(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)]              # test_gpu_long.py's
KW = dict(clip_frames=CLIP, min_context=CTX)
ROUTE_RATES = [48000, 16000]


def _file(sr, seed=41):
    """A recording of 300 frames and 77 samples at `sr` Hz as an fp32 and an int16 file."""
    from speech_inpainting_amd import synth
    n = N_REC * (sr // 50) + 77
    x16 = (synth.synth_wave(1, n, seed, sr=sr)[0] * 32767.0).to(torch.int16)
    return x16.to(torch.float32) / 32768.0, x16                      # the fp32 file holds the int16 file's values: one model pass serves both


def _full_pass_reference(eng, x32, sr, got, whole=False):
    """rate_ref on a FULL generator pass per context: -> the `interpolate` record (shared by both sample types) and the gains.
    whole: the recording is one context of its own length."""
    n_file = x32.numel()
    wave22 = eng.resample(x32.to(eng.device)[None], sr, 22050)[0]
    L22 = wave22.numel() if whole else CLIP * 441
    ctxs = got["contexts"]
    cut22 = torch.stack([wave22[441 * c["start"]:441 * c["start"] + L22] for c in ctxs])
    cut16 = eng.resample(cut22, 22050, 16000)
    full = eng.predict_multigap_batch(cut16, cut22, [c["own"] + c["foreign"] for c in ctxs], vocode=True)
    wave = full["wave"].cpu().numpy()
    lim_loc = min(L22, wave.shape[1])
    windows = [(b, 441 * c["start"], lim_loc, 441 * c["start"] + lim_loc) for b, c in enumerate(ctxs)]
    spans = []
    for b, c in enumerate(ctxs):
        lim_f = G.file_lim(windows[b][3], sr, n_file)
        spans += [(s, l, b, lim_f) for s, l in G.file_spans([(c["start"] + p, l) for p, l in c["own"]], sr)]
    gains = torch.cat([p["gain"] for p in got["passes"]]).cpu().numpy()
    return R.interpolate(sr, spans, windows, list(wave), G.file_fade(5.0, sr), n_file), gains


@pytest.mark.parametrize("sr", ROUTE_RATES)
@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_patch_file_against_full_generator_passes(voc, sr):
    """The acceptance test.  Outside the regions the output is the file's bits, fp32 and int16; inside, it is the definition applied to
    a full generator pass of each context within E -- which windows without the interpolation's reach would miss."""
    eng = _engine(voc)
    x32, x16 = _file(sr)
    got = eng.patch_file(x32, sr, GAPS, return_windows=True, **KW)
    got16 = eng.patch_file(x16.numpy(), sr, list(reversed(GAPS)), **KW)                 # a host array, the gaps in any order
    torch.cuda.synchronize()
    assert got["patched"].dtype == torch.float32 and got16["patched"].dtype == torch.int16 and got16["patched"].shape == x16.shape
    assert [c["start"] for c in got["contexts"]] == [0, 68, 106, 225] and got16["contexts"] == got["contexts"]
    assert got["label_off"] == [0, 3, 8, 12, 18, 23] and torch.equal(got["labels"], got16["labels"])
    it, gains = _full_pass_reference(eng, x32, sr, got)
    inside = it["owner"] >= 0
    fade_f = G.file_fade(5.0, sr)
    assert int(inside.sum()) == sum(l for _, l in G.file_spans(GAPS, sr)) + 2 * fade_f * len(GAPS)
    for x, res, pcm in ((x32, got, False), (x16, got16, True)):
        ref, E, written = R.blend(x.numpy(), it, gains)
        out = res["patched"].cpu().numpy()
        _check(out, ref, E, written, x.numpy(), pcm, f"patch_file {sr} Hz {voc}")
        for s, l in G.file_spans(GAPS, sr):                           # every gap was filled, by something other than the recording
            assert not np.array_equal(out[s:s + l], x.numpy()[s:s + l])
    SUMMARY.report(keys=[f"patch_file {sr} Hz {voc}"])


@pytest.mark.parametrize("sr", [8000, 11025, 44100])
def test_a_recording_shorter_than_a_clip_at_other_rates(sr):
    """One context, the whole recording with its true sample count (60 frames and 57 samples, int16), at a rate with 178 taps per
    wing, at the one with a single phase (11 025 Hz: P / Q = 2) and at the one with two (44 100 Hz); gaps further apart than a
    context's budget.  The same acceptance check."""
    from speech_inpainting_amd import synth
    eng = _engine()
    gaps = [(2, 3), (30, 4), (35, 4), (50, 8)]
    n = -(-60 * sr // 50) + 57
    x16 = (synth.synth_wave(1, n, 53, sr=sr)[0] * 32767.0).to(torch.int16)
    got = eng.patch_file(x16, sr, gaps, return_windows=True, **KW)
    torch.cuda.synchronize()
    assert len(got["contexts"]) == 1 and got["contexts"][0]["own"] == gaps and got["label_off"] == [0, 3, 7, 11, 19]
    it, gains = _full_pass_reference(eng, x16.to(torch.float32) / 32768.0, sr, got, whole=True)
    ref, E, written = R.blend(x16.numpy(), it, gains)
    assert int(written.sum()) == sum(l for _, l in G.file_spans(gaps, sr)) + 2 * G.file_fade(5.0, sr) * 4      # (30, 4) | (35, 4) lie one frame apart: 20 ms, no overlap at 5 ms
    _check(got["patched"].cpu().numpy(), ref, E, written, x16.numpy(), True, f"patch_file short {sr} Hz")


@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_batching_changes_no_byte(voc):
    eng = _engine(voc)
    for sr in ROUTE_RATES:
        _, x16 = _file(sr, seed=43)
        full = eng.patch_file(x16, sr, GAPS, batch=32, **KW)
        for batch in (1, 2):
            got = eng.patch_file(x16, sr, GAPS, batch=batch, **KW)
            torch.cuda.synchronize()
            assert torch.equal(got["patched"], full["patched"]) and torch.equal(got["labels"], full["labels"]), (sr, batch)
            assert got["label_off"] == full["label_off"] and got["contexts"] == full["contexts"]


def test_a_22050_hz_file_is_patch_recording_bit_for_bit():
    eng = _engine()
    x32, x16 = _file(22050, seed=45)
    ref = eng.patch_recording(x16.to(torch.float32) / 32768.0, GAPS, fade=110, pcm=True, **KW)
    got16 = eng.patch_file(x16, 22050, GAPS, **KW)
    ref32 = eng.patch_recording(x32, GAPS, fade=110, **KW)
    got32 = eng.patch_file(x32, 22050, GAPS, **KW)
    torch.cuda.synchronize()
    assert got16["patched"].dtype == torch.int16 and torch.equal(got16["patched"], ref["patched_pcm"]) and "patched_pcm" not in got16
    assert torch.equal(_i32(got32["patched"]), _i32(ref32["patched"])) and torch.equal(got32["labels"], ref32["labels"])
    keep = torch.ones(x16.numel(), dtype=torch.bool)
    for p, l in GAPS:
        keep[441 * p - 110:441 * (p + l) + 110] = False
    assert torch.equal(got16["patched"].cpu()[keep], x16[keep]) and not torch.equal(got16["patched"].cpu(), x16)


def test_conceal_file_finds_the_dropouts_of_an_int16_48k_file():
    eng = _engine()
    sr = 48000
    _, x16 = _file(sr, seed=47)
    x16 = x16.clone()
    for s, l in G.file_spans(GAPS, sr):
        x16[s:s + l] = 0
    # find_gaps' default merge_frames (two cross-fades' frames) joins (100, 5) and (106, 4), one frame apart, by design
    assert eng.find_gaps(x16, sr)["gaps"] == [(2, 3), (100, 10), (140, 6), (292, 5)]
    got = eng.conceal_file(x16, sr, threshold=0.0, merge_frames=1, **KW)
    ref = eng.patch_file(x16, sr, GAPS, **KW)
    torch.cuda.synchronize()
    assert got["gaps"] == GAPS and got["skipped"] == []
    assert got["patched"].dtype == torch.int16 and torch.equal(got["patched"], ref["patched"]) and torch.equal(got["labels"], ref["labels"])
    for s, l in G.file_spans(GAPS, sr):
        assert int((got["patched"][s:s + l] != 0).sum()) > l // 2
    # nothing to find: a copy, and only the detection kernels ran
    _, clean = _file(sr, seed=49)
    eng.ctx.profile_start(100)
    none = eng.conceal_file(clean, sr, threshold=0.0, **KW)
    launched = {e["name"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    assert none["gaps"] == [] and torch.equal(none["patched"].cpu(), clean) and launched and all(n.startswith("detect_") for n in launched)


@pytest.mark.parametrize("pcm", [False, True], ids=["fp32", "int16"])
def test_no_gaps_is_an_exact_copy_and_launches_nothing(pcm):
    eng = _engine()
    x32, x16 = _file(48000, seed=51)
    x = (x16 if pcm else x32).to(eng.device)
    if not pcm:
        x.view(torch.int32)[5] = -2 ** 31
        x.view(torch.int32)[6] = 0x7fc12345
    eng.ctx.profile_start(100)
    got = eng.patch_file(x, 48000, [], **KW)
    launched = [e for e in eng.ctx.profile_stop() if e["launches"] > 0]
    torch.cuda.synchronize()
    assert launched == [], launched
    assert got["patched"].data_ptr() != x.data_ptr() and got["patched"].dtype == x.dtype
    assert torch.equal(got["patched"].view(torch.int16), x.view(torch.int16))
    assert got["contexts"] == [] and got["labels"].numel() == 0 and got["label_off"] == [0]
    with pytest.raises(ValueError, match="outside 4000 .. 192000"):
        eng.patch_file(x, 3000, [], **KW)


def test_predict_entry_point_with_rate_file(tmp_path, monkeypatch, capsys):
    """predict.py with `long: {rate: file}` on a 48 kHz int16 file: the three waves keep the file's rate, type and sample count,
    patched.wav equals the file outside the planned regions; a stereo file is refused with a message."""
    import joblib
    from scipy.io import wavfile
    from sklearn.cluster import MiniBatchKMeans
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.predict import main

    harch, varch = HubertArch.base(), VocoderArch.v1()
    hsd, gsd, cb = synth.synth_hubert_state(harch, pos_conv_style="legacy"), synth.synth_generator_state(varch), synth.synth_codebook(100)
    (tmp_path / "trained_models").mkdir()
    torch.save(dict(hsd), tmp_path / "trained_models" / "save_checkpoint.pt")
    (tmp_path / "hifi_gan" / "LJ_V1").mkdir(parents=True)
    torch.save({"generator": dict(gsd)}, tmp_path / "hifi_gan" / "LJ_V1" / "generator_v1")
    (tmp_path / "hifi_gan" / "LJ_V1" / "config.json").write_text(json.dumps(dict(
        resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
        resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=80, sampling_rate=22050, seed=1234)))
    kdir = tmp_path / "kmeans" / "km_model_100"
    kdir.mkdir(parents=True)
    km = MiniBatchKMeans(n_clusters=100)
    km.cluster_centers_ = cb.numpy()
    joblib.dump(km, kdir / "model.km")
    sr = 48000
    n = 3 * sr + 77
    pcm_in = (synth.synth_wave(1, n, 5, sr=sr)[0].numpy() * 32767).astype(np.int16)
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", sr, pcm_in)
    wavfile.write(tmp_path / "wavs" / "stereo.wav", sr, np.stack([pcm_in, pcm_in], axis=1))
    text = f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/NAME.wav', save_pred: '{tmp_path}/prediction'}}}}
masks:
  - {{start_pos_in_sec: 2.0, end_pos_in_sec: 2.125}}
  - {{start_pos_in_sec: 0.5, end_pos_in_sec: 0.625}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2, rate: file}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
"""
    (tmp_path / "predict.yaml").write_text(text.replace("NAME", "call"))
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    assert sorted(p.name for p in out.iterdir()) == ["masked.wav", "orig.wav", "patched.wav"]
    files = {}
    for f in ("orig.wav", "masked.wav", "patched.wav"):
        rate, files[f] = wavfile.read(out / f)
        assert rate == sr and files[f].dtype == np.int16 and files[f].shape == (n,), f
    assert np.array_equal(files["orig.wav"], pcm_in)
    gaps = [(25, 6), (100, 6)]                                            # 0.5 s and 2 s on the 20 ms grid; 125 ms = 6 frames
    keep = np.ones(n, dtype=bool)
    zeroed = pcm_in.copy()
    for p, l in gaps:
        keep[960 * p - 240:960 * (p + l) + 240] = False                   # 960 samples per frame, the default fade: 5 ms = 240
        zeroed[960 * p:960 * (p + l)] = 0
        assert not np.array_equal(files["patched.wav"][960 * p:960 * (p + l)], pcm_in[960 * p:960 * (p + l)])
    assert np.array_equal(files["patched.wav"][keep], pcm_in[keep])
    assert np.array_equal(files["masked.wav"], zeroed)
    printed = capsys.readouterr().out
    assert all(f"gap {k} = frames [{p}, {p + l})" in printed for k, (p, l) in enumerate(gaps))
    (tmp_path / "predict.yaml").write_text(text.replace("NAME", "stereo"))
    with pytest.raises(ValueError, match="2 channels"):
        main([])
