"""Every file kernel at the far end of the longest files it accepts.  No model but for the one route test.

A far file is a body of one repeated value, filled on the device, with a tail of far.K sample times uploaded from numpy behind it; the
geometries (tests/far.py) are the smallest at which an element offset passes 2^31 or 2^32, a packed 24-bit byte offset 2^32, or a
sample time reaches the cap.  What a call gives there is what the float64 references of the existing tests give on the SHORT file --
far.Z sample times of the same fill and the same tail -- moved by the shift (far.lift; tests/test_far_host.py shows that the references
themselves obey that law and that a wrapped offset would break it).  Each comparison is the existing GPU test's own: run tables and PCM
equal, fp32 within that test's bound, through that test's helper.  As a second assertion the far call's output equals, bit for bit, the
same GPU call on the short file.

At most one far tensor is alive at a time (two where a call needs `orig` and `out`), freed in `finally`; a test that finds less free
device memory than it needs skips and says so."""
import functools

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import far
from tests import feed_ref as F
from tests import invalid_ref as IV
from tests import mend_ref as M
from tests import pair_ref as PR
from tests import rate_ref as RR
from tests import s24_ref as S
from tests.harness import build_engine
from tests.test_gpu_feed import _check as check_clips
from tests.test_gpu_mend import _compare as compare_mend
from tests.test_gpu_mend import _hold_condition as hold_condition
from tests.test_gpu_pair import _check16 as check_clips16
from tests.test_gpu_rate import _check as check_patch

pytestmark = pytest.mark.gpu

K, Z = far.K, far.Z
TORCH = {np.float32: torch.float32, np.int16: torch.int16}
FILLS = ["zero", "const"]
GIB = 2 ** 30


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", "fp32", key=("patch", "fp32"))


# ------------------------------------------------------------------------------------------------------------ files on the device
def _upload(x, dev):
    """A host file (its dtype far.S24 = int32 for packed 24-bit values) on the device in the type the kernels read."""
    return torch.from_numpy(S.pack(x) if x.dtype.type is far.S24 else np.ascontiguousarray(x)).to(dev)


def _download(t, dtype):
    host = t.cpu().numpy()
    return S.unpack(host).astype(far.S24) if dtype is far.S24 else host


def _fill_bytes(fill):
    return [(int(fill) >> s) & 0xFF for s in (0, 8, 16)]


def _far_file(geom, fill, tail, dev, copies=1):
    """The far file of `geom`: n - K sample times of fill written on the device, the tail behind them.  Skips when the device has not
    the memory for `copies` of it and a gibibyte of scratch."""
    need = copies * geom.bytes + GIB
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"{geom.name}: {need / GIB:.1f} GiB of device memory needed, {free / GIB:.1f} GiB free")
    shape = (geom.n,) if geom.ch == 1 else (geom.n, geom.ch)
    if geom.dtype is far.S24:
        x = torch.zeros(shape + (3,), dtype=torch.uint8, device=dev)
        if int(fill) != 0:
            for b, v in enumerate(_fill_bytes(fill)):
                x[..., b].fill_(v)
    else:
        x = torch.zeros(shape, dtype=TORCH[geom.dtype], device=dev)
        if float(fill) != 0.0:
            x.fill_(fill.item())
    x[geom.n - K:] = _upload(tail, dev)
    return x


def _body_is_fill(x, geom, fill, upto):
    """Sample times [0, upto) all hold `fill`: minimum and maximum by device reductions, no copy of the body."""
    body = x[:upto]
    if geom.dtype is far.S24:
        return all(tuple(int(v) for v in torch.aminmax(body[..., b])) == (v0, v0) for b, v0 in enumerate(_fill_bytes(fill)))
    lo, hi = torch.aminmax(body)
    return lo.item() == hi.item() == fill.item()


def _free():
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ the five detectors
def _find(eng, det, p, x, channel):
    """One engine call -> the rows on the host."""
    if det == "quiet":
        rows = eng.find_quiet_runs(x, p["thr"], 1, channel=channel)
    elif det == "dead":
        rows = eng.find_dead_runs(x, p["kind"], p.get("thr", 0.0), p.get("rel", 0.0), 0.0, 1, channel=channel)
    elif det == "level":
        rows = eng.find_level_runs(x, half=p["half"], threshold=p.get("thr", 0.0), rel_threshold=p.get("rel", 0.0), channel=channel)
    elif det == "burst":
        rows = eng.find_burst_runs(x, half=p["half"], threshold=p.get("thr", 0.0), rel_threshold=p.get("rel", 0.0), channel=channel)
    else:
        rows = eng.find_invalid_runs(x, p["ceiling"], channel=channel)
    return rows.cpu().numpy()


@pytest.mark.parametrize("fi", [0, 1], ids=FILLS)
@pytest.mark.parametrize("det", far.DETECTORS)
@pytest.mark.parametrize("gname", far.DETECTOR_GEOMETRIES)
def test_detector_rows_are_the_short_file_s_rows_moved(gname, det, fi):
    """find_*_runs on the far file, mono at CAP, the last channel and joint elsewhere, under every parameter set of far.detector_params
    (half 0, 1 and the largest; one relative threshold per detector, so that the peak pass runs far out): the rows are the reference's
    rows of the short file lifted by the shift -- under the zero fill with the body's run of almost 2^31 samples in front."""
    eng = _engine()
    g = far.GEOMETRIES[gname]
    fill, tail, shift = far.fills(g.dtype)[fi], far.detector_tail(g, det), far.shift_of(g.n)
    short = far.short_file(tail, fill)
    xs = _upload(short, eng.device)
    x, ends = None, False
    try:
        x = _far_file(g, fill, tail, eng.device)
        for p in far.detector_params(det, g.dtype):
            dead = far.fill_is_dead(det, p, fill)
            for c in far.channels_of(g):
                want = far.lift(far.reference_rows(det, p, short, c), shift, dead)
                got = _find(eng, det, p, x, c)
                assert np.array_equal(got, want), (gname, det, FILLS[fi], p, c, got[:3].tolist(), got[-3:].tolist(), want[:3].tolist(), want[-3:].tolist())
                assert np.array_equal(got, far.lift(_find(eng, det, p, xs, c), shift, dead)), (gname, det, FILLS[fi], p, c, "the short call")
                assert len(want) > int(dead) and (not dead or (want[0, 0] == 0 and want[0, 1] > shift))
                ends |= int(want[-1].sum()) == g.n
        assert ends, "no parameter set has a run that ends with the file"
    finally:
        del x, xs
        _free()


# ------------------------------------------------------------------------------------------------------------ si_mend_runs
@functools.lru_cache(maxsize=None)
def _mend_reference(gname, edge, fi):
    g = far.GEOMETRIES[gname]
    tail, rows = far.mend_case(g, edge)
    fill, c = far.fills(g.dtype)[fi], far.mend_channel(g)
    short = far.short_file(tail, fill)
    table = [(s + Z, m) for s, m in rows]
    ref = M.mend(short, table, channel=c, **far.MEND)
    hold_condition(f"far {gname}", ref, M.mend(short, table, channel=c, exact=True, **far.MEND))
    return tail, rows, short, table, ref


@pytest.mark.parametrize("fi", [0, 1], ids=FILLS)
@pytest.mark.parametrize("edge", [False, True], ids=["mended", "edge"])
@pytest.mark.parametrize("gname", far.MEND_GEOMETRIES)
def test_mend_runs_in_place_at_the_far_end(gname, edge, fi):
    """engine.mend_runs(inplace=True) on the far tensor, mono or its last channel: a row whose context reaches into the body, rows of 5,
    16 and 64 samples, and a last row whose e + context is n exactly (mended) or n + 1 (SI_MEND_EDGE, the file untouched there).
    tests/test_gpu_mend.py's comparison on the last Z + K sample times; everything in front still holds the fill."""
    eng = _engine()
    g = far.GEOMETRIES[gname]
    tail, rows, short, table, ref = _mend_reference(gname, edge, fi)
    fill, c, shift = far.fills(g.dtype)[fi], far.mend_channel(g), far.shift_of(g.n)
    assert ref.status.tolist() == [M.AR] * 4 + [M.EDGE if edge else M.AR]
    x = y = None
    try:
        x = _far_file(g, fill, tail, eng.device)
        y, status = eng.mend_runs(x, [(s + shift, m) for s, m in table], channel=c, inplace=True, **far.MEND)
        torch.cuda.synchronize()
        assert y.data_ptr() == x.data_ptr()
        got = _download(x[g.n - K - Z:], g.dtype)
        compare_mend(f"far {gname} {FILLS[fi]}", short, table, ref, got, status.cpu().numpy(), c, quiet=True)
        assert _body_is_fill(x, g, fill, g.n - K - Z), (gname, "the body changed")
        ys, ss = eng.mend_runs(_upload(short, eng.device), table, channel=c, **far.MEND)
        assert _download(ys, g.dtype).tobytes() == got.tobytes() and torch.equal(ss, status), (gname, "the short call")
    finally:
        del x, y
        _free()


# ------------------------------------------------------------------------------------------------------------ the cutters
def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _axis22(gname, sr, fi, valid):
    """The float64 reference of EVERY 22.05 kHz sample of the short file's channel (tests/test_gpu_feed.py's shape), for the plain
    cutters on the "dead" tail and for the _valid ones on the "invalid" tail with its invalid samples staged as +0.0."""
    g = far.GEOMETRIES[gname]
    plan = far.cut_plan(g, sr)
    tail = far.tail(g, "invalid" if valid else "dead")
    short = far.short_file(tail, far.fills(g.dtype)[fi], plan["lead"])
    col = short if short.ndim == 1 else short[:, g.ch - 1]
    col = IV.clean(col, far.ceiling(g.dtype)) if valid else col
    y, A, _ = F.samples(far.column(col, None), np.arange(plan["N22s"]), sr)
    return tail, short, y, A


@pytest.mark.parametrize("valid", [False, True], ids=["plain", "valid"])
@pytest.mark.parametrize("fi", [0, 1], ids=FILLS)
@pytest.mark.parametrize("gname,sr", [(g, sr) for g in far.CUT_GEOMETRIES for sr in far.cut_rates(far.GEOMETRIES[g])])
def test_cut_rate_at_the_far_end(gname, sr, fi, valid):
    """si_cut_rate / si_cut_rate_valid, mono or the last channel: a clip that ends with the 22.05 kHz axis (its right taps read the zero
    extension past n_file), one across that clip's last tile seam and one further in, within tests/test_gpu_feed.py's bound of the
    reference on the short file; the _valid form meets over-ceiling samples among the file's last."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    g = far.GEOMETRIES[gname]
    plan = far.cut_plan(g, sr)
    tail, short, y, A = _axis22(gname, sr, fi, valid)
    c = None if g.ch == 1 else g.ch - 1
    filt = eng._feed_filter(sr)
    cut = (lambda t, starts: ctx.cut_rate_valid(t, sr, starts, plan["L"], filt, far.ceiling(g.dtype), channel=c)) if valid else \
          (lambda t, starts: ctx.cut_rate(t, sr, starts, plan["L"], filt, channel=c))
    x = None
    try:
        x = _far_file(g, far.fills(g.dtype)[fi], tail, dev)
        got = cut(x, plan["starts"])
        want = cut(_upload(short, dev), plan["short"])
        torch.cuda.synchronize()
        check_clips(got.cpu().numpy(), plan["short"], plan["L"], y, A, sr, f"far {gname} cut_rate {sr} Hz")
        assert torch.equal(_bits(got), _bits(want)), (gname, sr, int((_bits(got) != _bits(want)).sum()))
        assert float(got[0, -8:].abs().max()) > 0 and float(got.abs().max()) > 0.01
    finally:
        del x
        _free()


@pytest.mark.parametrize("valid", [False, True], ids=["plain", "valid"])
@pytest.mark.parametrize("gname,sr", [(g, sr) for g in far.CUT_GEOMETRIES for sr in far.cut_rates(far.GEOMETRIES[g])])
def test_cut_pair_at_the_far_end(gname, sr, valid):
    """si_cut_pair / si_cut_pair_valid under the constant fill, the shift a whole number of 20 ms frames: the 22.05 kHz rows are
    si_cut_rate's bytes, the 16 kHz rows lie within tests/test_gpu_pair.py's bound of the reference on the short file; the first clip
    ends with both axes."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    g = far.GEOMETRIES[gname]
    pp = far.pair_plan(g, sr)
    tail = far.tail(g, "invalid" if valid else "dead")
    fill = far.fills(g.dtype)[1]
    short = far.short_file(tail, fill, pp["lead"])
    col = short if short.ndim == 1 else short[:, g.ch - 1]
    col = far.column(IV.clean(col, far.ceiling(g.dtype)) if valid else col, None)
    y16, A16, _ = PR.samples16(col, np.arange(pp["lims"]), sr)
    c = None if g.ch == 1 else g.ch - 1
    f22, f16 = eng._feed_filter(sr), eng._feed_filter16(sr)
    ceil = far.ceiling(g.dtype)
    pair = (lambda t, fr: ctx.cut_pair_valid(t, sr, fr, pp["L22"], pp["L16"], f22, f16, ceil, channel=c)) if valid else \
           (lambda t, fr: ctx.cut_pair(t, sr, fr, pp["L22"], pp["L16"], f22, f16, channel=c))
    rate = (lambda t, st: ctx.cut_rate_valid(t, sr, st, pp["L22"], f22, ceil, channel=c)) if valid else \
           (lambda t, st: ctx.cut_rate(t, sr, st, pp["L22"], f22, channel=c))
    x = None
    try:
        x = _far_file(g, fill, tail, dev)
        g22, g16 = pair(x, pp["frames"])
        r22 = rate(x, [441 * f for f in pp["frames"]])
        s22, s16 = pair(_upload(short, dev), pp["short"])
        torch.cuda.synchronize()
        assert torch.equal(_bits(g22), _bits(r22)), (gname, sr, "out22 | si_cut_rate")
        check_clips16(g16.cpu().numpy(), pp["short"], y16, A16, sr, f"far {gname} cut_pair {sr} Hz")
        assert torch.equal(_bits(g22), _bits(s22)) and torch.equal(_bits(g16), _bits(s16)), (gname, sr, "the short call")
        assert float(g16.abs().max()) > 0.01 and float(g22[0, -8:].abs().max()) > 0
    finally:
        del x
        _free()


# ------------------------------------------------------------------------------------------------------------ si_patch_rate
@pytest.mark.parametrize("fi", [0, 1], ids=FILLS)
@pytest.mark.parametrize("gname", ["CAP", "S24"])
def test_patch_rate_at_the_far_end(gname, fi):
    """One span that ends with the file, cross-faded in front (tests/test_gpu_channels.py's), mono at CAP and the last channel at S24,
    `out` a clone of the far file: the written samples meet the definition on the short file by
    tests/test_gpu_rate.py's check (packed 24-bit: tests/test_gpu_s24.py's, the store rule inside the bound), and everything outside the
    span keeps its bits -- the other channel, and the whole body, by one device reduction."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    g = far.GEOMETRIES[gname]
    sr = 48000
    fade_f, filt = G.file_fade(5.0, sr), eng._rate_filter(sr)
    plan = far.patch_plan(g, sr, fade_f, filt["reach"])
    fill, tail = far.fills(g.dtype)[fi], far.tail(g, "dead")
    short = far.short_file(tail, fill, plan["lead"])
    c = None if g.ch == 1 else g.ch - 1
    col = far.column(short, c)
    k, wl = plan["k"], plan["wl"]
    gen_host = ((torch.rand(1, wl + 5, generator=torch.Generator().manual_seed(3)) * 2 - 1) * 0.3).contiguous()
    it = RR.interpolate(sr, plan["short"]["spans"], plan["short"]["windows"], [gen_host[0].numpy()], fade_f, k)
    ref, E, written = RR.blend(col, it, None)
    assert written[k - 700:].all() and written.sum() == 700 + fade_f and not written[:k - 700 - fade_f].any()
    gen = gen_host.to(dev)
    table = native.RateTable(plan["far"]["spans"], plan["far"]["windows"], plan["far"]["chunks"], 1, fade_f, dev)
    table_s = native.RateTable(plan["short"]["spans"], plan["short"]["windows"], plan["short"]["chunks"], 1, fade_f, dev)
    x = out = None
    try:
        x = _far_file(g, fill, tail, dev, copies=2)
        out = x.clone()
        ctx.patch_rate(x, sr, table, gen, filt, out, None, channel=c)
        xs = _upload(short, dev)
        outs = xs.clone()
        ctx.patch_rate(xs, sr, table_s, gen, filt, outs, None, channel=c)
        torch.cuda.synchronize()
        got = _download(out[g.n - k:], g.dtype)
        assert np.array_equal(got, _download(outs, g.dtype)), (gname, "the short call")
        gcol = got if c is None else got[:, c]
        scol = short if c is None else short[:, c]
        if g.dtype is far.S24:
            assert np.array_equal(gcol[~written], scol[~written]), gname
            lo, hi = S.store_f64(ref[written] - E[written]), S.store_f64(ref[written] + E[written])
            assert np.all((lo <= gcol[written]) & (gcol[written] <= hi)), (gname, int(((gcol[written] < lo) | (gcol[written] > hi)).sum()))
        else:
            check_patch(gcol, ref, E, written, scol, True, f"far {gname} patch_rate {sr} Hz")
        assert int((gcol[written] != scol[written]).sum()) > 600 and int((gcol[-5:] != scol[-5:]).sum()) >= 3
        if c is not None:
            others = [q for q in range(g.ch) if q != c]
            assert np.array_equal(got[:, others], short[:, others]), (gname, "another channel was written")
        assert _body_is_fill(out, g, fill, g.n - k) and _body_is_fill(x, g, fill, g.n - k), (gname, "the body changed")
        assert np.array_equal(_download(x[g.n - k:], g.dtype), short), (gname, "orig was written")
    finally:
        del x, out
        _free()


# ------------------------------------------------------------------------------------------------------------ the 22.05 kHz recording
@pytest.mark.parametrize("fi", [0, 1], ids=FILLS)
def test_cut_clips_at_the_cap_of_the_22050_hz_axis(fi):
    """si_cut_clips and si_cut_clips_valid on an fp32 recording of SI_MAX_REC samples (R22): a clip that ends with the recording, one a
    thousand samples earlier and one across the body's end.  The plain rows are the short file's slices bit for bit -- NaN payloads and
    infinities included; the _valid rows are tests/invalid_ref.py's `clean` of them: NaN, inf and over-ceiling samples, the last two of
    the recording among them, as +0.0."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    g = far.GEOMETRIES["R22"]
    fill, tail, shift = far.fills(g.dtype)[fi], far.tail(g, "invalid"), far.shift_of(g.n)
    short = far.short_file(tail, fill)
    L, ceil = 2049, far.ceiling(g.dtype)
    starts = [Z + K - L, Z + K - L - 1000, Z - 100]
    want = np.stack([short[s:s + L] for s in starts])
    want_valid = np.stack([IV.clean(short, ceil)[s:s + L] for s in starts])
    assert not np.isfinite(want[0, -2:]).any() and np.isnan(want[0]).any() and float(np.nanmax(np.abs(want_valid))) <= ceil
    x = None
    try:
        x = _far_file(g, fill, tail, dev)
        got = ctx.cut_clips(x, [s + shift for s in starts], L)
        got_valid = ctx.cut_clips_valid(x, [s + shift for s in starts], L, ceil)
        xs = _upload(short, dev)
        torch.cuda.synchronize()
        assert starts[0] + shift + L == g.n
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(got_valid.cpu().numpy().view(np.int32), want_valid.view(np.int32))
        assert torch.equal(_bits(got), _bits(ctx.cut_clips(xs, starts, L))) and torch.equal(_bits(got_valid), _bits(ctx.cut_clips_valid(xs, starts, L, ceil)))
        assert _body_is_fill(x, g, fill, g.n - K)
    finally:
        del x
        _free()


def test_patch_regions_at_the_cap_of_the_22050_hz_axis():
    """si_patch_regions on R22 under the constant fill: one span of 700 samples that ends with the recording, a ramp of 110 in front,
    its generator row reaching the recording's last sample, a gain.  Where the weight is 1 the output is fl32(gain * gen) bit for bit;
    on the ramp it lies inside tests/rate_ref.py's `blend` bound (the same blend, tests/test_gpu_rate.py's check); every other sample
    of `out` -- the whole body by one device reduction -- and all of `orig` keep their bits."""
    eng = _engine()
    ctx, dev = eng.ctx, eng.device
    g = far.GEOMETRIES["R22"]
    fill, tail, shift, fade = far.fills(g.dtype)[1], far.tail(g, "dead"), far.shift_of(g.n), 110
    short = far.short_file(tail, fill)
    k, l = Z + K, 700
    s = k - l
    ws = s - fade - 3
    gen_host = ((torch.rand(1, k - ws + 5, generator=torch.Generator().manual_seed(5)) * 2 - 1) * 0.3).contiguous()
    gain_host = np.array([0.8], dtype=np.float32)
    w, owner = RR.weights([(s, l, 0, k)], fade, k)
    it = {"w": w, "owner": owner, "y": np.zeros(k), "A": np.zeros(k), "ctx": np.zeros(k, dtype=np.int64)}
    it["y"][ws:] = gen_host[0, :k - ws].numpy().astype(np.float64)
    it["A"][ws:] = np.abs(it["y"][ws:])
    ref, E, written = RR.blend(short, it, gain_host)
    assert written.sum() == l + fade and written[-1] and (w[s:] == 1).all() and 0 < w[s - 1] < 1

    def table(off, n):
        region = G.region_chunks(G.file_regions([(s + off, l)], [n], fade))
        return native.RegionTable([(s + off, l, 0, n)], [(0, ws + off, n - ws - off)], region, 1, fade, dev)

    gen, gain = gen_host.to(dev), torch.from_numpy(gain_host).to(dev)
    x = out = None
    try:
        x = _far_file(g, fill, tail, dev, copies=2)
        out = x.clone()
        ctx.patch_regions(x, table(shift, g.n), gen, gain, out)
        xs = _upload(short, dev)
        outs = xs.clone()
        ctx.patch_regions(xs, table(0, k), gen, gain, outs)
        torch.cuda.synchronize()
        got = out[g.n - k:].cpu().numpy()
        assert np.array_equal(got.view(np.int32), outs.cpu().numpy().view(np.int32)), "the short call"
        want = (gain_host[0] * gen_host[0, s - ws:k - ws].numpy()).astype(np.float32)
        assert np.array_equal(got[s:].view(np.int32), want.view(np.int32)) and float(np.abs(want[-5:]).max()) > 0
        check_patch(got, ref, E, written, short, False, "far R22 patch_regions")
        assert _body_is_fill(out, g, fill, g.n - k) and _body_is_fill(x, g, fill, g.n - k), "the body changed"
        assert np.array_equal(x[g.n - k:].cpu().numpy().view(np.int32), short.view(np.int32)), "orig was written"
    finally:
        del x, out
        _free()


# ------------------------------------------------------------------------------------------------------------ one route
def test_conceal_file_route_at_the_far_end():
    """engine.conceal_file on E31 under the constant fill, kind "invalid" (the body is valid), detect="each", feed="contexts"
    with clips16="file" (both clip sets cut straight from the file by si_cut_pair: no copy of the file's length but the output), mend_ms = 1, the tiny engine of the other route tests: a tail of 300 frames of speech whose last channel holds single clipped
    samples and a clipped block of 10 frames, and whose first channel holds two singles.  The gaps, skipped and mended lists are the
    short file's moved by the shift (a whole number of 20 ms frames), the output's tail equals the short run's bit for bit and the
    body keeps its fill: the Python arithmetic between the kernels -- runs_to_gaps, the region and chunk tables, the frame indices --
    at positions near 2^28 sample times and element offsets near 2^31."""
    from speech_inpainting_amd import synth
    eng = _engine()
    dev = eng.device
    g = far.GEOMETRIES["E31"]
    need = 3 * g.bytes + GIB                                           # the file, the mended copy and `patched`
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"E31 route: {need / GIB:.1f} GiB of device memory needed, {free / GIB:.1f} GiB free")
    sr, per, frames, lead_f = 48000, 960, 300, 100
    kt = frames * per + 77
    lead = lead_f * per + (g.n - lead_f * per - kt) % per
    shift = g.n - lead - kt
    assert shift % per == 0 and lead >= 75 * per
    shift_f = shift // per
    fill = far.fills(g.dtype)[1]
    tail = np.stack([(synth.synth_wave(1, kt, 60 + c, sr=sr)[0] * 20000.0).to(torch.int16).numpy() for c in range(g.ch)], axis=1)
    singles = [(8 + 9 * i) * per + 10 + 37 * i for i in range(10)] + [(200 + 9 * i) * per + 500 for i in range(8)]
    tail[singles, g.ch - 1] = 32767
    tail[120 * per:130 * per, g.ch - 1] = 32767
    tail[[50 * per + 5, 250 * per + 7], 0] = 32767
    tail = np.ascontiguousarray(tail)
    short = np.ascontiguousarray(np.concatenate([np.full((lead, g.ch), fill, np.int16), tail]))
    kw = dict(min_ms=0, kind="invalid", feed="contexts", clips16="file", detect="each", mend_ms=1.0, clip_frames=75, min_context=15, merge_frames=1)
    want = eng.conceal_file(torch.from_numpy(short).to(dev), sr, 32766.0, **kw)
    torch.cuda.synchronize()
    assert len(want["gaps"][g.ch - 1]) == 1 and want["gaps"][g.ch - 1][0][0] == lead // per + 120 and len(want["mended"][g.ch - 1]) == 18 and len(want["mended"][0]) == 2
    assert all(st == native.MEND_AR for rows in want["mended"] for _, _, st in rows) and want["gaps"][1:g.ch - 1] == [[]] * (g.ch - 2)
    x = got = body = None
    try:
        x = torch.zeros((g.n, g.ch), dtype=torch.int16, device=dev)
        x.fill_(fill.item())
        x[g.n - kt:] = torch.from_numpy(tail).to(dev)
        got = eng.conceal_file(x, sr, 32766.0, **kw)
        torch.cuda.synchronize()
        assert got["gaps"] == [[(f + shift_f, c) for f, c in rows] for rows in want["gaps"]]
        assert got["skipped"] == [[(f + shift_f,) + tuple(rest) for f, *rest in rows] for rows in want["skipped"]]
        assert got["mended"] == [[(s + shift, m, st) for s, m, st in rows] for rows in want["mended"]]
        assert torch.equal(got["patched"][g.n - lead - kt:], want["patched"]), "the tail of the output"
        body = got["patched"][:g.n - kt]
        lo, hi = torch.aminmax(body)
        assert lo.item() == hi.item() == fill.item(), "the body changed"
        changed = int((want["patched"].cpu() != torch.from_numpy(short)).sum())
        assert changed > 10 * per // 2 + 20
    finally:
        del x, got, body
        _free()
