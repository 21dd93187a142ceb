"""tests/far.py on the CPU: what tests/test_gpu_far.py stands on.

1. The shift law from the references alone: for a mid-sized "far" file of about 3 * 2^16 sample times every reference gives
   ref(far) == lift(ref(short)) -- both fills, mono, one channel and joint, every detector and parameter set, mend and the cutters.
   That is the condition that lets the GPU tests leave the body out of the reference.
2. No level or burst case has an undecided sample (Case.undecided of tests/level_ref.py and tests/burst_ref.py).
3. The tests can fail: a reader whose element offset wrapped to int32 or to uint32, or whose packed 24-bit byte offset 3 e wrapped to
   uint32, gives another result than the expectation at every geometry that crosses that boundary, and a writer's footprint differs.
4. The geometry table's own asserts: what each geometry crosses, the phase of the shifts, Z against the largest reach, N22 of LOW."""
import functools

import numpy as np
import pytest

from speech_inpainting_amd import gaps as G
from tests import far
from tests import feed_ref as F
from tests import mend_ref as M
from tests import pair_ref as PR

MID = 3 * 2 ** 16
DET_CASES = [(g, d) for g in far.DETECTOR_GEOMETRIES for d in far.DETECTORS]


def _mid_file(tail, fill, shift, lead=far.Z):
    return far.short_file(tail, fill, lead + shift)


@functools.lru_cache(maxsize=None)
def _short_rows(gname, det):
    """{(fill index, parameter index, channel): the reference's rows on the short file}, computed once."""
    g = far.GEOMETRIES[gname]
    t = far.detector_tail(g, det)
    out = {}
    for fi, fill in enumerate(far.fills(g.dtype)):
        x = far.short_file(t, fill)
        for pi, p in enumerate(far.detector_params(det, g.dtype)):
            for c in far.channels_of(g):
                out[fi, pi, c] = far.reference_rows(det, p, x, c)
    return out


# ------------------------------------------------------------------------------------------------------------ 1: the shift law
@pytest.mark.parametrize("gname,det", DET_CASES)
def test_shift_law_of_the_detectors(gname, det):
    g = far.GEOMETRIES[gname]
    t = far.detector_tail(g, det)
    shift = MID - far.Z - far.K
    want = _short_rows(gname, det)
    bodies = 0
    for fi, fill in enumerate(far.fills(g.dtype)):
        mid = _mid_file(t, fill, shift)
        assert mid.shape[0] == MID
        for pi, p in enumerate(far.detector_params(det, g.dtype)):
            dead = far.fill_is_dead(det, p, fill)
            bodies += dead
            for c in far.channels_of(g):
                got = far.reference_rows(det, p, mid, c)
                lifted = far.lift(want[fi, pi, c], shift, dead)
                assert np.array_equal(got, lifted), (gname, det, fi, p, c, got[:4].tolist(), lifted[:4].tolist())
                assert len(lifted) > int(dead), (gname, det, fi, p, c, "the tail holds no run")
    assert bodies > 0 or det in ("burst", "invalid")


def test_lift_moves_rows_and_stretches_the_body_s_run():
    rows = np.array([[0, far.Z + 3], [far.Z + 10, 4], [far.Z + far.K - 2, 2]])
    assert far.lift(rows, 1000, True).tolist() == [[0, far.Z + 1003], [far.Z + 1010, 4], [far.Z + far.K + 998, 2]]
    assert far.lift(rows[1:], 1000, False).tolist() == [[far.Z + 1010, 4], [far.Z + far.K + 998, 2]]
    assert far.lift(np.zeros((0, 2)), 5, False).shape == (0, 2)
    for bad, dead in ((rows, False), (rows[1:], True), (np.array([[0, 5]]), True)):      # a body run nobody expects, none where one is, a short one
        with pytest.raises(AssertionError):
            far.lift(bad, 1000, dead)
    cap = far.GEOMETRIES["CAP"].n
    top = far.lift(rows, far.shift_of(cap), True)                      # the top of int32: lengths and ends stay below 2^31
    assert top.dtype == np.int32 and top[0].tolist() == [0, cap - far.K + 3] and int(top[-1].sum()) == cap


@pytest.mark.parametrize("gname", far.MEND_GEOMETRIES)
@pytest.mark.parametrize("edge", [False, True], ids=["mended", "edge"])
def test_shift_law_of_mend(gname, edge):
    """The statuses and the unrounded results of every row are the short file's, the last row AR at e + K == n and EDGE at n + 1."""
    g = far.GEOMETRIES[gname]
    t, rows = far.mend_case(g, edge)
    c = far.mend_channel(g)
    shift = MID - far.Z - far.K
    for fill in far.fills(g.dtype):
        short, mid = far.short_file(t, fill), _mid_file(t, fill, shift)
        a = M.mend(short, [(s + far.Z, m) for s, m in rows], channel=c, **far.MEND)
        b = M.mend(mid, [(s + far.Z + shift, m) for s, m in rows], channel=c, **far.MEND)
        assert a.status.tolist() == b.status.tolist() == [M.AR] * 4 + [M.EDGE if edge else M.AR]
        assert all((u is None and v is None) or list(u) == list(v) for u, v in zip(a.u, b.u))
        assert np.array_equal(a.y[far.Z:].view(np.uint8), b.y[far.Z + shift:].view(np.uint8)) and bool(np.all(b.y[:far.Z + shift] == fill))
        last = rows[-1][0] + far.Z
        col = (lambda y: y) if short.ndim == 1 else (lambda y: y[:, c])
        assert (col(a.y)[last:last + 4].tobytes() == col(short)[last:last + 4].tobytes()) == edge      # EDGE leaves the file untouched


@pytest.mark.parametrize("gname", far.CUT_GEOMETRIES)
def test_shift_law_of_the_cutters(gname):
    """si_cut_rate's and si_cut_pair's references on a mid-sized file whose shift is a whole number of Q file samples (of 20 ms frames):
    the same float64 values as on the short file, bit for bit."""
    g = far.GEOMETRIES[gname]
    t = far.tail(g, "dead")
    c = None if g.ch == 1 else g.ch - 1
    for sr in far.cut_rates(g):
        plan = far.cut_plan(g, sr)
        P, Q = plan["P"], plan["Q"]
        shift = (MID - plan["k"]) // Q * Q
        for fill in far.fills(g.dtype):
            short, mid = far.column(far.short_file(t, fill, plan["lead"]), c), far.column(_mid_file(t, fill, shift, plan["lead"]), c)
            ys, As, _ = F.clips(short, sr, plan["short"], plan["L"])
            ym, Am, _ = F.clips(mid, sr, [s + shift // Q * P for s in plan["short"]], plan["L"])
            assert np.array_equal(ys, ym) and np.array_equal(As, Am) and float(np.abs(ys[0, -8:]).max()) > 0
            assert plan["short"][0] + plan["L"] == F.n22(short.size, sr)
        pp = far.pair_plan(g, sr)
        per = sr // 50
        shift = (MID - pp["k"]) // per * per
        fill = far.fills(g.dtype)[1]
        short, mid = far.column(far.short_file(t, fill, pp["lead"]), c), far.column(_mid_file(t, fill, shift, pp["lead"]), c)
        a = PR.clips(short, sr, pp["short"], pp["L22"], pp["L16"])
        b = PR.clips(mid, sr, [f + shift // per for f in pp["short"]], pp["L22"], pp["L16"])
        assert all(np.array_equal(a[key], b[key]) for key in ("y22", "A22", "y16", "A16"))
        assert 441 * pp["short"][0] + pp["L22"] == pp["N22s"] and 320 * pp["short"][0] + pp["L16"] == pp["lims"]


# ------------------------------------------------------------------------------------------------------------ 2: no undecided case
@pytest.mark.parametrize("gname", far.DETECTOR_GEOMETRIES)
@pytest.mark.parametrize("det", ["level", "burst"])
def test_no_level_or_burst_case_is_undecided(det, gname):
    g = far.GEOMETRIES[gname]
    t = far.detector_tail(g, det)
    for fill in far.fills(g.dtype):
        x = far.short_file(t, fill)
        for p in far.detector_params(det, g.dtype):
            for c in far.channels_of(g):
                assert far.undecided(det, p, x, c) == [], (gname, det, float(fill), p, c)


# ------------------------------------------------------------------------------------------------------------ 3: the tests can fail
def _whole_tail(g, wrap):
    """Does every element of the tail wrap (not only the last sample times)?"""
    first = (g.n - far.K) * g.ch
    return {"int32": first >= 2 ** 31, "uint32": first >= 2 ** 32, "bytes24": 3 * first >= 2 ** 32}[wrap]


@pytest.mark.parametrize("gname,det", DET_CASES)
def test_a_wrapped_reader_changes_the_detectors_rows(gname, det):
    """Per geometry, boundary it crosses, fill and channel argument: the wrapped reader's rows differ from the expectation under at least
    one parameter set of the detector, and under EVERY set when the whole tail lies past the boundary.  (Where only the last three or
    five sample times wrap, half = 1024 cannot tell: they are 5 of 2049 squares.  half = 0 and 1 can.)"""
    g = far.GEOMETRIES[gname]
    t = far.detector_tail(g, det)
    want = _short_rows(gname, det)
    wraps = [w for w in far.WRAPS if g.crosses(w)]
    assert wraps or gname == "CAP"
    for w in wraps:
        for fi, fill in enumerate(far.fills(g.dtype)):
            x = far.seen(g, t, fill, w)
            assert x.shape == far.short_file(t, fill).shape and not np.array_equal(x.view(np.uint8), far.short_file(t, fill).view(np.uint8))
            for c in far.channels_of(g):
                differs = [not np.array_equal(far.reference_rows(det, p, x, c), want[fi, pi, c]) for pi, p in enumerate(far.detector_params(det, g.dtype))]
                assert any(differs) and (all(differs) or not _whole_tail(g, w)), (gname, det, w, fi, c, differs)


@pytest.mark.parametrize("gname", far.MEND_GEOMETRIES)
def test_a_wrapped_reader_and_writer_change_mend(gname):
    """The row at e + K == n reads the file's last sample times: a wrapped reader fills it with other samples.  A wrapped writer's
    footprint differs wherever a filled run lies past the boundary -- K >= 8 keeps every run below sample time n - 8, so that is the
    case at E32 (int32) and S24 (the bytes) and cannot be at E31 and F32, whose last five / three sample times alone lie past 2^31, nor
    at E32 for uint32.  W32, with 64 sample times past 2^32, is there for that: its last row's stores lie past 2^32."""
    g = far.GEOMETRIES[gname]
    t, rows = far.mend_case(g, False)
    c = far.mend_channel(g)
    fill = far.fills(g.dtype)[1]
    table = [(s + far.Z, m) for s, m in rows]
    want = M.mend(far.short_file(t, fill), table, channel=c, **far.MEND)
    for w in [w for w in far.WRAPS if g.crosses(w)]:
        got = M.mend(far.seen(g, t, fill, w), table, channel=c, **far.MEND)
        assert got.status.tolist() != want.status.tolist() or not np.array_equal(got.y[far.Z:].view(np.uint8), want.y[far.Z:].view(np.uint8)), (gname, w)
        times = np.concatenate([np.arange(s, s + m) for s, m in rows]) + g.n - far.K
        moved = not np.array_equal(far.footprint(g, times, c or 0, w), far.true_footprint(g, times, c or 0, w))
        assert moved == ((gname, w) in (("E32", "int32"), ("W32", "int32"), ("W32", "uint32"), ("S24", "bytes24"))), (gname, w, moved)
    assert [w for w in far.WRAPS if g.crosses(w)] or gname in ("CAP", "M24", "M32")


@pytest.mark.parametrize("gname", ["E31", "S24"])
def test_a_wrapped_reader_changes_the_clips_and_a_wrapped_writer_the_patch(gname):
    g = far.GEOMETRIES[gname]
    t = far.tail(g, "dead")
    c = g.ch - 1
    fill = far.fills(g.dtype)[1]
    for sr in far.cut_rates(g):
        plan = far.cut_plan(g, sr)
        want, _, _ = F.clips(far.column(far.short_file(t, fill, plan["lead"]), c), sr, plan["short"][:1], plan["L"])
        for w in [w for w in far.WRAPS if g.crosses(w)]:
            got, _, _ = F.clips(far.column(far.seen(g, t, fill, w, plan["lead"]), c), sr, plan["short"][:1], plan["L"])
            assert not np.array_equal(got.astype(np.float32), want.astype(np.float32)), (gname, sr, w)
            times = np.arange(g.n - 700, g.n)                          # the patched span ends with the file
            assert not np.array_equal(far.footprint(g, times, c, w), far.true_footprint(g, times, c, w)), (gname, w)


# ------------------------------------------------------------------------------------------------------------ 4: the table
def test_the_geometry_table():
    assert far.check_geometries()
    assert far.Z >= max(far.REACH.values()) and far.REACH["detect"] == 2 * G.LEVEL_MAX_HALF + 1 and far.REACH["mend"] >= M.MAX_CONTEXT
    assert far.MEND["context"] <= far.REACH["mend"] and far.K > far.CHUNK + far.REACH["detect"]
    for g in far.GEOMETRIES.values():
        assert far.lead_of(g.n) == far.Z and far.shift_of(g.n) == g.n - far.Z - far.K > 2 ** 27
        assert 0 < far.last_seam(g.n) < far.K and (g.n - far.K + far.last_seam(g.n)) % far.CHUNK == 0
    for gname in far.CUT_GEOMETRIES:
        g = far.GEOMETRIES[gname]
        for sr in far.cut_rates(g):
            plan, pp = far.cut_plan(g, sr), far.pair_plan(g, sr)
            assert plan["shift"] % plan["Q"] == 0 and pp["shift"] % (sr // 50) == 0 and max(F.reach(sr), PR.reach(sr, 16000)) <= far.REACH["cut"]
            assert plan["N22"] <= far.MAX_REC and plan["starts"][0] + plan["L"] == plan["N22"] and plan["starts"][1] + far.TILE > plan["starts"][0]
            assert plan["lead"] < far.Z + plan["Q"] and pp["lead"] < far.Z + sr // 50
    low = far.cut_plan(far.GEOMETRIES["LOW"], 16000)
    assert far.MAX_REC - 2 < low["N22"] <= far.MAX_REC                 # the 22.05 kHz axis at its cap while n is not
    assert far.cut_plan(far.GEOMETRIES["CAP"], 48000)["N22"] < 2 ** 30


def test_the_fills_and_the_tails():
    """|fill| lies below the tail's peak, the peak is in every channel, and the constant is above every absolute threshold."""
    for gname in far.DETECTOR_GEOMETRIES:
        g = far.GEOMETRIES[gname]
        zero, const = far.fills(g.dtype)
        assert float(zero) == 0.0 and 0 < float(const) < float(far.peak_of(g.dtype)) < far.ceiling(g.dtype)
        for det in far.DETECTORS:
            t = far.detector_tail(g, det).reshape(far.K, -1)
            finite = np.where(np.isfinite(t.astype(np.float64)), np.abs(t.astype(np.float64)), 0.0)
            if det != "invalid":
                assert np.all(finite.max(axis=0) == float(far.peak_of(g.dtype))), (gname, det)
            for p in far.detector_params(det, g.dtype):
                if det in ("quiet", "dead", "level") and "thr" in p:
                    assert p["thr"] < float(const)
            c = t[:, -1]
            assert np.any(c[-3:] != c[-1]) or det == "invalid"         # damage and intact samples among the last three of the last channel


@pytest.mark.parametrize("gname", far.DETECTOR_GEOMETRIES)
def test_a_held_run_crosses_the_far_file_s_last_chunk_seam(gname):
    """For every channel argument the tests run, under both fills: the HELD reference has a row with start < seam < start + len, the seam
    being the first sample time of the far file's last chunk -- the link into the last, partial chunk is exercised on every load route."""
    g = far.GEOMETRIES[gname]
    t = far.detector_tail(g, "dead")
    seam = far.Z + far.last_seam(g.n)
    assert (far.shift_of(g.n) + seam) % far.CHUNK == 0 and seam < far.Z + far.K
    for fill in far.fills(g.dtype):
        x = far.short_file(t, fill)
        for c in far.channels_of(g):
            rows = far.reference_rows("dead", dict(kind="held"), x, c)
            assert any(s < seam < s + m for s, m in rows.tolist()), (gname, float(fill), c, rows[-3:].tolist(), seam)
