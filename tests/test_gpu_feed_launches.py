"""What the file feeds and si_patch_rate do per route, in one place.  tests/feed_cases.py builds the calls: every
feed with and without a ceiling and si_patch_rate, on one file of 3001 sample times at 48 / 44.1 / 16 / 8 kHz in fp32, int16 and packed
24-bit, as (n,), (n, 1) with channel 0 and (n, 2) with channel 1.  Per call:
    the sha256 of the output tensors' bytes equals the digest recorded in tests/golden/feed_launches.json (tools/record_feed_launches.py,
        on an MI355X): the kernels hold no atomics and write each output once, so there is no tolerance.  The float64 references stay
        the authority on what the bytes should be (tests/test_gpu_feed.py, test_gpu_pair.py, test_gpu_rate.py, test_gpu_invalid_feed.py);
        this file holds them still;
    the three layouts of one file give the same output bytes, the ceiling changes them, and (n, 2) leaves channel 0 alone;
    the profile is exactly one launch of the route's family -- cut_rate, cut_rate_ch, patch_rate, patch_rate_ch, cut_clips; a _valid call
        reports under the plain name and takes an (n, 1) file as the mono file -- and its flops and bytes equal the launcher's model,
        written out in tests/feed_cases.py from C, L, H, cap, the element size and the grid.
The refusals: for each of the eleven entry points and each pair of consecutive refusals in its order, one call wrong in both is refused
with the EARLIER one's text under the entry's own name, and launches nothing.  (Two refusals of one argument that exclude each other --
sr below 4000 and sr = 22050 -- merge into the earlier one alone.)  C = 0, and an empty rate table, are served and launch nothing."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from speech_inpainting_amd import native
from tests import feed_cases as FC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feed_launches.json")
_GOLD = {}


def _golden():
    if not _GOLD:
        with open(GOLDEN) as f:
            _GOLD.update(json.load(f))
    return _GOLD


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("group", sorted(FC.groups()))
def test_bits_profile_flops_and_bytes_of_every_route(group):
    eng = FC.engine()
    gold = _golden()
    same, n = {}, 0
    for key, call, model in FC.groups()[group](eng):
        outs, prof = FC.profiled(eng.ctx, call)
        torch.cuda.synchronize()
        print(key, prof)
        assert prof == model, (key, prof, model)
        got = FC.digest(*outs)
        assert got == gold[key], (key, got, gold[key])
        parts = key.split("/")
        if parts[0] == "patch_rate":                                   # the repaired channel; channel 0 of the interleaved file keeps its bytes
            channel = FC.LAYOUTS[parts[3]][1]
            got = FC.digest(outs[0] if channel is None else outs[0][:, channel].contiguous())
            if channel == 1:
                kept = outs[0][:, 0].cpu().numpy()
                assert np.array_equal(FC.S.unpack(kept) if parts[2] == "s24" else kept, FC.column(parts[2], int(parts[1]), 1)), key
        same.setdefault(tuple(p for p in parts if p not in FC.LAYOUTS), set()).add(got)
        n += 1
    assert n > 0 and all(len(v) == 1 for v in same.values()), (group, {k: len(v) for k, v in same.items()})
    plain = {k: v for k, v in same.items() if k[-1] == "plain"}
    for k, v in plain.items():                                         # the file holds samples the ceiling makes invalid
        assert v != same[k[:-1] + ("ceiling",)], k


def test_the_fixture_names_these_calls_and_no_others():
    keys = [key for make in FC.groups().values() for key, _, _ in make(FC.engine())]
    assert sorted(keys) == sorted(_golden()) and len(set(keys)) == len(keys) == 2 * 4 * 18 + 4 * 9 + 2


# ------------------------------------------------------------------------------------------------------------ 2
SR = 48000
INF = float("inf")
CHANNELS = [(dict(channels=9), "channels = 9, outside 1 .. SI_MAX_CHANNELS = 8"), (dict(channel=2), "channel = 2, outside 0 .. 1")]
CEILING = [(dict(ceiling=0.0), "ceiling = 0 is not above 0, or is NaN")]
RATE = [(dict(sr=3999), "sr = 3999 Hz, outside 4000 .. 192000"), (dict(sr=22050), "sr = 22050 Hz is the model's own rate: that file is si_cut_clips'"),
        (dict(n=0), "n_file = 0"), (dict(n=2 ** 31 - 1), "n_file = 2147483647 samples, at most [0-9]+")]
TOO_LONG = (dict(sr=8000, n=2 ** 30), "n_file = 1073741824 samples at 8000 Hz are [0-9]+ samples at 22050 Hz, at most")
CUT_RATE = RATE + [TOO_LONG, (dict(f=dict(size=-8)), "filt: si_sinc_filter size mismatch"),
                   (dict(f=dict(num_table=0)), r"filt: bad filter table \(nwin [0-9]+, num_table 0,"),
                   (dict(f=dict(step="cap")), "filt: bad filter table: [0-9]+ taps per wing at [0-9]+ Hz need [0-9]+ staged samples per tile, at most 16384"),
                   (dict(C=-1), r"C = -1 clips in one call, 0 .. 65535 \(the launch grid's second dimension\)"), (dict(L=0), "L = 0"),
                   (dict(x=False), "x is NULL"), (dict(out=False), "out is NULL"), (dict(host=False), "host_start is NULL"),
                   (dict(dev=False), "start is NULL"),
                   (dict(table=(0, -1)), r"start\[1\]: clip = 22.05 kHz samples \[-1, 99\) is outside the recording's [0-9]+ samples")]
CUT_PAIR = RATE + [(dict(f=dict(size=-8)), "filt22: si_sinc_filter size mismatch"), (dict(f=dict(num_table=0)), r"filt22: bad filter table \(nwin [0-9]+, num_table 0,"),
                   (dict(f=dict(step=1)), "filt22: bad filter table: [0-9]+ taps per wing at [0-9]+ Hz, no tile's staged samples fit 64 KB"), TOO_LONG,
                   (dict(f16=None), "filt16 is NULL at sr = [0-9]+ Hz: only a 16000 Hz file goes without the 16 kHz filter"),
                   (dict(f16=dict(size=-8)), "filt16: si_sinc_filter size mismatch"), (dict(f16=dict(num_table=0)), r"filt16: bad filter table \(nwin [0-9]+, num_table 0,"),
                   (dict(f16=dict(step=1)), "filt16: bad filter table: [0-9]+ taps per wing at [0-9]+ Hz, no tile's staged samples fit 64 KB"),
                   (dict(f=dict(step="cap")), "filt22: bad filter table: [0-9]+ taps per wing at [0-9]+ Hz need [0-9]+ staged samples per tile, at most 16384"),
                   (dict(C=-1), r"C = -1 clips in one call, 0 .. 65535 \(the launch grid's second dimension\)"), (dict(L=0), "L22 = 0"),
                   (dict(L16=0), "L16 = 0"), (dict(x=False), "x is NULL"), (dict(out=False), "out22 is NULL"), (dict(out16=False), "out16 is NULL"),
                   (dict(host=False), "host_frame is NULL"), (dict(dev=False), "frame is NULL"),
                   (dict(table=(-1, 0)), r"frame\[0\] = -1: clip = 22.05 kHz samples \[-441, -341\) is outside the recording's [0-9]+ samples"),
                   (dict(L16=2000), r"frame\[0\] = 0: clip = 16 kHz samples \[0, 2000\) ends past ceil\(N22 320 / 441\) = [0-9]+ \(N22 = [0-9]+\)")]
CUT_CLIPS = [(dict(x=False), "NULL / empty argument"), (dict(n=2 ** 31 - 1), "a source of 2147483647 samples, at most [0-9]+"),
             (dict(C=65536), r"65536 clips in one call, at most 65535 \(the launch grid's second dimension\)")]
CLIP = [(dict(table=(0, -1)), r"clip 1 = samples \[-1, 99\) is outside the source's [0-9]+ samples")]
PATCH = [(dict(x=False), "NULL / empty argument"), (dict(out="orig"), r"out is orig \(orig is read while out is written\)"), RATE[0],
         (dict(sr=22050), "sr = 22050 Hz is the generator's own rate: that file is si_patch_regions'"),
         (dict(n=2 ** 31 - 1), "a file of 2147483647 samples, at most [0-9]+"),
         (dict(sr=8000, n=2 ** 30), "1073741824 samples at 8000 Hz are [0-9]+ samples at 22050 Hz, at most"),
         (dict(f=dict(size=-8)), "si_sinc_filter size mismatch"), (dict(f=dict(num_table=0)), r"bad filter table \(nwin [0-9]+, num_table 0,"),
         (dict(f=dict(step="cap")), "bad filter table: [0-9]+ taps per wing at [0-9]+ Hz need [0-9]+ staged samples per chunk, at most 16384"),
         (dict(ts=dict(struct_size=8)), "si_rate_table size mismatch"), (dict(ts=dict(fade=-1)), "fade of -1 samples is negative or too long"),
         (dict(ts=dict(num_windows=-1)), "rate table with 1 contexts / -1 windows / 1 spans / 2 chunks"), (dict(ts=dict(ramp=None)), "rate table with NULL ramp"),
         (dict(gen=False), "1 windows but NULL window arrays / generator rows"), (dict(ts=dict(host_start=None)), "1 spans but NULL span arrays"),
         (dict(ts=dict(host_chunk=None)), "2 chunks but NULL chunk arrays"), (dict(windows="names context 5"), "window 0 names context 5 of 1")]
ORDER = {
    "si_cut_rate": CUT_RATE, "si_cut_rate_ch": CHANNELS + CUT_RATE, "si_cut_rate_valid": CHANNELS + CEILING + CUT_RATE,
    "si_cut_pair": CUT_PAIR, "si_cut_pair_ch": CHANNELS + CUT_PAIR, "si_cut_pair_valid": CHANNELS + CEILING + CUT_PAIR,
    "si_cut_clips": CUT_CLIPS + CLIP, "si_cut_clips_valid": CUT_CLIPS + CEILING + CLIP,
    "si_patch_rate": PATCH, "si_patch_rate_ch": CHANNELS + PATCH,
}


def _table_pairs(spans, windows, chunks, N22):
    """si_patch_rate's checks of the table's rows, from `window names context` on: per pair of consecutive refusals the rows wrong in
    both, and the earlier one's text."""
    (s, l, _, n), (_, ws, wl, _) = spans[0], windows[0]
    return [
        (dict(windows=[(5, -1, wl, N22)]), "window 0 names context 5 of 1"),
        (dict(windows=[(0, ws, N22 + 5, ws)]), r"window 0 = 22.05 kHz samples \[[0-9]+, \+[0-9]+\) is outside the recording \([0-9]+ samples, rows of [0-9]+\)"),
        (dict(windows=[(0, ws, wl, ws)], chunks=[(99, 0, 1)]), "window 0 starts at 22.05 kHz sample [0-9]+, its context's audio ends at [0-9]+ of [0-9]+"),
        (dict(chunks=[(1, 0, 1), (-1, 0, 1)]), "chunk entry 1 names chunk -1, at or past the file's [0-9]+ samples"),
        (dict(chunks=[(1, 0, 1), (0, 2, 1)]), "chunk entry 1 names chunk 0 after chunk 1: not strictly increasing"),
        (dict(chunks=[(0, 0, 5)], spans=[(-1, l, 0, n)]), r"chunk entry 0 walks spans \[0, 5\) of 1"),
        (dict(spans=[(-1, 100, 0, n), (50, 10, 0, n)], chunks=[(0, 0, 2)]), r"span 0 = samples \[-1, \+100\) with lim [0-9]+ does not lie in the file's [0-9]+ samples"),
        (dict(spans=[(100, 100, 0, n), (150, 10, 7, n)]), "span 1 starts at 150, before span 0 ends: unsorted or overlapping"),
        (dict(spans=[(100, 50, 7, n), (300, 50, 0, n)], windows=[(0, 0, wl, 5)]), "span 0 names window 7 of 1"),
        (dict(windows=[(0, ws + 50, wl, ws + 51)]), "span 0 writes up to file sample [0-9]+ = 22.05 kHz sample [0-9]+, its context's audio ends at [0-9]+"),
        (dict(windows=[(0, ws + 50, wl, N22)], chunks=[(0, 0, 1)]),
         r"span 0 blends file samples \[[0-9]+, [0-9]+\) and reads 22.05 kHz samples \[[0-9]+, [0-9]+\), its window's row holds \[[0-9]+, [0-9]+\)"),
        (dict(chunks=[(1, 0, 0)]), r"span 0 blends samples \[[0-9]+, [0-9]+\), the chunk list lacks chunk 0"),
    ]


def _merged(good, first, second):
    """good with both overrides, the first's value where they name the same argument; filter and table fields merge."""
    args = {**good, **second, **first}
    for k in ("f", "f16", "ts"):
        if isinstance(first.get(k), dict) and isinstance(second.get(k), dict):
            args[k] = {**second[k], **first[k]}
    return args


def test_the_earlier_refusal_wins_and_nothing_is_launched():
    eng = FC.engine()
    ctx, dev = eng.ctx, eng.device
    lib, h = ctx.lib, ctx._h
    f22, f16, frate = eng._feed_filter(SR), eng._feed_filter16(SR), eng._rate_filter(SR)
    spans, windows, chunks, lrow, N22 = FC.rate_table(SR, FC.reach(frate))
    x = torch.zeros(FC.N_FILE, 2, device=dev)
    outs = [torch.full((2, 100), 7.0, device=dev), torch.full((2, 80), 7.0, device=dev), torch.full((FC.N_FILE, 2), 7.0, device=dev)]
    gen = torch.zeros(1, lrow, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t, on=True: C.c_void_p(t.data_ptr()) if on else C.c_void_p(0)
    held = []
    assert windows[0][1] + 50 + windows[0][2] <= N22

    def sinc(tables, over):
        if over is None:
            return None
        nwin = tables["win"].numel()
        step = over.get("step", int(tables["step"]))
        step = max(1, nwin // 10000) if step == "cap" else step        # a third of the table's samples per wing: over 64 KB of LDS, under 16 385 taps
        assert over.get("step") != "cap" or 8192 < -(-nwin // step) <= 16384
        assert over.get("step") != 1 or nwin > 16384
        f = native.SincFilter(C.sizeof(native.SincFilter) + over.get("size", 0), nwin, over.get("num_table", int(tables["num_table"])), step, 0, 0,
                              float(tables["scale"]), 0.0, tables["win"].data_ptr(), tables["dwin"].data_ptr(), None)
        return C.byref(f)

    def invoke(fn, a):
        kind = fn[3:].replace("_ch", "").replace("_valid", "")
        file = (h, P(x, a["x"]), 0, a["n"]) + ((a["channels"], a["channel"]) if fn.endswith(("_ch", "_valid")) else ())
        ceil = (C.c_float(a["ceiling"]),) if fn.endswith("_valid") else ()
        host = np.ascontiguousarray(np.asarray(a["table"], dtype=np.int32))
        held.append(torch.from_numpy(host).to(dev))                   # read by the launch: kept until the test ends
        tab = (host.ctypes.data_as(C.c_void_p) if a["host"] else None, P(held[-1], a["dev"]), len(host) if a["C"] is None else a["C"])
        if kind == "cut_rate":
            return getattr(lib, fn)(*file, a["sr"], *tab, a["L"], sinc(f22, a["f"]), *ceil, P(outs[0], a["out"]), st)
        if kind == "cut_pair":
            return getattr(lib, fn)(*file, a["sr"], *tab, a["L"], a["L16"], sinc(f22, a["f"]), sinc(f16, a["f16"]), *ceil, P(outs[0], a["out"]),
                                    P(outs[1], a["out16"]), st)
        if kind == "cut_clips":
            return getattr(lib, fn)(h, P(x, a["x"]), a["n"], *tab, a["L"], *ceil, P(outs[0], a["out"]), st)
        rows = a["windows"] if a["windows"] != "names context 5" else [(5,) + windows[0][1:]]
        held.append(native.RateTable(a["spans"], rows, a["chunks"], 1, FC.FADE, dev))
        ts = held[-1].struct()
        for k, v in a["ts"].items():
            setattr(ts, k, v)
        return getattr(lib, fn)(*file, a["sr"], C.byref(ts), P(gen, a["gen"]), lrow, None, sinc(frate, a["f"]), P(x if a["out"] == "orig" else outs[2], True), st)

    good = dict(x=True, n=FC.N_FILE, channels=2, channel=1, sr=SR, host=True, dev=True, table=(0, 1), C=None, L=100, L16=80, f={}, f16={}, ceiling=0.5,
                out=True, out16=True, gen=True, ts={}, spans=spans, windows=windows, chunks=chunks)
    pairs = {}
    for fn, order in ORDER.items():
        both = [(_merged(good, first, second), msg) for (first, msg), (second, _) in zip(order, order[1:])]
        if "cut_pair" in fn:                                           # the 16 kHz file's own refusal, in front of the cap and C
            both.append(({**good, "sr": 16000, "C": -1}, "filt16 is not NULL at sr = 16000 Hz: the 16 kHz clips are the file's own samples, no filter is applied"))
        if "patch_rate" in fn:
            both += [({**good, **over}, msg) for over, msg in _table_pairs(spans, windows, chunks, N22)]
        for args, msg in both:
            rc, prof = FC.profiled(ctx, lambda: invoke(fn, args))
            err = lib.si_last_error(h).decode()
            assert rc == -1 and prof == {}, (fn, msg, rc, prof)
            assert re.match(re.escape(fn) + ": " + msg, err), (fn, msg, err)
        pairs[fn] = len(both)
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs), fn
        rc, prof = FC.profiled(ctx, lambda: invoke(fn, good))          # the same arguments, none of them wrong, are served: one launch
        assert rc == 0 and [v[0] for v in prof.values()] == [1], (fn, lib.si_last_error(h).decode(), prof)
        if "cut_clips" not in fn:                                      # C = 0, or a table of no spans: served, whatever the pointers
            empty = dict(table=(), x=False, out=False, out16=False, host=False, dev=False) if "cut_" in fn else dict(spans=[], windows=[], chunks=[], gen=False)
            rc, prof = FC.profiled(ctx, lambda: invoke(fn, {**good, **empty}))
            assert rc == 0 and prof == {}, (fn, lib.si_last_error(h).decode(), prof)
        torch.cuda.synchronize()
        for o in outs:
            o.fill_(7.0)
    assert pairs == {"si_cut_rate": 14, "si_cut_rate_ch": 16, "si_cut_rate_valid": 17, "si_cut_pair": 23, "si_cut_pair_ch": 25, "si_cut_pair_valid": 26,
                     "si_cut_clips": 3, "si_cut_clips_valid": 4, "si_patch_rate": 16 + 12, "si_patch_rate_ch": 18 + 12}, pairs
