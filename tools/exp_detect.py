"""Experiment: what finding the dropouts costs.  The 10-minute synthetic recording of tools/exp_long.py with its 60
gaps of 200 ms zeroed, HuBERT-base bf16 + HiFi-GAN V1 fp16 stream, in ONE process, the variants alternated inside each repeat after
warm-up, device-synchronised wall clock per call:

  (a) si_quiet_runs (five launches) + the one D2H copy of the count: engine.find_quiet_runs
  (b) the torch formulation on the same device: q = x.abs() <= thr, diff of the zero-padded mask, nonzero of the rises and of the
      falls, the length filter, stack -- the baseline a caller would write
  (c) engine.conceal_recording(pcm=True): find the gaps, then patch_recording
  (d) engine.patch_recording(pcm=True) with the known gaps
  (e) engine.find_dead_runs(kind="held") on the same recording with its gaps filled by the HELD last sample instead of zeros
      (si_dead_runs: pass 1 with the links, the four scan passes), and (f) its torch formulation: the links
      |x[i] - x[i-1]| <= 0, held = link(i) | link(i+1), then (b)'s run extraction
  (g) engine.find_dead_runs(kind="any", rel_threshold=1e-3) on that file (pass 0 reads the samples once more for the peak), and (h)
      its torch formulation: the peak over the finite samples, T = fp32(1e-3) * peak, (abs() <= T) | held
  (i) engine.find_level_runs(half=22, threshold=16 int16 steps) on the same recording with its gaps filled by seeded NOISE of sigma =
      12 int16 steps (si_level_runs: pass 1 with the windowed energy, the four scan passes), and (j) its torch
      formulation: avg_pool1d of the float64 squares (count_include_pad=False: the truncated count) against T^2, max_pool1d of the
      mask, then (b)'s run extraction
  (k) engine.find_burst_runs(half=44, threshold=1.15 of full scale) on the same recording with its gaps filled by seeded full-scale
      GARBAGE, uniformly random int16 (si_burst_runs: pass 1 with the windowed energy of the second difference, the four
      scan passes), and (l) its torch formulation: the float64 squares of x[k-1] - 2 x[k] + x[k+1] for 1 <= k <= n - 2, avg_pool1d of
      them and of the centres' indicator (times the window: the sum and the truncated count) against T^2, max_pool1d of the mask, then
      (b)'s run extraction
  (m) engine.find_invalid_runs(ceiling=4.0) on the same recording with its gaps filled by seeded NaN, +-inf and 3e38 (DESIGN.md 4.30;
      si_invalid_runs: pass 1 with the value predicate, the four scan passes), and (n) its torch formulation: ~(x.abs() <= c), then
      (b)'s run extraction; (o) engine.conceal_file(kind="invalid", threshold=4.0, feed="contexts", min_ms=0) on the 48 kHz copy of
      the recording with the same damage in its gaps' file samples, beside (p) engine.patch_file(feed="contexts") with the known gaps
      on the zero-filled 48 kHz copy.  fp32 only: skipped with --pcm16.  A timed block of its own behind the others.

Prints whether (a) equals (b), (e) equals (f), (g) equals (h), (i) equals (j), (k) equals (l) and (c) equals (d) bit for bit, one line per repeat, the medians, and -- from a separate, untimed run
under the library's profiler -- the per-kernel times of the detect_* family and the effective bytes per second of the whole call
(the recording's bytes / the family's summed time).
usage: python tools/exp_detect.py [--repeats 7] [--minutes 10] [--gaps 60] [--pcm16]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--gaps", type=int, default=60)
ap.add_argument("--fade", type=int, default=110)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--pcm16", action="store_true", help="time (a) and (b) on the int16 PCM of the recording instead of its fp32 samples")
a = ap.parse_args()
WARMUP = 2
CLIP, CTX, LM, MIN_LEN = 200, 50, 10, 110

import torch

from speech_inpainting_amd import synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from speech_inpainting_amd.engine import InpaintingEngine

dev = torch.device("cuda:0")
harch, varch = HubertArch.base(), VocoderArch.v1()
eng = InpaintingEngine(harch, varch, 100, dev, "bf16", "fp16").load_state(
    synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100))
N22 = int(a.minutes * 60 * 22050) + 123
n_rec = N22 // 441
tile = synth.synth_wave(1, 30 * 22050, synth.DEFAULT_SEED + 6, sr=22050)[0]
wave22 = tile.repeat(-(-N22 // tile.numel()))[:N22].contiguous().to(dev)
every = n_rec // a.gaps
gaps = [(k * every + every // 2, LM) for k in range(a.gaps)]
for p, l in gaps:
    wave22[441 * p:441 * (p + l)] = 0
x = eng.to_int16(wave22) if a.pcm16 else wave22
KW = dict(fade=a.fade, clip_frames=CLIP, min_context=CTX, batch=a.batch, pcm=True)


def torch_runs():
    q = (x.abs() <= 0).to(torch.int8) if not a.pcm16 else (x.to(torch.int32).abs() <= 0).to(torch.int8)
    d = torch.diff(q, prepend=q.new_zeros(1), append=q.new_zeros(1))
    start, end = torch.nonzero(d == 1).flatten(), torch.nonzero(d == -1).flatten()
    keep = end - start >= MIN_LEN
    return torch.stack([start[keep], (end - start)[keep]], dim=1).to(torch.int32)


# the same recording with every gap filled by the last sample before it (x[s - 1] is a sample of the tile, not a zero)
held22 = wave22.clone()
for p, l in gaps:
    held22[441 * p:441 * (p + l)] = held22[441 * p - 1]
xh = eng.to_int16(held22) if a.pcm16 else held22


def torch_dead(rel):
    v = xh.to(torch.int32) if a.pcm16 else xh
    link = (v[1:] - v[:-1]).abs() <= 0
    no = link.new_zeros(1)
    dead = torch.cat([no, link]) | torch.cat([link, no])
    if rel > 0:
        mag = v.abs().to(torch.float32)
        peak = mag[torch.isfinite(mag)].max()
        dead = dead | (mag <= torch.tensor(rel, dtype=torch.float32, device=dev) * peak)
    q = dead.to(torch.int8)
    d = torch.diff(q, prepend=q.new_zeros(1), append=q.new_zeros(1))
    start, end = torch.nonzero(d == 1).flatten(), torch.nonzero(d == -1).flatten()
    keep = end - start >= MIN_LEN
    return torch.stack([start[keep], (end - start)[keep]], dim=1).to(torch.int32)


# the same recording with every gap filled by a noise floor: rint(N(0, 12)) int16 steps, seeded (values on the 2^-15 grid in fp32)
LEVEL_HALF, LEVEL_T = 22, 16.0
noise22 = wave22.clone()
gen = torch.Generator(device="cpu").manual_seed(7)
for p, l in gaps:
    noise22[441 * p:441 * (p + l)] = (torch.randn(441 * l, generator=gen) * 12.0).round().to(dev) / 32768.0
xn = eng.to_int16(noise22) if a.pcm16 else noise22
level_thr = LEVEL_T if a.pcm16 else LEVEL_T / 32768.0


def torch_level():
    sq = xn.to(torch.float64).square()[None, None]
    mean = torch.nn.functional.avg_pool1d(sq, 2 * LEVEL_HALF + 1, 1, LEVEL_HALF, count_include_pad=False)
    low = (mean <= level_thr * level_thr).to(torch.float32)
    q = (torch.nn.functional.max_pool1d(low, 2 * LEVEL_HALF + 1, 1, LEVEL_HALF)[0, 0] > 0).to(torch.int8)
    d = torch.diff(q, prepend=q.new_zeros(1), append=q.new_zeros(1))
    start, end = torch.nonzero(d == 1).flatten(), torch.nonzero(d == -1).flatten()
    keep = end - start >= MIN_LEN
    return torch.stack([start[keep], (end - start)[keep]], dim=1).to(torch.int32)


# the same recording with every gap filled by full-scale garbage: uniformly random int16, seeded (values on the 2^-15 grid in fp32)
BURST_HALF, BURST_T = 44, 1.15
garb22 = wave22.clone()
for p, l in gaps:
    garb22[441 * p:441 * (p + l)] = torch.randint(-32768, 32768, (441 * l,), generator=gen).to(dev) / 32768.0
xb = eng.to_int16(garb22) if a.pcm16 else garb22
burst_thr = BURST_T * 32768.0 if a.pcm16 else BURST_T


def torch_burst():
    v = xb.to(torch.float64)
    n, L = v.numel(), 2 * BURST_HALF + 1
    sq, centre = v.new_zeros(n), v.new_zeros(n)
    sq[1:n - 1] = (v[:-2] - 2 * v[1:-1] + v[2:]).square()
    centre[1:n - 1] = 1
    pool = lambda t: torch.nn.functional.avg_pool1d(t[None, None], L, 1, BURST_HALF, count_include_pad=True) * L
    T = float(torch.tensor(burst_thr, dtype=torch.float32))
    E, cnt = pool(sq), pool(centre).round()
    hot = ((cnt >= 1) & (E >= T * T * cnt)).to(torch.float32)
    q = (torch.nn.functional.max_pool1d(hot, L, 1, BURST_HALF)[0, 0] > 0).to(torch.int8)
    d = torch.diff(q, prepend=q.new_zeros(1), append=q.new_zeros(1))
    start, end = torch.nonzero(d == 1).flatten(), torch.nonzero(d == -1).flatten()
    keep = end - start >= MIN_LEN
    return torch.stack([start[keep], (end - start)[keep]], dim=1).to(torch.int32)


variants = {"a": lambda: eng.find_quiet_runs(x, 0.0, MIN_LEN), "b": torch_runs,
            "c": lambda: eng.conceal_recording(wave22, **KW), "d": lambda: eng.patch_recording(wave22, gaps, **KW),
            "e": lambda: eng.find_dead_runs(xh, "held", min_len=MIN_LEN), "f": lambda: torch_dead(0.0),
            "g": lambda: eng.find_dead_runs(xh, "any", rel_threshold=1e-3, min_len=MIN_LEN), "h": lambda: torch_dead(1e-3),
            "i": lambda: eng.find_level_runs(xn, half=LEVEL_HALF, threshold=level_thr, min_len=MIN_LEN), "j": torch_level,
            "k": lambda: eng.find_burst_runs(xb, half=BURST_HALF, threshold=burst_thr, min_len=MIN_LEN), "l": torch_burst}
oa, ob, oc, od, oe, of, og, oh, oi, oj, ok, ol = (fn() for fn in variants.values())
torch.cuda.synchronize()
print(f"recording of {N22} samples ({N22 / 22050 / 60:.2f} min, {x.element_size()} bytes per sample), {len(gaps)} gaps of {LM} frames zeroed")
print(f"(a) equals (b): {torch.equal(oa, ob)} ({oa.shape[0]} runs);  (c) found the gaps: {oc['gaps'] == gaps};  (c) equals (d) bit for bit: fp32",
      torch.equal(oc["patched"].view(torch.int32), od["patched"].view(torch.int32)), " int16", torch.equal(oc["patched_pcm"], od["patched_pcm"]))
print(f"(e) equals (f): {torch.equal(oe, of)} ({oe.shape[0]} runs, {int((oe[:, 1] == 441 * LM + 1).sum())} of them a gap and the sample it holds);  "
      f"(g) equals (h): {torch.equal(og, oh)} ({og.shape[0]} runs)")
print(f"(i) equals (j): {torch.equal(oi, oj)} ({oi.shape[0]} runs, {sum(1 for r in oi.tolist() if r in [[441 * p, 441 * l] for p, l in gaps])} of them exactly a gap;  "
      f"the sample-wise detector at the same threshold finds {eng.find_quiet_runs(xn, level_thr, MIN_LEN).shape[0]} runs)")
covered = sum(1 for p, l in gaps if any(r[0] <= 441 * p and r[0] + r[1] >= 441 * (p + l) for r in ok.tolist()))
print(f"(k) equals (l): {torch.equal(ok, ol)} ({ok.shape[0]} runs, {covered} of {len(gaps)} gaps inside one of them;  quiet, held and level detection on that "
      f"file find {eng.find_quiet_runs(xb, 0.0, MIN_LEN).shape[0]}, {eng.find_dead_runs(xb, 'held', min_len=MIN_LEN).shape[0]} and "
      f"{eng.find_level_runs(xb, half=LEVEL_HALF, threshold=level_thr, min_len=MIN_LEN).shape[0]} runs)")
del oa, ob, oc, od, oe, of, og, oh, oi, oj, ok, ol
for fn in variants.values():
    for _ in range(WARMUP):
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in variants}
for r in range(a.repeats):
    for k, fn in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) * 1e3)
    print(f"repeat {r}: " + "  ".join(f"({k}) {ms[k][-1]:.3f} ms" for k in variants), flush=True)
med = {k: statistics.median(v) for k, v in ms.items()}
print("median ms/recording: " + "  ".join(f"({k}) {med[k]:.3f}" for k in variants))
print(f"spread of (d) over {a.repeats} repeats: {max(ms['d']) - min(ms['d']):.3f} ms;  (c) - (d) {med['c'] - med['d']:+.3f} ms;  (a) / (b) {med['a'] / med['b']:.3f};  "
      f"(e) / (f) {med['e'] / med['f']:.3f};  (g) / (h) {med['g'] / med['h']:.3f};  (e) / (a) {med['e'] / med['a']:.3f};  (g) / (a) {med['g'] / med['a']:.3f};  (i) / (j) {med['i'] / med['j']:.3f};  (i) / (a) {med['i'] / med['a']:.3f};  (k) / (l) {med['k'] / med['l']:.3f};  (k) / (i) {med['k'] / med['i']:.3f}")
# per-kernel device times, from a run of their own under the library's event profiler (every launch bracketed: not a step time)
eng.ctx.profile_start(1000)
for _ in range(10):
    eng.find_quiet_runs(x, 0.0, MIN_LEN)
rows = {e["name"]: e for e in eng.ctx.profile_stop() if e["name"].startswith("detect_")}
total = sum(e["ms"] for e in rows.values()) / 10
print(f"si_quiet_runs under the profiler: {total * 1e3:.1f} us per call = {x.numel() * x.element_size() / (total * 1e-3) / 1e9:.1f} GB/s of the recording;  "
      + "  ".join(f"{n} {e['ms'] / e['launches'] * 1e3:.1f} us" for n, e in rows.items()))
for what, call in (("kind=held", lambda: eng.find_dead_runs(xh, "held", min_len=MIN_LEN)),
                   ("kind=any, rel_threshold=1e-3", lambda: eng.find_dead_runs(xh, "any", rel_threshold=1e-3, min_len=MIN_LEN))):
    eng.ctx.profile_start(1000)
    for _ in range(10):
        call()
    rows = {e["name"]: e for e in eng.ctx.profile_stop() if e["name"].startswith("detect_")}
    total = sum(e["ms"] for e in rows.values()) / 10
    print(f"si_dead_runs ({what}) under the profiler: {total * 1e3:.1f} us per call = {xh.numel() * xh.element_size() / (total * 1e-3) / 1e9:.1f} GB/s of the "
          f"recording;  " + "  ".join(f"{n} {e['ms'] / e['launches'] * 1e3:.1f} us" for n, e in rows.items()))
eng.ctx.profile_start(1000)
for _ in range(10):
    eng.find_level_runs(xn, half=LEVEL_HALF, threshold=level_thr, min_len=MIN_LEN)
rows = {e["name"]: e for e in eng.ctx.profile_stop() if e["name"].startswith("detect_")}
total = sum(e["ms"] for e in rows.values()) / 10
print(f"si_level_runs (half={LEVEL_HALF}) under the profiler: {total * 1e3:.1f} us per call = {xn.numel() * xn.element_size() / (total * 1e-3) / 1e9:.1f} GB/s of the "
      f"recording;  " + "  ".join(f"{n} {e['ms'] / e['launches'] * 1e3:.1f} us" for n, e in rows.items()))
for half in (0, 110, 1024):
    eng.ctx.profile_start(1000)
    for _ in range(10):
        eng.find_level_runs(xn, half=half, threshold=level_thr, min_len=MIN_LEN)
    e = {e["name"]: e for e in eng.ctx.profile_stop()}["detect_dead"]             # the level kernel is profiled in pass 1's family
    print(f"detect_level_kernel at half={half}: {e['ms'] / e['launches'] * 1e3:.1f} us")
for half in (0, 44, 1024):
    eng.ctx.profile_start(1000)
    for _ in range(10):
        eng.find_burst_runs(xb, half=half, threshold=burst_thr, min_len=MIN_LEN)
    e = {e["name"]: e for e in eng.ctx.profile_stop()}["detect_dead"]             # the burst kernel is profiled in pass 1's family too
    print(f"detect_burst_kernel at half={half}: {e['ms'] / e['launches'] * 1e3:.1f} us")

# ---- (m) .. (p): the sample values themselves are the damage.  fp32 only
if not a.pcm16:
    from speech_inpainting_amd import gaps as G
    CEIL = 4.0
    bad = torch.tensor([float("nan"), float("inf"), float("-inf"), 3e38, -3e38], dtype=torch.float32)
    pick = lambda n: bad[torch.randint(0, bad.numel(), (n,), generator=gen)].to(dev)
    inv22 = wave22.clone()
    for p, l in gaps:
        inv22[441 * p:441 * (p + l)] = pick(441 * l)
    SR = 48000
    wave48 = eng.resample(wave22[None], 22050, SR)[0].contiguous()              # the zero-filled copy at 48 kHz
    zero48, inv48 = wave48.clone(), wave48.clone()
    for s, l in G.file_spans(gaps, SR):
        zero48[s:s + l] = 0
        inv48[s:s + l] = pick(l)
    FKW = dict(clip_frames=CLIP, min_context=CTX, batch=a.batch, feed="contexts")

    def torch_invalid():
        q = (~(inv22.abs() <= CEIL)).to(torch.int8)
        d = torch.diff(q, prepend=q.new_zeros(1), append=q.new_zeros(1))
        start, end = torch.nonzero(d == 1).flatten(), torch.nonzero(d == -1).flatten()
        keep = end - start >= MIN_LEN
        return torch.stack([start[keep], (end - start)[keep]], dim=1).to(torch.int32)

    legs = {"m": lambda: eng.find_invalid_runs(inv22, CEIL, MIN_LEN), "n": torch_invalid,
            "o": lambda: eng.conceal_file(inv48, SR, CEIL, min_ms=0, kind="invalid", **FKW), "p": lambda: eng.patch_file(zero48, SR, gaps, **FKW)}
    om, on, oo, op = (fn() for fn in legs.values())
    torch.cuda.synchronize()
    inside = torch.zeros(zero48.numel(), dtype=torch.bool, device=dev)
    for s, l in G.file_spans(oo["gaps"], SR):
        inside[s:s + l] = True
    print(f"(m) equals (n): {torch.equal(om, on)} ({om.shape[0]} runs, {sum(1 for r in om.tolist() if r in [[441 * p, 441 * l] for p, l in gaps])} of them exactly "
          f"a gap);  (o) found the gaps: {oo['gaps'] == gaps}, skipped {len(oo['skipped'])};  (o) is finite: {bool(torch.isfinite(oo['patched']).all())};  "
          f"(o) equals (p) inside the gaps bit for bit: {torch.equal(oo['patched'][inside].view(torch.int32), op['patched'][inside].view(torch.int32))}, labels "
          f"{torch.equal(oo['labels'], op['labels'])};  quiet, held, level and burst detection on that file find "
          f"{eng.find_quiet_runs(inv22, 0.0, MIN_LEN).shape[0]}, {eng.find_dead_runs(inv22, 'held', min_len=MIN_LEN).shape[0]}, "
          f"{eng.find_level_runs(inv22, half=LEVEL_HALF, threshold=level_thr, min_len=MIN_LEN).shape[0]} and "
          f"{eng.find_burst_runs(inv22, half=BURST_HALF, threshold=burst_thr, min_len=MIN_LEN).shape[0]} runs")
    del om, on, oo, op
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms2 = {k: [] for k in legs}
    for r in range(a.repeats):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms2[k].append((time.perf_counter() - t0) * 1e3)
        print(f"repeat {r}: " + "  ".join(f"({k}) {ms2[k][-1]:.3f} ms" for k in legs), flush=True)
    med2 = {k: statistics.median(v) for k, v in ms2.items()}
    print("median ms/recording: " + "  ".join(f"({k}) {med2[k]:.3f}" for k in legs)
          + f";  (m) / (n) {med2['m'] / med2['n']:.3f};  (m) / (a) {med2['m'] / med['a']:.3f};  (o) - (p) {med2['o'] - med2['p']:+.3f} ms, spread of (p) "
          f"{max(ms2['p']) - min(ms2['p']):.3f} ms")
    eng.ctx.profile_start(1000)
    for _ in range(10):
        eng.find_invalid_runs(inv22, CEIL, MIN_LEN)
    e = {e["name"]: e for e in eng.ctx.profile_stop()}["detect_bits"]            # the invalid kernel is profiled in the quiet pass 1's family
    print(f"detect_invalid_kernel: {e['ms'] / e['launches'] * 1e3:.1f} us")
