"""Experiment: what mending the short runs saves.  A 10-minute synthetic recording at 48 kHz, fp32, with 600 NaN runs of
one to eight samples (one every second) and 60 NaN blocks of 200 ms, HuBERT-base bf16 + HiFi-GAN V1 fp16 stream, in ONE process, the
two variants alternated inside each repeat after warm-up, device-synchronised wall clock per call:

  (a) engine.conceal_file(kind="invalid", feed="contexts", min_ms=0, mend_ms=1): the short runs are filled by si_mend_runs, the blocks
      are inpainted
  (b) the same call with mend_ms=0, the parent's: every short run costs a generated 20 ms frame and two cross-fades

Prints, per variant, the median milliseconds per call, the gaps and the generated frames, and the samples of `patched` whose bits
differ from the file's; for (a) also the mended rows by status and -- from a separate, untimed run under the library's profiler --
the time of the patch_rate family's launches (si_mend_runs is profiled there).  Times are reported, not asserted.

--leg impulse: the same recording with no NaN in it and 600 planted IN-RANGE clicks of one to three samples (+-0.5 of
full scale added, clipped to [-1, 1]) instead:
  (c) engine.conceal_file(kind="impulse", min_ms=0, mend_ms=1, feed="contexts"): detected by si_impulse_runs, mended by si_mend_runs
  (d) engine.find_impulse_runs alone at the same settings, and (e) engine.find_burst_runs(half=44) on the same file in the same process
Prints the median milliseconds per call of each, the runs found and how many planted clicks lie in one, the mended rows by status, the
gaps, and the samples of `patched` that differ from the file's.
usage: python tools/exp_mend.py [--repeats 5] [--minutes 10] [--blocks 60] [--runs 600] [--leg mend|impulse]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--blocks", type=int, default=60)
ap.add_argument("--runs", type=int, default=600)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--leg", choices=("mend", "impulse"), default="mend")
a = ap.parse_args()
WARMUP = 1
SR, PER, CLIP, CTX, LM = 48000, 960, 200, 50, 10

import torch

from speech_inpainting_amd import native, synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from speech_inpainting_amd.engine import InpaintingEngine

dev = torch.device("cuda:0")
harch, varch = HubertArch.base(), VocoderArch.v1()
eng = InpaintingEngine(harch, varch, 100, dev, "bf16", "fp16").load_state(
    synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100))
n = int(a.minutes * 60 * SR) + 123
n_rec = n // PER
tile = synth.synth_wave(1, 30 * SR, synth.DEFAULT_SEED + 6, sr=SR)[0]
x = tile.repeat(-(-n // tile.numel()))[:n].contiguous()
every_b, every_r = n_rec // a.blocks, n_rec // a.runs


def impulse_leg():
    from speech_inpainting_amd import gaps as G
    y = x.clone()
    g = torch.Generator().manual_seed(1)
    clicks = []
    for k in range(a.runs):
        s, m = PER * (k * every_r + every_r // 4) + 17 + (131 * k) % 800, 1 + k % 3
        y[s:s + m] = (y[s:s + m] + 0.5 * (2.0 * torch.randint(0, 2, (m,), generator=g) - 1.0)).clamp(-1.0, 1.0)
        clicks.append((s, m))
    y = y.to(dev)
    d = G.IMPULSE_DEFAULTS
    half = G.level_half(d["win_ms"], SR)
    legs = {"c": lambda: eng.conceal_file(y, SR, kind="impulse", min_ms=0, mend_ms=1.0, feed="contexts", clip_frames=CLIP, min_context=CTX, batch=a.batch),
            "d": lambda: eng.find_impulse_runs(y, half=half, order=d["order"], guard=d["guard"], pad=d["pad"], ratio=d["ratio"]),
            "e": lambda: eng.find_burst_runs(y, half=44, threshold=1.15)}
    took, out = {k: [] for k in legs}, {}
    for r in range(WARMUP + a.repeats):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[k] = fn()
            torch.cuda.synchronize()
            if r >= WARMUP:
                took[k].append((time.perf_counter() - t0) * 1e3)
    rows = out["d"].tolist()
    starts = sorted(rows)
    import bisect
    inside = 0
    for s, m in clicks:
        i = bisect.bisect_right(starts, [s, 1 << 30]) - 1
        inside += i >= 0 and starts[i][0] <= s and s + m <= starts[i][0] + starts[i][1]
    count = {}
    for _, _, st in out["c"]["mended"]:
        count[native.MEND_STATUS[st]] = count.get(native.MEND_STATUS[st], 0) + 1
    changed = int((out["c"]["patched"].contiguous().view(torch.int32) != y.view(torch.int32)).sum())
    med = {k: statistics.median(v) for k, v in took.items()}
    print(f"(c) conceal_file(kind='impulse', min_ms=0, mend_ms=1): median {med['c']:.3f} ms per call;  {len(out['c']['gaps'])} gaps, "
          f"{len(out['c']['skipped'])} skipped;  mended rows by status: {count};  {changed} samples of patched differ from the file's")
    print(f"(d) find_impulse_runs(half={half}) alone: median {med['d']:.3f} ms per call;  {len(rows)} runs, the longest {max((l for _, l in rows), default=0)} samples;  "
          f"{inside} of {len(clicks)} planted clicks lie inside one run")
    print(f"(e) find_burst_runs(half=44) on the same file: median {med['e']:.3f} ms per call;  {out['e'].shape[0]} runs")


if a.leg == "impulse":
    impulse_leg()
    sys.exit(0)
blocks = [(k * every_b + every_b // 2, LM) for k in range(a.blocks)]
for p, l in blocks:
    x[PER * p:PER * (p + l)] = float("nan")
short = []
for k in range(a.runs):
    f = k * every_r + every_r // 4
    if any(p - 3 <= f < p + l + 3 for p, l in blocks):                  # keep a short run's frame clear of a block's cross-fade
        f += 5
    s, m = PER * f + 17 + (131 * k) % 800, 1 + k % 8
    x[s:s + m] = float("nan")
    short.append((s, m))
x = x.to(dev)
KW = dict(min_ms=0, kind="invalid", feed="contexts", clip_frames=CLIP, min_context=CTX, batch=a.batch)


def call(mend_ms):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.conceal_file(x, SR, mend_ms=mend_ms, **KW)
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


times = {"a": [], "b": []}
for r in range(WARMUP + a.repeats):
    (oa, ta), (ob, tb) = call(1.0), call(0.0)
    if r >= WARMUP:
        times["a"].append(ta)
        times["b"].append(tb)
        print(f"repeat {r - WARMUP}: (a) {ta:.3f} ms, (b) {tb:.3f} ms")
bits = lambda t: t.contiguous().view(torch.int32)
for key, out in (("a", oa), ("b", ob)):
    changed = int((bits(out["patched"]) != bits(x)).sum())
    print(f"({key}) median {statistics.median(times[key]):.3f} ms per call;  {len(out['gaps'])} gaps, {sum(l for _, l in out['gaps'])} generated frames, "
          f"{len(out['skipped'])} skipped;  {changed} samples of patched differ from the file's;  finite: {bool(torch.isfinite(out['patched']).all())}")
count = {}
for _, _, st in oa["mended"]:
    count[native.MEND_STATUS[st]] = count.get(native.MEND_STATUS[st], 0) + 1
print(f"(a) mended rows by status: {count} of {len(short)} short runs planted")
eng.ctx.profile_start(20000)
eng.conceal_file(x, SR, mend_ms=1.0, **KW)
prof = {e["name"]: e for e in eng.ctx.profile_stop()}
torch.cuda.synchronize()
e = prof.get("patch_rate")
if e:
    print(f"(a) under the profiler: patch_rate family {e['launches']} launches, {e['ms']:.3f} ms (si_mend_runs is one of them)")
print(f"(a) / (b) {statistics.median(times['a']) / statistics.median(times['b']):.3f}")
