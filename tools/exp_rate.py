"""Experiment: what keeping the file's own rate costs.  A 10-minute synthetic 48 kHz int16 recording with 60 gaps of
200 ms, HuBERT-base bf16 + HiFi-GAN V1 fp16 stream, in ONE process, the variants alternated inside each repeat after warm-up,
device-synchronised wall clock per call:

  (a) engine.patch_file(x, 48000, gaps): the recording stays 48 kHz int16, one si_patch_rate per pass
  (b) the only way back there was: resample to 22.05 kHz, engine.patch_recording, engine.resample of the WHOLE result to 48 kHz,
      to_int16 -- which returns none of the file's own samples

  (c) engine.patch_file(x, 48000, gaps, feed="contexts"): as (a), but the model is fed by context clips cut straight
      from the int16 file (one si_cut_rate per pass)

(a) and (b) resample the whole recording to 22.05 kHz on the way in; (c) does not.  Prints the first (warm-up) call of each variant
on its own line -- it includes building and uploading the filter tables, for (a) and (b) a float64 time table of the recording's
length --, one line per repeat, the medians, how many samples of the file each variant changed, how many predicted labels differ between
(a) and (c), and -- from separate, untimed runs -- the profiler's time of the cut_rate, patch_rate and resample_sinc families and the
peak device memory (torch.cuda.max_memory_allocated above what is allocated before the call) per variant.
usage: python tools/exp_rate.py [--repeats 5] [--minutes 10] [--gaps 60] [--sr 48000]      (sparse case: --minutes 60 --gaps 6)

--clips16 runs another pair instead, by the same protocol: feed="contexts" with clips16="file" (one si_cut_pair per pass
yields both clip sets) against clips16="resampled" (si_cut_rate, then the clips resampled to 16 kHz), on the recording and on a 16 kHz
int16 copy of it; wall clock, the profiler's rows of the way in, and the labels and samples that differ between the two."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--gaps", type=int, default=60)
ap.add_argument("--sr", type=int, default=48000)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--clips16", action="store_true")
a = ap.parse_args()
WARMUP = 1
CLIP, CTX, LM = 200, 50, 10

import torch

from speech_inpainting_amd import synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from speech_inpainting_amd.engine import InpaintingEngine

dev = torch.device("cuda:0")
harch, varch = HubertArch.base(), VocoderArch.v1()
eng = InpaintingEngine(harch, varch, 100, dev, "bf16", "fp16").load_state(
    synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100))
sr = a.sr
n = int(a.minutes * 60 * sr) + 77
n_rec = n * 50 // sr
tile = synth.synth_wave(1, 30 * sr, synth.DEFAULT_SEED + 6, sr=sr)[0]
x = (tile.repeat(-(-n // tile.numel()))[:n] * 32767.0).to(torch.int16).contiguous().to(dev)
every = n_rec // a.gaps
gaps = [(k * every + every // 2, LM) for k in range(a.gaps)]
KW = dict(clip_frames=CLIP, min_context=CTX, batch=a.batch)


def keep_rate():
    return eng.patch_file(x, sr, gaps, **KW)["patched"]


def feed_contexts():
    return eng.patch_file(x, sr, gaps, feed="contexts", **KW)["patched"]


def round_trip():
    wave22 = eng.resample((x.to(torch.float32) / 32768.0)[None], sr, 22050)[0].contiguous()
    patched = eng.patch_recording(wave22, gaps, fade=110, **KW)["patched"]
    return eng.to_int16(eng.resample(patched[None], 22050, sr)[0][:n].contiguous())


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def clips16_pair(xf, srf, label):
    """clips16="file" against "resampled" on the file xf at srf Hz: alternated wall clock, profiled rows, what differs."""
    run = {m: (lambda m=m: eng.patch_file(xf, srf, gaps, feed="contexts", clips16=m, **KW)) for m in ("resampled", "file")}
    t = {m: [] for m in run}
    for r in range(WARMUP + a.repeats):
        for m in (("resampled", "file") if r % 2 == 0 else ("file", "resampled")):
            ms, out = timed(run[m])
            del out
            if r >= WARMUP:
                t[m].append(ms)
    for m in run:
        print(f"{label}: median clips16={m}: {statistics.median(t[m]):.1f} ms over {len(t[m])} repeats (min {min(t[m]):.1f}, max {max(t[m]):.1f})")
    res = {}
    for m in run:
        eng.ctx.profile_start(20000)
        res[m] = run[m]()
        prof = {e["name"]: e for e in eng.ctx.profile_stop()}
        for name in ("cut_rate", "resample_sinc", "patch_rate"):
            if name in prof and prof[name]["launches"]:
                print(f"{label}: profiled clips16={m}: {name} {prof[name]['launches']} launches, {prof[name]['ms']:.3f} ms")
    print(f"{label}: clips16 file | resampled: {int((res['file']['labels'] != res['resampled']['labels']).sum())} of {res['file']['labels'].numel()} "
          f"predicted labels differ, {int((res['file']['patched'] != res['resampled']['patched']).sum())} of {xf.numel()} samples of patched differ")


if a.clips16:
    clips16_pair(x, sr, f"{sr} Hz int16")
    x16k = eng.to_int16(eng.resample((x.to(torch.float32) / 32768.0)[None], sr, 16000)[0].contiguous())
    clips16_pair(x16k, 16000, "16000 Hz int16 copy")
    sys.exit(0)


VARIANTS = (("patch_file", keep_rate), ("feed_contexts", feed_contexts), ("round_trip", round_trip))
times = {name: [] for name, _ in VARIANTS}
for r in range(WARMUP + a.repeats):
    order = VARIANTS[r % 3:] + VARIANTS[:r % 3]                        # alternated: each variant takes each place in turn
    row = {}
    for name, fn in order:
        row[name], out = timed(fn)
        if r == WARMUP:
            print(f"{name}: {int((out != x[:out.numel()]).sum())} of {n} samples differ from the file's")
        del out
    if r >= WARMUP:
        for k, v in row.items():
            times[k].append(v)
        print(f"repeat {r - WARMUP}: " + ", ".join(f"{k} {row[k]:.1f} ms" for k, _ in VARIANTS))
    else:
        print("first call (tables built and uploaded): " + ", ".join(f"{k} {row[k]:.1f} ms" for k, _ in VARIANTS))
for k, v in times.items():
    print(f"median {k}: {statistics.median(v):.1f} ms over {len(v)} repeats")

ra = eng.patch_file(x, sr, gaps, **KW)
rc = eng.patch_file(x, sr, gaps, feed="contexts", **KW)
print(f"feed=recording | feed=contexts: {int((ra['labels'] != rc['labels']).sum())} of {ra['labels'].numel()} predicted labels differ, "
      f"{int((ra['patched'] != rc['patched']).sum())} of {n} samples of patched differ")
del ra, rc
for name, fn in VARIANTS:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    print(f"peak device memory {name}: {(torch.cuda.max_memory_allocated() - before) / 2 ** 20:.1f} MiB above the {before / 2 ** 20:.1f} MiB held before the call")
for label, fn in (("patch_file", keep_rate), ("feed_contexts", feed_contexts)):
    eng.ctx.profile_start(20000)
    fn()
    prof = {e["name"]: e for e in eng.ctx.profile_stop()}
    for name in ("cut_rate", "cut_clips", "patch_rate", "resample_sinc"):
        if name in prof and prof[name]["launches"]:
            print(f"profiled {label}: {name} {prof[name]['launches']} launches, {prof[name]['ms']:.3f} ms")
eng.ctx.profile_start(20000)
round_trip()
prof = {e["name"]: e for e in eng.ctx.profile_stop()}
for name in ("patch_regions", "resample_sinc"):
    if name in prof:
        print(f"profiled round trip: {name} {prof[name]['launches']} launches, {prof[name]['ms']:.3f} ms")
