"""Experiment: what serving an interleaved file in place costs.  A 10-minute synthetic 48 kHz int16 STEREO recording
with 60 joint gaps of 200 ms (both channels zeroed), HuBERT-base bf16 + HiFi-GAN V1 fp16 stream, in ONE process, one warm-up round, the
variants alternated inside each repeat, device-synchronised wall clock per call:

  (a) engine.conceal_file(x2d, 48000, feed="contexts"): the file stays interleaved; detection per channel (si_quiet_runs_ch), the
      contexts of both channels share the passes, one si_cut_rate_ch and one si_patch_rate_ch launch per channel present in a pass
  (b) the route before it: x2d[:, c].contiguous() per channel, two mono engine.conceal_file(feed="contexts") calls, torch.stack

Prints the first (warm-up) call of each variant on its own line, one line per repeat, the medians, whether the two results are the
same bytes, and -- from separate, untimed runs -- the peak device memory (torch.cuda.max_memory_allocated above what is allocated
before the call) and the profiler's sums of the detection, cut and write-back families per variant.
usage: python tools/exp_channels.py [--repeats 5] [--minutes 10] [--gaps 60] [--sr 48000] [--channels 2]"""
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
ap.add_argument("--channels", type=int, default=2)
ap.add_argument("--batch", type=int, default=32)
a = ap.parse_args()
WARMUP = 1
CLIP, CTX, LM = 200, 50, 10

import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from speech_inpainting_amd.engine import InpaintingEngine

dev = torch.device("cuda:0")
harch, varch = HubertArch.base(), VocoderArch.v1()
eng = InpaintingEngine(harch, varch, 100, dev, "bf16", "fp16").load_state(
    synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100))
sr, ch = a.sr, a.channels
n = int(a.minutes * 60 * sr) + 77
n_rec = n * 50 // sr
cols = []
for c in range(ch):
    tile = synth.synth_wave(1, 30 * sr, synth.DEFAULT_SEED + 6 + c, sr=sr)[0]
    col = (tile.repeat(-(-n // tile.numel()))[:n] * 32767.0).to(torch.int16)
    col[col == 0] = 1                                                 # the only exact zeros are the dropouts
    cols.append(col)
x = torch.stack(cols, dim=1).contiguous()
every = n_rec // a.gaps
gaps = [(k * every + every // 2, LM) for k in range(a.gaps)]
for s, l in G.file_spans(gaps, sr):
    x[s:s + l, :] = 0
x = x.to(dev)
KW = dict(clip_frames=CLIP, min_context=CTX, batch=a.batch, feed="contexts")


def interleaved():
    out = eng.conceal_file(x, sr, **KW)
    if out["gaps"] != [gaps] * ch:
        print("NOTE: the dropouts found are not the planted ones:", [len(g) for g in out["gaps"]], "gaps per channel,", len(gaps), "planted")
    return out["patched"]


def per_channel():
    return torch.stack([eng.conceal_file(x[:, c].contiguous(), sr, **KW)["patched"] for c in range(ch)], dim=1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


VARIANTS = (("interleaved", interleaved), ("per_channel", per_channel))
times = {name: [] for name, _ in VARIANTS}
for r in range(WARMUP + a.repeats):
    order = VARIANTS[r % 2:] + VARIANTS[:r % 2]                        # alternated: each variant takes each place in turn
    row, outs = {}, {}
    for name, fn in order:
        row[name], outs[name] = timed(fn)
    if r == WARMUP:
        same = torch.equal(outs["interleaved"], outs["per_channel"])
        print(f"interleaved | per_channel: {'the same bytes' if same else 'DIFFERENT bytes'}; "
              f"{int((outs['interleaved'] != x).sum())} of {n * ch} samples differ from the file's")
    del outs
    if r >= WARMUP:
        for k, v in row.items():
            times[k].append(v)
        print(f"repeat {r - WARMUP}: " + ", ".join(f"{k} {row[k]:.1f} ms" for k, _ in VARIANTS))
    else:
        print("first call (tables built and uploaded): " + ", ".join(f"{k} {row[k]:.1f} ms" for k, _ in VARIANTS))
for k, v in times.items():
    print(f"median {k}: {statistics.median(v):.1f} ms over {len(v)} repeats (min {min(v):.1f}, max {max(v):.1f})")

for name, fn in VARIANTS:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    print(f"peak device memory {name}: {(torch.cuda.max_memory_allocated() - before) / 2 ** 20:.1f} MiB above the {before / 2 ** 20:.1f} MiB held before the call")
FAMILIES = ("detect_bits_ch", "detect_bits", "detect_carry", "detect_count", "detect_offsets", "detect_emit", "cut_rate_ch", "cut_rate",
            "patch_rate_ch", "patch_rate")
for label, fn in VARIANTS:
    eng.ctx.profile_start(40000)
    fn()
    prof = {e["name"]: e for e in eng.ctx.profile_stop()}
    total = sum(e["ms"] for e in prof.values())
    for name in FAMILIES:
        if name in prof and prof[name]["launches"]:
            print(f"profiled {label}: {name} {prof[name]['launches']} launches, {prof[name]['ms']:.3f} ms")
    print(f"profiled {label}: all families {sum(e['launches'] for e in prof.values())} launches, {total:.1f} ms")
