"""Experiment: what keeping a 24-bit file packed costs.  tools/exp_rate.py's 10-minute synthetic 48 kHz recording as a
packed 24-bit file with 60 dropouts of 200 ms (exact zeros), HuBERT-base bf16 + HiFi-GAN V1 fp16 stream, in ONE process, the two
variants alternated inside each repeat after warm-up, device-synchronised wall clock per call:

  (a) engine.conceal_file(s24, 48000, feed="contexts"): detection, both cutters and the patch read and write the packed bytes
  (b) what such a file cost before: a torch unpack on the device (bytes -> int32 by shifts -> fp32), conceal_file on the fp32, and a
      repack of the result (fp32 -> int32 -> bytes)

Prints one line per repeat, the medians, whether (a) is the store rule of (b)'s fp32 result, and -- from separate, untimed runs -- the
profiler's time of the detection and cut / patch families and the peak device memory per variant.  Nothing is asserted.
usage: python tools/exp_s24.py [--repeats 6] [--minutes 10] [--gaps 60] [--sr 48000]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=6)
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--gaps", type=int, default=60)
ap.add_argument("--sr", type=int, default=48000)
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
sr = a.sr
n = int(a.minutes * 60 * sr) + 77
n_rec = n * 50 // sr
tile = synth.synth_wave(1, 30 * sr, synth.DEFAULT_SEED + 6, sr=sr)[0]
v = (tile.repeat(-(-n // tile.numel()))[:n].double() * 8388607.0).trunc().to(torch.int32)
v[v == 0] = 1
every = n_rec // a.gaps
gaps = [(k * every + every // 2, LM) for k in range(a.gaps)]
for s, l in G.file_spans(gaps, sr):
    v[s:s + l] = 0
v = v.to(dev)


def pack(v32):
    return torch.stack([v32 & 0xFF, (v32 >> 8) & 0xFF, (v32 >> 16) & 0xFF], dim=-1).to(torch.uint8)


def unpack(b):
    w = b.to(torch.int32)
    return ((w[..., 0] << 8 | w[..., 1] << 16 | w[..., 2] << 24) >> 8)


x24 = pack(v).contiguous()
KW = dict(clip_frames=CLIP, min_context=CTX, batch=a.batch, feed="contexts", merge_frames=1)


def packed():
    return eng.conceal_file(x24, sr, **KW)


def through_fp32():
    f = unpack(x24).to(torch.float32) * (1.0 / 8388608.0)
    out = eng.conceal_file(f, sr, **KW)
    p = out["patched"] * 8388608.0
    out["repacked"] = pack(torch.nan_to_num(p, nan=0.0).trunc().clamp(-8388608.0, 8388607.0).to(torch.int32))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


VARIANTS = (("s24", packed), ("fp32 round trip", through_fp32))
times = {name: [] for name, _ in VARIANTS}
for r in range(WARMUP + a.repeats):
    row = {}
    for name, fn in (VARIANTS if r % 2 == 0 else VARIANTS[::-1]):
        row[name], out = timed(fn)
        del out
    if r >= WARMUP:
        for k, ms in row.items():
            times[k].append(ms)
        print(f"repeat {r - WARMUP}: " + ", ".join(f"{k} {row[k]:.1f} ms" for k, _ in VARIANTS))
for k, t in times.items():
    print(f"median {k}: {statistics.median(t):.1f} ms over {len(t)} repeats (min {min(t):.1f}, max {max(t):.1f})")

ra, rb = packed(), through_fp32()
print(f"gaps found: {len(ra['gaps'])} | {len(rb['gaps'])} of {len(gaps)}; {int((ra['labels'] != rb['labels']).sum())} of {ra['labels'].numel()} labels differ; "
      f"{int((ra['patched'] != rb['repacked']).any(dim=-1).sum())} of {n} samples of patched differ from the repacked fp32 result")
del ra, rb
for name, fn in VARIANTS:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    print(f"peak device memory {name}: {(torch.cuda.max_memory_allocated() - before) / 2 ** 20:.1f} MiB above the {before / 2 ** 20:.1f} MiB held before the call")
for name, fn in VARIANTS:
    eng.ctx.profile_start(20000)
    fn()
    prof = {e["name"]: e for e in eng.ctx.profile_stop()}
    for fam in ("detect_bits", "detect_carry", "detect_count", "detect_offsets", "detect_emit", "cut_rate", "patch_rate"):
        if fam in prof and prof[fam]["launches"]:
            print(f"profiled {name}: {fam} {prof[fam]['launches']} launches, {prof[fam]['ms']:.3f} ms")
