"""Experiment: what a long recording costs.  A 10-minute synthetic recording at 22.05 kHz with 60 gaps of 200 ms, one
every 10 s (each gap gets a context of its own: 60 contexts of 4 s, two passes of 32 and 28), HuBERT-base bf16 + HiFi-GAN V1 fp16
stream, in ONE process, the variants alternated inside each repeat after warm-up, device-synchronised wall clock per call:

  (a) engine.patch_recording(pcm=True): si_cut_clips, the multi-gap pass, the generator over the own gaps' windows, ONE si_patch_regions
      per pass into the clone of the recording
  (b) the per-context route a caller would write (the reference of tests/test_gpu_long.py): torch slicing into a stacked batch,
      patch_multigap_batch(pcm=True) -- a full (32, 88200) compose per pass -- and two slice pastes (fp32, int16) per gap into clones

Both resample the cut 22.05 kHz clips to 16 kHz per pass and plan on the host inside the timed call.  Prints whether (a) equals (b) bit
for bit, one line per repeat, the medians and (b)'s own repeat-to-repeat spread, then -- from a separate, untimed run under the
library's profiler -- the per-kernel times of cut_clips and patch_regions beside (b)'s patch_compose.
usage: python tools/exp_long.py [--repeats 7] [--minutes 10] [--gaps 60] [--fade 110]"""
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
a = ap.parse_args()
WARMUP = 2
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
N22 = int(a.minutes * 60 * 22050) + 123
n_rec = N22 // 441
# one 30 s stretch of synthetic speech, tiled: the content does not matter to the clock, its level and spectrum do to the arg-max
tile = synth.synth_wave(1, 30 * 22050, synth.DEFAULT_SEED + 6, sr=22050)[0]
wave22 = tile.repeat(-(-N22 // tile.numel()))[:N22].contiguous().to(dev)
every = n_rec // a.gaps
gaps = [(k * every + every // 2, LM) for k in range(a.gaps)]
n22, n16 = CLIP * 441, CLIP * 320
lim = min(eng.ctx.num_frames(n16), eng.ctx.mel_frames(n22))
n_out = eng.ctx.vocoder_samples(eng.ctx.mel_frames(n22), True)


def long_route():
    return eng.patch_recording(wave22, gaps, fade=a.fade, clip_frames=CLIP, min_context=CTX, batch=a.batch, pcm=True)


def per_context_route():
    plan = G.plan_contexts(gaps, n_rec, CLIP, CTX, lim_frames=lim)
    patched, pcm = wave22.clone(), eng.to_int16(wave22)
    for i in range(0, len(plan), a.batch):
        cb = plan[i:i + a.batch]
        cut22 = torch.stack([wave22[441 * c["start"]:441 * c["start"] + n22] for c in cb])
        out = eng.patch_multigap_batch(eng.resample(cut22, 22050, 16000), cut22, [c["own"] + c["foreign"] for c in cb], fade=a.fade, pcm=True)
        for b, c in enumerate(cb):
            s0 = 441 * c["start"]
            for lo, hi in G.blend_regions(G.spans22([c["own"]], [n22])[0], n22, n_out, a.fade):
                patched[s0 + lo:s0 + hi] = out["patched"][b, lo:hi]
                pcm[s0 + lo:s0 + hi] = out["patched_pcm"][b, lo:hi]
    return {"patched": patched, "patched_pcm": pcm, "contexts": plan}


variants = {"a": long_route, "b": per_context_route}
oa, ob = long_route(), per_context_route()
torch.cuda.synchronize()
print(f"recording of {N22} samples ({N22 / 22050 / 60:.2f} min), {len(gaps)} gaps of {LM} frames, {len(oa['contexts'])} contexts, passes of {a.batch}")
print("(a) equals (b) bit for bit: fp32", torch.equal(oa["patched"].view(torch.int32), ob["patched"].view(torch.int32)),
      " int16", torch.equal(oa["patched_pcm"], ob["patched_pcm"]))
del oa, ob
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
print(f"spread of (b) over {a.repeats} repeats: {max(ms['b']) - min(ms['b']):.3f} ms;  (a) - (b) {med['a'] - med['b']:+.3f} ms")
# per-kernel device times, from a run of their own under the library's event profiler (every launch bracketed: not a step time)
for k, fn in variants.items():
    eng.ctx.profile_start(20000)
    fn()
    rows = {e["name"]: e for e in eng.ctx.profile_stop()}
    total = sum(e["ms"] for e in rows.values())
    line = "  ".join(f"{n} {rows[n]['launches']} x {rows[n]['ms'] / rows[n]['launches'] * 1e3:.1f} us"
                     for n in ("cut_clips", "patch_regions", "patch_compose", "pcm16", "wave_peak", "gather_windows") if n in rows and rows[n]["launches"])
    print(f"({k}) profiled kernels: {total:.3f} ms in all;  {line}")
