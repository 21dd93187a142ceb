"""Experiment: what patch mode costs at the bench shape (BASELINE configs[1]: 32 x 4 s clips, HuBERT-base bf16 + HiFi-GAN V1 fp16 stream,
resident raw clips), in ONE process, the variants alternated inside each repeat after warm-up, device-synchronised wall clock per
block of `steps` steps:

  (a) today's step for one 200 ms gap per clip (masked log-mel -> encoder -> arg-max / splice -> FULL generator pass) + to_int16
  (b) engine.patch_multigap_batch(pcm=True) for the same gap: the generator over the windows the gap needs, composed into the
      caller's samples, int16 fused into the composition
  (c) (b) with three 200 ms gaps per clip

The gap tables of every variant are built once, like bench.py's mask tensors.  Prints one line per repeat, the medians, (a)'s own
repeat-to-repeat spread and the vocoded fraction of the stretched frames.

The kernels' rates come from a run of its own under the profiler, never from the timing run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/exp_patch.py --variants ab --repeats 1 --steps 20
then `--kernel-stats DIR/*/*_kernel_stats.csv --variants ab --repeats 1 --steps 20` (no GPU needed) prints the achieved bytes/s of
patch_compose and gather_windows beside pcm16 and upsample_stream, the path's HBM-bound yardsticks, from that one table.
usage: python tools/exp_patch.py [--steps 20] [--repeats 7] [--variants abc] | --kernel-stats CSV --variants V --repeats R --steps K"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--variants", default="abc", help="which of a, b, c to run")
ap.add_argument("--fade", type=int, default=110)
ap.add_argument("--kernel-stats", metavar="CSV", default=None, help="read a rocprofv3 kernel_stats.csv of a profiled run; no GPU")
a = ap.parse_args()
WARMUP = 3
B, N, LM, HOP = 32, 64000, 10, 256
n22 = N * 22050 // 16000

if a.kernel_stats:
    import csv
    # bytes per launch, by the kernels' own contracts: compose reads 4 and writes 4 + 2 per sample (fp32 + int16 out), pcm16 reads 4 and
    # writes 2; the gather's and the upsampler's bytes depend on the windows, so they are reported as time and calls only
    n_out = (((n22 + 624 - 1024) // 441 + 1) * 441 // 256) * HOP
    per_call = {"patch_compose_kernel": 10.0 * B * n22, "pcm16_kernel": 6.0 * B * n_out}
    print(f"{'kernel':<44}{'calls':>8}{'avg us':>11}{'GB/s':>9}")
    with open(a.kernel_stats, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("void ", "").split("(")[0]
            if not any(k in name for k in ("patch_compose", "gather_windows", "pcm16", "upsample_stream", "wave_peak")):
                continue
            calls, ns = int(row["Calls"]), float(row["TotalDurationNs"])
            nb = next((v for k, v in per_call.items() if name.startswith(k)), None)
            rate = f"{nb * calls / ns:9.1f}" if nb else f"{'-':>9}"
            print(f"{name[:43]:<44}{calls:>8}{ns / calls * 1e-3:>11.2f}{rate}")
    raise SystemExit(0)

import torch

from speech_inpainting_amd import synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from speech_inpainting_amd.engine import InpaintingEngine

dev = torch.device("cuda:0")
harch, varch = HubertArch.base(), VocoderArch.v1()
eng = InpaintingEngine(harch, varch, 100, dev, "bf16", "fp16").load_state(
    synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100))
T = harch.num_frames(N)
wave = synth.synth_wave(B, N, synth.DEFAULT_SEED + 3).to(dev)
wave22 = synth.synth_wave(B, n22, synth.DEFAULT_SEED + 6, sr=22050).to(dev)
g = torch.Generator().manual_seed(5)
third = T // 3
gaps3 = [[(j * third + int(torch.randint(1, third - LM - 1, (1,), generator=g)), LM) for j in range(3)] for _ in range(B)]
gaps1 = [[clip[1]] for clip in gaps3]
T1 = eng.gap_tables(gaps1, [N] * B, [n22] * B)
P1 = eng.gap_tables(gaps1, [N] * B, [n22] * B, patch_fade=a.fade)
P3 = eng.gap_tables(gaps3, [N] * B, [n22] * B, patch_fade=a.fade)


def step_full():
    out = eng.predict_multigap_batch(wave, wave22, gaps1, tables=T1)
    out["pcm"] = eng.to_int16(out["wave"])
    return out


variants = {"a": step_full,
            "b": lambda: eng.patch_multigap_batch(wave, wave22, gaps1, fade=a.fade, tables=P1, pcm=True),
            "c": lambda: eng.patch_multigap_batch(wave, wave22, gaps3, fade=a.fade, tables=P3, pcm=True)}
variants = {k: fn for k, fn in variants.items() if k in a.variants}
t_out = eng.ctx.vocoder_samples(eng.ctx.mel_frames(n22), True) // HOP
for k, p in (("b", P1), ("c", P3)):
    fr = [sum(w1 - w0 for w0, w1 in w) for w in p["patch"]["windows"]]
    print(f"({k}) vocoded stretched frames per clip: mean {sum(fr) / B:.1f} of {t_out} ({sum(fr) / B / t_out:.1%}), {len(p['patch']['wins'])} windows, "
          f"longest {max(w1 - w0 for _, w0, w1 in p['patch']['wins'])} frames")
if "a" in variants and "b" in variants:
    oa, ob = variants["a"](), variants["b"]()
    torch.cuda.synchronize()
    gain = eng.ctx.wave_peak(wave22, T1["tab22"]) / 0.95
    s, l = T1["tab22"].spans()[0][0]
    print("(b) inside the gap of clip 0 equals gain x (a)'s wave:", torch.equal(ob["patched"][0, s:s + l], gain[0] * oa["wave"][0, s:s + l]),
          " outside:", torch.equal(ob["patched"][0, :s - a.fade], wave22[0, :s - a.fade]))
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
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    print(f"repeat {r}: " + "  ".join(f"({k}) {ms[k][-1]:.3f} ms" for k in variants), flush=True)
med = {k: statistics.median(v) for k, v in ms.items()}
print("median ms/step: " + "  ".join(f"({k}) {med[k]:.3f}" for k in variants))
if "a" in variants:
    print(f"spread of (a) over {a.repeats} repeats: {max(ms['a']) - min(ms['a']):.3f} ms;  "
          + "  ".join(f"({k}) - (a) {med[k] - med['a']:+.3f}" for k in variants if k != "a"))
