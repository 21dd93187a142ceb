"""Experiment: what several gaps per clip cost at the bench shape (BASELINE configs[1]: 32 x 4 s clips, HuBERT-base bf16 + HiFi-GAN V1
fp16 stream, resident raw clips; step = masked log-mel front-end -> encoder -> arg-max / splice -> vocoder), in ONE process, the
variants alternated after warm-up, device-synchronised wall clock per block of `steps` steps:

  (a) one 200 ms gap per clip through the existing single-gap entry points (bench.py's step)
  (b) the same gap through the span route (span tables + frame table)
  (c) three 200 ms gaps per clip through the span route, one pass
  (d) what a caller pays today for (c): three sequential single-gap steps

The tables of (b) / (c) are built once, like bench.py's mask tensors.  Prints one line per repeat and the medians.

The time of the mask-reading kernels comes from a run of its own under the profiler, never from the timing run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/exp_multigap.py --variants ac --repeats 1 --steps 20
runs 3 warm-up + 20 timed steps of (a) and of (c) and nothing else; the single-span kernels of (a) and the `_spans` siblings of (c) have
different names, so `--kernel-stats DIR/*/*_kernel_stats.csv --repeats 1 --steps 20` (the profiled run's own counts; no GPU needed)
prints each family's time per step of (a) and of (c) from that one table.
usage: python tools/exp_multigap.py [--steps 10] [--repeats 5] [--variants abcd] | --kernel-stats CSV --repeats R --steps K"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from speech_inpainting_amd.engine import InpaintingEngine
from speech_inpainting_amd.native import SpanTable

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--variants", default="abcd", help="which of a, b, c, d to run")
ap.add_argument("--kernel-stats", metavar="CSV", default=None, help="read a rocprofv3 kernel_stats.csv of a `--variants ac` run; no GPU")
a = ap.parse_args()
WARMUP = 3
MASK_FAMS = ("wave_stats", "conv0_lagsums", "conv0_apply", "wave_peak", "mel_frames", "codebook_splice")

if a.kernel_stats:
    import csv
    per_step = a.repeats * a.steps + WARMUP                      # steps of (a), and of (c), in the profiled run
    tot = {"a": {}, "c": {}}
    allk = 0.0
    with open(a.kernel_stats, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("void ", "")
            ns = float(row["TotalDurationNs"])
            allk += ns
            fam = next((m for m in MASK_FAMS if name.startswith(m)), None)
            if fam is None:
                continue
            k = "c" if "_spans" in name.split("(")[0].split("<")[0] else "a"
            tot[k][fam] = tot[k].get(fam, 0.0) + ns
    for k in ("a", "c"):
        print(f"({k}) mask-reading kernels, ms per step: " + ", ".join(f"{m} {v / per_step * 1e-6:.4f}" for m, v in sorted(tot[k].items()))
              + f"; together {sum(tot[k].values()) / per_step * 1e-6:.4f}")
    print(f"all kernels of the run: {allk / per_step * 1e-6:.3f} ms per (a) step + (c) step")
    raise SystemExit(0)

B, N, LM = 32, 64000, 10
dev = torch.device("cuda:0")
harch, varch = HubertArch.base(), VocoderArch.v1()
eng = InpaintingEngine(harch, varch, 100, dev, "bf16", "fp16").load_state(
    synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100))
T = harch.num_frames(N)
n22 = N * 22050 // 16000
wave = synth.synth_wave(B, N, synth.DEFAULT_SEED + 3).to(dev)
wave22 = synth.synth_wave(B, n22, synth.DEFAULT_SEED + 6, sr=22050).to(dev)
# three disjoint 200 ms gaps per clip: one in each third of the clip, seeded
g = torch.Generator().manual_seed(5)
third = T // 3
gaps3 = [[(j * third + int(torch.randint(1, third - LM - 1, (1,), generator=g)), LM) for j in range(3)] for _ in range(B)]
gaps1 = [[clip[1]] for clip in gaps3]


def single_tensors(k):
    pos = torch.tensor([clip[k][0] for clip in gaps3], dtype=torch.int32, device=dev)
    return dict(pos=pos, ms=(pos * 320 + 80).to(torch.int32), ml=torch.full_like(pos, LM * 320 - 81),
                s22=(pos * 320 * 22050 // 16000).to(torch.int32), e22=((pos + LM) * 320 * 22050 // 16000).to(torch.int32))


def span_tensors(gaps):
    ci, fp, off = G.frame_table(gaps)
    tab = torch.tensor([ci, fp], dtype=torch.int32).to(dev)
    return dict(t16=SpanTable(G.spans16(gaps), dev), t22=SpanTable(G.spans22(gaps, [n22] * B), dev), fclip=tab[0].contiguous(), fpos=tab[1].contiguous())


S = [single_tensors(k) for k in range(3)]
P1, P3 = span_tensors(gaps1), span_tensors(gaps3)


def step_single(s):
    mel = eng.mel(wave22, s["s22"], s["e22"])
    return eng.predict_batch(wave, mel, s["pos"], LM, mask_start=s["ms"], mask_len=s["ml"])


def step_spans(p):
    mel = eng.mel(wave22, spans=p["t22"])
    feats = eng.encode(wave, spans=p["t16"])
    labels = eng.splice_spans(feats, p["fclip"], p["fpos"], mel)            # (mel is this step's own tensor: spliced in place)
    return {"feats": feats, "labels": labels, "mel": mel, "wave": eng.vocode(mel, stretch=True)}


variants = {"a": lambda: step_single(S[1]), "b": lambda: step_spans(P1), "c": lambda: step_spans(P3),
            "d": lambda: [step_single(s) for s in S][-1]}
variants = {k: fn for k, fn in variants.items() if k in a.variants}

if "a" in variants and "b" in variants:
    oa, ob = variants["a"](), variants["b"]()
    torch.cuda.synchronize()
    print("(b) equals (a): feats", torch.equal(oa["feats"], ob["feats"]), "labels", torch.equal(oa["labels"].reshape(-1), ob["labels"]),
          "wave", torch.equal(oa["wave"], ob["wave"]))
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
if set("abcd") <= set(variants):
    print(f"spread of (a) over {a.repeats} repeats: {max(ms['a']) - min(ms['a']):.3f} ms;  (b) - (a) {med['b'] - med['a']:+.3f}  (c) - (a) {med['c'] - med['a']:+.3f}  "
          f"(d) / (c) {med['d'] / med['c']:.2f}")
