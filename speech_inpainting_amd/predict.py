"""`predict.py` entry point of the I_ea path, re-stated over the HIP engine.

Run as the reference is run (I_ea/predict.py:58-62): from a directory holding `predict.yaml`

    python -m speech_inpainting_amd.predict            # or: python predict.py

It reads the reference's YAML schema, loads the same three artefacts (CustomModel `.pt` / local HF directory, HiFi-GAN
`generator` checkpoint + `config.json`, joblib k-means codebook), and writes the reference's output files
`<save_pred>/<wave_name>/{orig,masked,hifi_masked,expected_inpaint,inpainted}.wav` (I_ea/predict.py:84,128,134,201,207;
`expected_inpaint.wav` only when the ground-truth label file exists).  `predict_clips` is the importable batch form.

With an optional `long:` mapping ({clip_s: 4.0, context_s: 1.0, batch: 32, rate: 22050 | file}) the file is a RECORDING of any length: the gaps of
`mask:` / `masks:` are read on the file's own time axis, the recording is served as context clips (engine.patch_recording, DESIGN.md
4.14; the cross-fade comes from `patch:`, 5 ms without it) and `orig.wav`, `masked.wav` and `patched.wav` are written at 22.05 kHz,
all with the recording's own sample count.  The whole-clip diagnostics (`hifi_masked.wav`, `inpainted.wav`, `expected_inpaint.wav`)
are NOT produced on this route: no generator pass over a whole recording exists there.  With a `detect:` mapping ({threshold: 0.0,
min_ms: 5.0, max_ms: 400.0, pad_frames: 0}) beside `long:` and instead of `mask:` / `masks:` the gaps are FOUND: the runs of
|x| <= threshold of at least min_ms in the file's own samples (engine.find_gaps); each gap and each skipped run is
printed and `gaps.json` is written beside the three waves.  `detect:` also takes `kind:` (quiet, the default; held: samples that
repeat a neighbour, as an underrun or a DC level leaves them; any), `rel_threshold:` (a fraction of the file's own peak: the
threshold is max(threshold, rel_threshold * peak)) and `held_tol:` (full scale, like threshold); off their defaults the effective
threshold is printed and gaps.json records `kind` and `T` (engine.find_dead_runs).  `kind: level` with `win_ms:` (2 by
default) finds a dropout that is a noise floor -- dither, a concealer's comfort noise -- by the RMS level of a window of win_ms
milliseconds against the threshold, and gaps.json records `kind`, `T` and `win_ms` (engine.find_level_runs).  `kind: burst`
finds damage that is LOUDER than the speech -- a block of corrupted PCM: random data, swapped or misaligned bytes -- by the RMS level of the
second difference over a window of `win_ms:` (4 by default at this kind) at or above `threshold:`; start from `threshold: 1.15` of full
scale, and a threshold of 0 is refused (engine.find_burst_runs).  `kind: impulse` finds clicks and pops of one to a few
in-range samples by their AR prediction error against that of their own neighbourhood (`ratio:` 10, `order:` 16, `guard:` 4, `pad:` 2,
`win_ms:` 23; give `min_ms: 0`, and `mend_ms: 1` to mend them in place; engine.find_impulse_runs).  `kind: invalid` finds a float file's samples whose
VALUE is the damage -- NaN, inf and, with `threshold:` (the ceiling, in full-scale units; 0 or absent: none), |x| above it; `min_ms:`
defaults to 0 at this kind, gaps.json records `kind` and `ceiling`, and the same ceiling keeps those samples out of the clips the model
is fed; it needs `long: {rate: file, feed: contexts}` unless the file is at 22.05 kHz (engine.find_invalid_runs).  With `mend_ms:` (and optionally
`mend_order:`, `mend_context:`) inside `detect:`, on the `rate: file` routes only, the runs of at most mend_ms milliseconds (at most 64
samples) are filled from their own neighbourhood by least-squares AR interpolation instead of a generated frame, only the rest is
inpainted, and gaps.json records `mended`, a count by status (engine.mend_runs).  With `rate: file` inside `long:` the recording is NOT brought to 22.05 kHz
on the way out: the three waves keep the file's own rate and sample type (an int16 file stays int16), and patched.wav holds the file's
own samples, bit for bit, outside the cross-fades (engine.patch_file).
With `feed: contexts` beside `rate: file` the recording is not resampled as a whole on the way in either: only the context clips
are cut from it, at its own rate and in its own sample type (si_cut_rate); `feed: recording` is the default.
With `clips16: file` beside `feed: contexts` the encoder's 16 kHz clips are cut straight from the file too, in the same launch, instead
of being resampled from the 22.05 kHz clips (si_cut_pair): a 16 kHz file's own samples reach the encoder; the key is
printed, and recorded in gaps.json when `detect:` writes one.  `clips16: resampled` is the default.
A multi-channel file of up to 8 channels is served with `rate: file, feed: contexts`: it stays interleaved, every
channel is repaired as the mono recording it is to the model, and the three waves are written multi-channel; with `rate: file` and the
default `feed: recording` it is refused, as it was (that feed would de-interleave it).  `mask:` / `masks:` apply to every
channel; `detect:` takes `channels: each` (the default: every channel is scanned and repaired on its own, gaps.json holds one list
per channel) or `channels: joint` (a gap is where ALL channels are quiet, repaired in all of them).  Without `rate: file` a
multi-channel file is mixed down to one channel at 22.05 kHz, as before.

Differences from the script, all outside the three replaced subsystems: no Whisper `Metrics` object is built (the
script constructs it and never uses it, I_ea/predict.py:72-73), PNG plots are skipped, and the two `librosa.load` calls are one
wav read plus the resampler librosa 0.9.1 itself uses (resampy `kaiser_best`) run on the GPU (si_resample_sinc; pinned against the
reference-held LJ001-0001 22k / 16k pair), the clips staying on the device from there to the int16 conversion (si_pcm16).
"""
from __future__ import annotations

import json
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import audio
from . import gaps as G
from .arch import HubertArch, VocoderArch
from .checkpoint import arch_for_type, load_codebook, load_generator_checkpoint, load_hubert_checkpoint
from .config import PredictConfig, choose_device, load_predict_config
from .engine import InpaintingEngine


def build_engine(cfg: PredictConfig, device: Optional[torch.device] = None, encoder_dtype: str = "fp32",
                 vocoder_dtype: str = "fp32") -> InpaintingEngine:
    device = device or choose_device(cfg.device_index)
    if device.type != "cuda":
        raise RuntimeError("no GPU selected/available: this package has no CPU path (device.index in the YAML)")
    hsd, harch = load_hubert_checkpoint(cfg.hubert_checkpoint, cfg.hubert_type)
    harch = harch or arch_for_type(cfg.hubert_type)
    gsd, varch = load_generator_checkpoint(cfg.hifigan_checkpoint)
    cb = load_codebook(cfg.km_model_path)
    if cb.shape[0] != cfg.n_clusters:
        raise ValueError(f"{cfg.km_model_path}: {cb.shape[0]} centroids but km_model.n_clusters = {cfg.n_clusters}")
    eng = InpaintingEngine(harch, varch, cfg.n_clusters, device, encoder_dtype, vocoder_dtype)
    return eng.load_state(hsd, gsd, cb)


def check_mask_span(engine: InpaintingEngine, n16: int, n22: int, mask_pos: Sequence[int], mask_frames: int) -> None:
    """The masked frames must exist on both sides: [pos, pos + Lm) inside the T encoder frames AND the Tm mel frames
    (for a 4 s clip T = 199 but Tm = 200).  The reference fails on the slice-shape mismatch at I_ea/predict.py:166-168,
    185-187; the kernels would leave such frames unspliced (label -1), so refuse here where positions are host ints."""
    T, Tm = engine.ctx.num_frames(n16), engine.ctx.mel_frames(n22)
    for i, p in enumerate(mask_pos):
        if int(p) < 0 or int(p) + int(mask_frames) > min(T, Tm):
            raise ValueError(f"clip {i}: masked frames [{int(p)}, {int(p) + int(mask_frames)}) do not fit the clip "
                             f"({T} encoder frames, {Tm} mel frames)")


def _one_of(mask_pos, mask_frames, gaps, blind: bool) -> None:
    if gaps is not None and (mask_pos is not None or mask_frames is not None or blind):
        raise ValueError("give either mask_pos / mask_frames (one gap per clip) or gaps= (several), not both; blind mode takes no gaps")
    if gaps is None and (mask_pos is None or mask_frames is None):
        raise ValueError("mask_pos and mask_frames (or gaps=) are required")


def _single_span22(mask_pos, mask_frames: int, mask22, n22: Sequence[int], dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """[start, end) of the one span zeroed per clip on the 22.05 kHz side, int32 (B) each on the device: the frame span
    (gaps.spans22, I_ea/predict.py:99-100) or the explicit `mask22` pairs, clamped to each clip's n22 samples."""
    if mask22 is None:
        pairs = [(s, s + l) for (s, l), in G.spans22([[(int(p), int(mask_frames))] for p in mask_pos], n22)]
    else:
        pairs = [(min(max(int(a), 0), n), min(max(int(b), 0), n)) for (a, b), n in zip(mask22, n22)]
    return tuple(torch.tensor(col, dtype=torch.int32, device=dev) for col in zip(*pairs))


def predict_clips(engine: InpaintingEngine, waves16: Sequence[np.ndarray], waves22: Sequence[np.ndarray],
                  mask_pos: Optional[Sequence[int]] = None, mask_frames: Optional[int] = None, blind: bool = False,
                  mask22: Optional[Sequence[Tuple[int, int]]] = None, diagnostics: bool = False,
                  target_labels: Optional[torch.Tensor] = None, gaps=None, patch: bool = False, fade: int = 110) -> Dict[str, torch.Tensor]:
    """Batch form of I_ea/predict.py:97-207 for clips of EQUAL length.
    waves16 / waves22: the same clips at 16 kHz / 22.05 kHz (float32, un-normalised), mask_pos: first masked 20 ms frame.
    mask22: per-clip [start, end) of the span zeroed on the 22.05 kHz side (predict.py:99-102: the 16 kHz sample
    positions of the YAML times scaled by 22050 // 16000); default = the frame span.
    diagnostics=True adds the script's other two vocoder passes as batch outputs: `hifi_masked` (the generator on the
    masked mel alone, predict.py:123-128) and -- when `target_labels` (B, Lm) int64 ground-truth codewords are given --
    `expected_inpaint` (their centroids spliced instead of the predicted ones, predict.py:177-189,198-201) plus the
    codeword metrics of predict.py:171-173 (`loss`, `cos_pred_target`).
    gaps: instead of mask_pos / mask_frames, per clip a list of (first frame, frame count) -- several gaps per clip, different per
    clip, in one pass (engine.predict_multigap_batch).  `labels` is then flat (F,) with `label_off` (B + 1), `target_labels` flat (F,)
    in the same order, and mask22 per clip a list of [start, end) pairs, one per gap in sorted order.
    patch=True (not with blind): PATCH MODE -- adds `patched` (B, n22): the caller's own 22.05 kHz samples, bit for bit, outside a
    cross-fade of `fade` samples around each gap, the generator's audio at the recording's level inside (engine.patch_multigap_batch;
    the generator then runs only over the windows the gaps need and there is no `wave`, unless diagnostics=True asks for the full
    passes anyway)."""
    dev = engine.device
    n16, n22 = len(waves16[0]), len(waves22[0])
    if any(len(w) != n16 for w in waves16) or any(len(w) != n22 for w in waves22):
        raise ValueError("clips in one batch must have equal length (predict_clips_ragged / predict_ragged take clips of "
                         "different lengths)")
    wave22 = torch.from_numpy(np.stack([np.asarray(w, dtype=np.float32) for w in waves22])).to(dev)
    wave = torch.from_numpy(np.stack([np.asarray(w, dtype=np.float32) for w in waves16])).to(dev)
    return predict_resident(engine, wave, wave22, mask_pos, mask_frames, blind, mask22, diagnostics, target_labels, gaps, patch, fade)


def _predict_gaps(engine: InpaintingEngine, wave: torch.Tensor, wave22: torch.Tensor, gaps, mask22, diagnostics: bool,
                  target_labels: Optional[torch.Tensor], len16=None, len22=None, patch: bool = False, fade: int = 110) -> Dict[str, object]:
    """The multi-gap body of predict_resident / predict_clips_ragged.  diagnostics: ONE full generator pass over the masked mel
    (`hifi_masked`); `wave` and `expected_inpaint` come from windowed passes over the merged windows around the gaps
    (engine.vocode_windows: bit-identical to full passes).  patch: `patched` by engine.patch_multigap_batch, or -- with diagnostics,
    where the full `wave` exists anyway -- by engine.patch_from_wave."""
    if patch and not diagnostics:
        return engine.patch_multigap_batch(wave, wave22, gaps, fade=fade, len16=len16, len22=len22, spans22=mask22)
    tables = None
    if patch:
        B = wave.shape[0]
        tables = engine.gap_tables(gaps, len16 if len16 is not None else [wave.shape[1]] * B, len22 if len22 is not None else [wave22.shape[1]] * B,
                                   spans22=mask22)
    out = engine.predict_multigap_batch(wave, wave22, gaps, len16=len16, len22=len22, spans22=mask22, tables=tables, vocode=not diagnostics)
    if not diagnostics:
        return out
    mlen = out["mel_len"] if len16 is not None else None
    mel = out["mel_masked"]
    base = engine.vocode_ragged(mel, mlen, stretch=True) if mlen is not None else engine.vocode(mel, stretch=True)
    out["hifi_masked"] = base
    out["wave"] = engine.vocode_windows(base, out["mel"], out["gaps"], mlen)
    if target_labels is not None:
        tgt = target_labels.to(engine.device, torch.int64).reshape(-1).contiguous()
        exp = mel.clone()
        engine.splice_labels_spans(tgt, out["frame_clip"], out["frame_pos"], exp)
        out["expected_inpaint"] = engine.vocode_windows(base, exp, out["gaps"], mlen)
        m = engine.codebook_metrics_spans(out["feats"], out["frame_clip"], out["frame_pos"], tgt)
        out["loss"], out["cos_pred_target"] = m["loss"], m["cos_pred_target"]
    if patch:
        out["patched"], _ = engine.patch_from_wave(wave22, out["wave"], tables["tab22"], fade, len22, out.get("wave_len"))
    return out


def _patch_args(patch: bool, blind: bool, gaps, mask_pos, mask_frames):
    """Patch mode's routing: it keeps what lies outside the gaps, so blind mode (every frame replaced) has nothing to keep; a single
    mask_pos / mask_frames gap is one gap per clip on the multi-gap route."""
    if not patch:
        return gaps
    if blind:
        raise ValueError("patch=True with blind=True: blind mode replaces every frame, there is nothing of the recording to keep")
    return gaps if gaps is not None else [[(int(p), int(mask_frames))] for p in mask_pos]


def predict_resident(engine: InpaintingEngine, wave: torch.Tensor, wave22: torch.Tensor, mask_pos: Optional[Sequence[int]] = None,
                     mask_frames: Optional[int] = None, blind: bool = False, mask22: Optional[Sequence[Tuple[int, int]]] = None,
                     diagnostics: bool = False, target_labels: Optional[torch.Tensor] = None, gaps=None, patch: bool = False,
                     fade: int = 110) -> Dict[str, torch.Tensor]:
    """`predict_clips` on clips that are already on the GPU: wave (B, n16) / wave22 (B, n22) float32 device tensors (e.g. straight
    out of `engine.resample`); same outputs."""
    _one_of(mask_pos, mask_frames, gaps, blind)
    if patch and gaps is None and not blind:
        # one gap per clip on the multi-gap route: mask22 becomes one [start, end) pair per clip's only gap, target labels go flat
        check_mask_span(engine, wave.shape[1], wave22.shape[1], mask_pos, mask_frames)
        mask22 = None if mask22 is None else [[m] for m in mask22]
        target_labels = None if target_labels is None else target_labels.reshape(-1)
    gaps = _patch_args(patch, blind, gaps, mask_pos, mask_frames)
    if gaps is not None:
        return _predict_gaps(engine, wave, wave22, gaps, mask22, diagnostics, target_labels, patch=patch, fade=fade)
    dev = engine.device
    n16, n22 = wave.shape[1], wave22.shape[1]
    if not blind:
        check_mask_span(engine, n16, n22, mask_pos, mask_frames)
    if blind:
        mel = engine.mel(wave22)                                                    # nothing zeroed; predict.py:104-106
    else:
        s22, e22 = _single_span22(mask_pos, mask_frames, mask22, [n22] * len(mask_pos), dev)
        mel = engine.mel(wave22, s22, e22)                                          # predict.py:99-106 on the GPU
    pos = torch.tensor(list(mask_pos), dtype=torch.int32, device=dev)
    if diagnostics and not blind:
        # The script's three generator passes (masked / expected / inpainted mel, I_ea/predict.py:123-128,196-207) differ only in the
        # Lm spliced frames: ONE full pass (the masked mel), the other two over the window the spliced frames can reach
        # (engine.vocode_window: bit-identical to full passes).
        feats = engine.encode(wave, (pos * 320 + 80).to(torch.int32), torch.full_like(pos, max(mask_frames * 320 - 81, 0)))
        mel2 = mel.clone()
        labels = engine.splice(feats, pos, mask_frames, mel2)
        base = engine.vocode(mel, stretch=True)
        out = {"feats": feats, "labels": labels, "mel": mel2, "hifi_masked": base,
               "wave": engine.vocode_window(base, mel2, list(mask_pos), mask_frames)}
    else:
        out = engine.predict_batch(wave, mel, pos, mask_frames, blind=blind)
        if diagnostics:
            out["hifi_masked"] = engine.vocode(mel, stretch=True)
    out["mel_masked"] = mel
    if diagnostics:
        if target_labels is not None and not blind:
            tgt = target_labels.to(dev, torch.int64).contiguous()
            exp = mel.clone()
            engine.splice_labels(tgt, pos, exp)
            out["expected_inpaint"] = engine.vocode_window(out["hifi_masked"], exp, list(mask_pos), mask_frames)
            m = engine.codebook_metrics(out["feats"], pos, mask_frames, tgt)
            out["loss"], out["cos_pred_target"] = m["loss"], m["cos_pred_target"]
    return out


def bucket_by_length(lengths: Sequence[int], max_batch: int = 32) -> List[List[int]]:
    """Group clip indices into batches of EXACTLY equal length (at most `max_batch` each), longest first, original
    order kept inside a group.  HuBERT-base's GroupNorm over time and the processor's per-clip normalisation make
    padded batches differ from the reference's one-clip-at-a-time loop (I_ea/predict.py:76-207 handles one file),
    so ragged inputs are bucketed instead of padded."""
    groups: Dict[int, List[int]] = {}
    for i, n in enumerate(lengths):
        groups.setdefault(int(n), []).append(i)
    out: List[List[int]] = []
    for n in sorted(groups, reverse=True):
        idx = groups[n]
        out.extend(idx[k:k + max_batch] for k in range(0, len(idx), max_batch))
    return out


def plan_ragged_batches(lengths: Sequence[int], max_batch: int = 32, max_waste: Optional[float] = None) -> List[List[int]]:
    """Clip indices sorted by length (longest first) and cut into batches of at most `max_batch`; with `max_waste` a batch is also
    closed before its STORAGE padding 1 - sum(len) / (n * longest) would exceed it.  (The kernels number their tiles clip by clip
    without gaps, so padding costs memory, not launched work: one full batch fills the chip best.)"""
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    out: List[List[int]] = []
    cur: List[int] = []
    tot = 0
    for i in order:
        n = int(lengths[i])
        if cur:
            longest = int(lengths[cur[0]])
            waste = 1.0 - (tot + n) / ((len(cur) + 1) * longest)
            if len(cur) >= max_batch or (max_waste is not None and waste > max_waste):
                out.append(cur)
                cur, tot = [], 0
        cur.append(i)
        tot += n
    if cur:
        out.append(cur)
    return out


def storage_padding(lengths: Sequence[int], batches: Sequence[Sequence[int]]) -> float:
    """Fraction of the padded (batch, longest) storage that holds no sample, over all batches."""
    real = sum(int(lengths[i]) for b in batches for i in b)
    padded = sum(len(b) * max(int(lengths[i]) for i in b) for b in batches)
    return 1.0 - real / max(padded, 1)


def pad_stack(waves: Sequence[np.ndarray]) -> Tuple[torch.Tensor, List[int]]:
    """Clips of different lengths -> pinned-memory-free (B, longest) float32 host tensor (zero tail) + their lengths."""
    lens = [len(w) for w in waves]
    out = torch.zeros(len(waves), max(lens), dtype=torch.float32)
    for i, w in enumerate(waves):
        out[i, :lens[i]] = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
    return out, lens


def predict_clips_ragged(engine: InpaintingEngine, waves16: Sequence[np.ndarray], waves22: Sequence[np.ndarray],
                         mask_pos: Optional[Sequence[int]] = None, mask_frames: Optional[int] = None, blind: bool = False,
                         mask22: Optional[Sequence[Tuple[int, int]]] = None, gaps=None, diagnostics: bool = False,
                         target_labels: Optional[torch.Tensor] = None, patch: bool = False, fade: int = 110) -> Dict[str, object]:
    """`predict_clips` for clips of DIFFERENT lengths in ONE set of launches (the library's ragged-batch entry points): every
    clip's outputs equal that clip's alone.  Tensors are (B, longest ...); `wave_len`, `frames`, `mel_len` give each clip's extent.
    gaps (with diagnostics / target_labels): several gaps per clip, as predict_clips.  patch / fade: patch mode, as predict_clips
    (`patched` (B, longest n22); clip b's own samples are its first len(waves22[b]))."""
    dev = engine.device
    _one_of(mask_pos, mask_frames, gaps, blind)
    if patch and gaps is None and not blind:
        for i, (a, b) in enumerate(zip(waves16, waves22)):
            check_mask_span(engine, len(a), len(b), [mask_pos[i]], mask_frames)
        mask22 = None if mask22 is None else [[m] for m in mask22]
        target_labels = None if target_labels is None else target_labels.reshape(-1)
    gaps = _patch_args(patch, blind, gaps, mask_pos, mask_frames)
    if gaps is not None:
        w22, len22 = pad_stack(waves22)
        w16, len16 = pad_stack(waves16)
        return _predict_gaps(engine, w16.to(dev), w22.to(dev), gaps, mask22, diagnostics, target_labels, len16, len22, patch, fade)
    if diagnostics or target_labels is not None:
        raise ValueError("predict_clips_ragged: diagnostics are served on the gaps= route")
    if not blind:
        for i, (a, b) in enumerate(zip(waves16, waves22)):
            check_mask_span(engine, len(a), len(b), [mask_pos[i]], mask_frames)
    w22, len22 = pad_stack(waves22)
    w16, len16 = pad_stack(waves16)
    wave22 = w22.to(dev)
    if blind:
        mel = engine.mel_ragged(wave22, len22)
    else:
        s22, e22 = _single_span22(mask_pos, mask_frames, mask22, len22, dev)
        mel = engine.mel_ragged(wave22, len22, s22, e22)
    mel_len = [engine.ctx.mel_frames(n) for n in len22]
    pos = torch.tensor(list(mask_pos), dtype=torch.int32, device=dev)
    out = engine.predict_ragged_batch(w16.to(dev), len16, mel, mel_len, pos, mask_frames, blind=blind)
    out["mel_masked"] = mel
    return out


def predict_ragged(engine: InpaintingEngine, waves16: Sequence[np.ndarray], waves22: Sequence[np.ndarray],
                   mask_pos: Sequence[int], mask_frames: int, blind: bool = False, max_batch: int = 32,
                   max_waste: Optional[float] = None, exact_length: bool = False) -> List[Dict[str, torch.Tensor]]:
    """The path over clips of DIFFERENT lengths (BASELINE configs[4]; the reference runs one file of any length per invocation,
    I_ea/predict.py:76-207): clips are sorted by length and cut into ragged batches (`plan_ragged_batches`) that share every
    launch; each clip's result equals that clip run alone.  Returns one dict per input clip, in input order, cut to the clip's own
    extent (tensors keep a batch dimension of 1).  exact_length=True is the older route -- batches of EXACTLY equal length through
    the uniform entry points (singletons on continuous lengths) -- kept as the reference the ragged route is tested against."""
    if not (len(waves16) == len(waves22) == len(mask_pos)):
        raise ValueError("waves16, waves22 and mask_pos must have one entry per clip")
    results: List[Optional[Dict[str, torch.Tensor]]] = [None] * len(waves16)
    if exact_length:
        # a bucket must agree on BOTH sample counts (the 22.05 kHz length follows from the resampler's rounding)
        keys = [len(a) * 1_000_003 + len(b) for a, b in zip(waves16, waves22)]
        for idx in bucket_by_length(keys, max_batch):
            out = predict_clips(engine, [waves16[i] for i in idx], [waves22[i] for i in idx], [mask_pos[i] for i in idx],
                                mask_frames, blind=blind)
            for k, i in enumerate(idx):
                results[i] = {name: v[k:k + 1] for name, v in out.items()}
        return results  # type: ignore[return-value]
    for idx in plan_ragged_batches([len(w) for w in waves16], max_batch, max_waste):
        out = predict_clips_ragged(engine, [waves16[i] for i in idx], [waves22[i] for i in idx], [mask_pos[i] for i in idx],
                                   mask_frames, blind=blind)
        for k, i in enumerate(idx):
            T, Tm, nl, nw = out["frames"][k], out["mel_len"][k], out["label_cnt"][k], out["wave_len"][k]
            results[i] = {"feats": out["feats"][k:k + 1, :T], "labels": out["labels"][k:k + 1, :nl], "mel": out["mel"][k:k + 1, :, :Tm],
                          "mel_masked": out["mel_masked"][k:k + 1, :, :Tm], "wave": out["wave"][k:k + 1, :nw]}
    return results  # type: ignore[return-value]


def _detect_gaps(cfg: PredictConfig, engine: InpaintingEngine, raw: np.ndarray, sr_file: int, n22: int, fade: int, clip_frames: int,
                 min_context: int, save_dir: str, x24: Optional[np.ndarray] = None) -> List[Tuple[int, int]]:
    """The `detect:` key of the `long:` route: the gaps found in the file's OWN samples at the file's rate, where a dropout is still
    exact zeros (the resampler's ringing fills it in at 22.05 kHz).  A mono int16 file is scanned as the int16 it holds, the threshold
    scaled by 32768 (an exact scaling: the same samples are quiet).  Prints every gap and every skipped run, writes gaps.json.
    With `kind:`, `rel_threshold:` or `held_tol:` off their defaults it also prints the effective threshold and records
    `kind` and `T` in gaps.json.  x24: the packed bytes (n, 3) of a 24-bit file under `pcm24: keep`, scanned as they
    are with the threshold scaled by 2^23."""
    from scipy.io import wavfile
    d = cfg.detect
    x, scale = raw, 1.0
    if x24 is not None:
        x, scale = x24, 8388608.0
    else:
        pcm_file = wavfile.read(cfg.wave_path)[1]
        if pcm_file.dtype == np.int16 and pcm_file.ndim == 1:
            x, scale = pcm_file, 32768.0
    n_rec, lim = engine.recording_frames(n22, clip_frames)
    max_ms = d["max_ms"] if n_rec <= clip_frames else min(d["max_ms"], 20.0 * (clip_frames - 2 * min_context))
    found = engine.find_gaps(x, sr_file, d["threshold"] * scale, d["min_ms"], max_ms, d["pad_frames"], None, fade, n_rec, lim,
                             **dead_keywords(cfg.detect_dead, scale), **level_keywords(cfg), **impulse_keywords(cfg))
    report = _dead_report(cfg, found, scale)
    for k, (pos, lm) in enumerate(found["gaps"]):
        print(f"Detected gap {k} = frames [{pos}, {pos + lm}) = {pos * 0.02:.2f} s .. {(pos + lm) * 0.02:.2f} s")
    for pos, lm, why in found["skipped"]:
        print(f"Skipped quiet run = frames [{pos}, {pos + lm}) = {pos * 0.02:.2f} s .. {(pos + lm) * 0.02:.2f} s: {why}")
    with open(os.path.join(save_dir, "gaps.json"), "w") as f:
        json.dump({"gaps": [list(g) for g in found["gaps"]], "skipped": [list(g) for g in found["skipped"]], **report, **clips16_keywords(cfg)}, f)
    return found["gaps"]


def dead_keywords(dead: Optional[dict], scale: float) -> dict:
    """`detect:`'s kind / rel_threshold / held_tol as find_gaps and conceal_file take them, for a file whose samples are `scale` times
    full-scale units (32768 for an int16 file, scanned as the int16 it holds): held_tol is scaled as the threshold is -- exact, a power
    of two -- and rel_threshold, a fraction of the file's own peak, is not."""
    dead = dead if dead is not None else {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}
    return {"kind": dead["kind"], "rel_threshold": dead["rel_threshold"], "held_tol": dead["held_tol"] * scale}


def level_keywords(cfg) -> dict:
    """`detect:`'s win_ms as find_gaps and conceal_file take it: given with `kind: level` alone, so that every other
    kind is called as it was.  win_ms is a time and, like rel_threshold, is not scaled for an int16 file."""
    dead, level = getattr(cfg, "detect_dead", None), getattr(cfg, "detect_level", None)
    if dead is None or dead["kind"] not in ("level", "burst", "impulse"):          # kinds burst and impulse (4.33) have level's window key
        return {}
    return {"win_ms": level["win_ms"] if level is not None else 2.0}


def impulse_keywords(cfg) -> dict:
    """`detect: {kind: impulse}`'s order / guard / pad / ratio as find_gaps and conceal_file take them: given at that kind
    alone, so that every other kind is called as it was.  None of them is scaled for a PCM file: the ratio test has no unit."""
    dead, imp = getattr(cfg, "detect_dead", None), getattr(cfg, "detect_impulse", None)
    if dead is None or dead["kind"] != "impulse" or imp is None:
        return {}
    return {"impulse_order": imp["order"], "impulse_guard": imp["guard"], "impulse_pad": imp["pad"], "impulse_ratio": imp["ratio"]}


def ceiling_keywords(cfg, scale: float) -> dict:
    """`detect: {kind: invalid}`'s ceiling as patch_file and patch_recording take it: the threshold in the units the
    file is read in, 0 or absent = +inf; given at that kind alone, so that every other run calls them as before."""
    dead = getattr(cfg, "detect_dead", None)
    if cfg.detect is None or dead is None or dead["kind"] != "invalid":
        return {}
    from . import gaps as G
    return {"ceiling": G.invalid_ceiling(cfg.detect["threshold"] * scale)}


def _dead_report(cfg: PredictConfig, found: dict, scale: float) -> dict:
    """What gaps.json gains when the detection went through find_dead_runs: `kind`, and `T`, the effective threshold in the units the
    file was scanned in (one per channel for `channels: each`).  Printed too.  Empty at the defaults: gaps.json is then what it was."""
    if "threshold" not in found:
        return {}
    T, unit = found["threshold"], {1.0: "full scale", 8388608.0: "24-bit steps"}.get(scale, "int16 steps")
    if cfg.detect_dead["kind"] == "invalid":                                       # the ceiling; null = none (non-finite samples only)
        many = isinstance(T, (list, tuple))
        c = T[0] if many else T
        print(f"Detection kind = invalid, ceiling = {'none' if c == float('inf') else c} ({unit})")
        return {"kind": "invalid", "ceiling": None if c == float("inf") else c, **({"unit": unit} if scale == 8388608.0 else {})}
    level = level_keywords(cfg)                                                    # kind level: the window is printed and recorded too
    window = f", window win_ms = {level['win_ms']}" if level else ""
    if cfg.detect_dead["kind"] == "impulse":                                       # the ratio test's settings are recorded as well
        imp = cfg.detect_impulse
        level = {**level, "ratio": imp["ratio"], "order": imp["order"], "guard": imp["guard"], "pad": imp["pad"]}
        window += f", ratio = {imp['ratio']}, order = {imp['order']}, guard = {imp['guard']}, pad = {imp['pad']}"
    print(f"Detection kind = {cfg.detect_dead['kind']}, effective threshold T = {T} ({unit}){window}")
    return {"kind": cfg.detect_dead["kind"], "T": T, **({"unit": unit} if scale == 8388608.0 else {}), **level}


def clips16_keywords(cfg) -> dict:
    """`long:`'s clips16 as patch_file and conceal_file take it: given off its default alone, so that every other run
    calls them, and writes gaps.json, as before."""
    clips16 = getattr(cfg, "long_clips16", "resampled")
    return {} if clips16 == "resampled" else {"clips16": clips16}


def mend_keywords(cfg) -> dict:
    """`detect:`'s mend_ms / mend_order / mend_context as conceal_file takes them: given when `mend_ms:` is above 0
    alone, so that every other run calls what it called and writes the gaps.json it wrote."""
    mend = getattr(cfg, "detect_mend", None)
    return {} if cfg.detect is None or not mend else {"mend_ms": mend["mend_ms"], "mend_order": mend["mend_order"], "mend_context": mend["mend_context"]}


def mended_report(rows) -> dict:
    """conceal_file's `mended` rows (start, len, status) as gaps.json records them: how many there are by status name."""
    from .native import MEND_STATUS
    count: Dict[str, int] = {}
    for _, _, st in rows:
        count[MEND_STATUS[st]] = count.get(MEND_STATUS[st], 0) + 1
    return count


def _main_long_file(cfg: PredictConfig, engine: InpaintingEngine, save_dir: str) -> int:
    """`long: {rate: file}`: the recording stays at the file's own rate and in its own sample type (engine.patch_file).  orig.wav,
    masked.wav and patched.wav are written at that rate; an int16 file is written as int16, any other as the float32 it was read to.
    With `feed: contexts` a multi-channel file (up to 8 channels) stays interleaved and is repaired channel by channel (DESIGN.md
    4.18): `mask:` / `masks:` apply to every channel, `detect: {channels: each | joint}` finds the gaps per channel or where all
    channels are quiet.  With the default `feed: recording` it is refused, as it was.
    `pcm24: keep`: a 24-bit PCM file goes to the engine as its packed bytes and the three files are written 24-bit;
    `detect:` thresholds are scaled by 2^23 and gaps.json names the unit "24-bit steps".  Any other file ignores the key."""
    from scipy.io import wavfile
    from . import gaps as G
    x24 = None
    if getattr(cfg, "long_pcm24", "float32") == "keep":
        packed, sr24, ch24 = audio.read_wav_pcm(cfg.wave_path)
        if packed.dtype == np.uint8 and packed.ndim == 3:                          # a 24-bit PCM file: (n, ch, 3) bytes
            if ch24 > 1:
                return _main_long_file_channels(cfg, engine, save_dir, sr24, packed)
            x24 = np.ascontiguousarray(packed[:, 0])
    sr_file, data = (sr24, x24) if x24 is not None else wavfile.read(cfg.wave_path)
    write = audio.write_wav_s24 if x24 is not None else audio.write_wav
    if x24 is None and data.ndim != 1:
        if cfg.long_feed != "contexts":                                            # the refusal of before, for the feed of before
            raise ValueError(f"{cfg.wave_path}: {data.shape[1]} channels -- `long: {{rate: file}}` with the default `feed: recording` resamples the "
                             f"whole file to feed the model and serves one channel; add `feed: contexts` to repair the channels in place, split "
                             f"the channels, or drop `rate: file` for the 22.05 kHz mix-down")
        return _main_long_file_channels(cfg, engine, save_dir, sr_file, data)
    raw = None
    if x24 is None:
        raw, sr_file = audio.read_wav(cfg.wave_path)
    x = data if x24 is not None or data.dtype == np.int16 else raw
    P, Q = G.rate_ratio(sr_file)
    fade_ms = cfg.patch_fade_ms if cfg.patch_fade_ms is not None else 5.0
    clip_frames, min_context = int(round(cfg.long["clip_s"] * 50)), int(round(cfg.long["context_s"] * 50))
    scale = 8388608.0 if x24 is not None else 32768.0 if x.dtype == np.int16 else 1.0   # the units patch_file reads x in: the ceiling's
    out = None
    if cfg.detect is not None and mend_keywords(cfg):                              # detection, mending and repair are conceal_file's
        d = cfg.detect
        out = engine.conceal_file(x, sr_file, d["threshold"] * scale, d["min_ms"], d["max_ms"], d["pad_frames"], fade_ms=fade_ms, clip_frames=clip_frames,
                                  min_context=min_context, batch=cfg.long["batch"], feed=cfg.long_feed, **dead_keywords(cfg.detect_dead, scale),
                                  **level_keywords(cfg), **impulse_keywords(cfg), **clips16_keywords(cfg), **mend_keywords(cfg))
        gap_list, report = out["gaps"], _dead_report(cfg, out, scale)
        for k, (pos, lm) in enumerate(gap_list):
            print(f"Detected gap {k} = frames [{pos}, {pos + lm}) = {pos * 0.02:.2f} s .. {(pos + lm) * 0.02:.2f} s")
        for pos, lm, why in out["skipped"]:
            print(f"Skipped quiet run = frames [{pos}, {pos + lm}) = {pos * 0.02:.2f} s .. {(pos + lm) * 0.02:.2f} s: {why}")
        print(f"Mended runs of at most {cfg.detect_mend['mend_ms']} ms, by status: {mended_report(out['mended'])}")
        with open(os.path.join(save_dir, "gaps.json"), "w") as f:
            json.dump({"gaps": [list(g) for g in gap_list], "skipped": [list(g) for g in out["skipped"]], **report, **clips16_keywords(cfg),
                       "mended": mended_report(out["mended"])}, f)
    elif cfg.detect is not None:
        gap_list = _detect_gaps(cfg, engine, raw, sr_file, -(-len(x) * P // Q), -(-G.file_fade(fade_ms, sr_file) * P // Q), clip_frames, min_context,
                                save_dir, x24)
    else:
        gap_list = sorted(cfg.gaps) if cfg.gaps is not None else [(cfg.mask_pos, cfg.mask_frames)]
    write(os.path.join(save_dir, "orig.wav"), x, sr_file)
    masked = x.copy()
    for s, l in G.file_spans(gap_list, sr_file):
        masked[s:s + l] = 0                                                        # the file samples whose time lies in the gap's frames
    write(os.path.join(save_dir, "masked.wav"), masked, sr_file)
    if out is None:
        out = engine.patch_file(x, sr_file, gap_list, fade_ms=fade_ms, clip_frames=clip_frames, min_context=min_context, batch=cfg.long["batch"],
                                feed=cfg.long_feed, **clips16_keywords(cfg), **ceiling_keywords(cfg, scale))
    if clips16_keywords(cfg):
        print(f"16 kHz clips: clips16 = {cfg.long_clips16} (cut straight from the file, with the 22.05 kHz clips)")
    labels, off = out["labels"].tolist(), out["label_off"]
    for k, (pos, lm) in enumerate(gap_list):
        print(f"Predicted codewords, gap {k} = frames [{pos}, {pos + lm}): ", labels[off[k]:off[k + 1]])
    write(os.path.join(save_dir, "patched.wav"), out["patched"].cpu().numpy(), sr_file)
    print("wrote", save_dir)
    return 0


def _wav_samples(data: np.ndarray) -> np.ndarray:
    """A WAV file's samples as patch_file takes them: int16 as it is, any other type as audio.read_wav's float32, channels kept."""
    if data.dtype == np.int16:
        return data
    if data.dtype == np.int32:
        return data.astype(np.float32) / 2147483648.0
    if data.dtype == np.uint8:
        return (data.astype(np.float32) - 128.0) / 128.0
    return data.astype(np.float32)


def _main_long_file_channels(cfg: PredictConfig, engine: InpaintingEngine, save_dir: str, sr_file: int, data: np.ndarray) -> int:
    """`long: {rate: file}` on a multi-channel file (n, ch): the three files are written multi-channel, at the file's rate and in its
    sample type; gaps.json holds one list per channel for `detect: {channels: each}`.  The file is uploaded once; with `detect:` the
    route is engine.conceal_file itself, otherwise engine.patch_file with the given gaps for every channel.  data uint8 (n, ch, 3): the
    packed bytes of a 24-bit file under `pcm24: keep`, kept as they are and written 24-bit."""
    from . import gaps as G
    ch = data.shape[1]
    s24 = data.dtype == np.uint8 and data.ndim == 3
    write = audio.write_wav_s24 if s24 else audio.write_wav
    if ch > G.MAX_CHANNELS:
        raise ValueError(f"{cfg.wave_path}: {ch} channels -- `long: {{rate: file}}` serves at most {G.MAX_CHANNELS}")
    x = np.ascontiguousarray(data if s24 else _wav_samples(data))
    fade_ms = cfg.patch_fade_ms if cfg.patch_fade_ms is not None else 5.0
    clip_frames, min_context = int(round(cfg.long["clip_s"] * 50)), int(round(cfg.long["context_s"] * 50))
    dev = torch.from_numpy(x).to(engine.device)                                    # the one upload: detection and repair read it
    kw = dict(fade_ms=fade_ms, clip_frames=clip_frames, min_context=min_context, batch=cfg.long["batch"], feed=cfg.long_feed, **clips16_keywords(cfg))
    if clips16_keywords(cfg):
        print(f"16 kHz clips: clips16 = {cfg.long_clips16} (cut straight from the file, with the 22.05 kHz clips)")
    if cfg.detect is not None:                                                     # conceal_file: its own budget for a gap, its own fade
        d = cfg.detect
        scale = 8388608.0 if s24 else 32768.0 if x.dtype == np.int16 else 1.0       # an int16 / 24-bit file is scanned as the integers it holds
        joint = cfg.detect_channels == "joint"
        out = engine.conceal_file(dev, sr_file, d["threshold"] * scale, d["min_ms"], d["max_ms"], d["pad_frames"], detect=cfg.detect_channels,
                                  **dead_keywords(cfg.detect_dead, scale), **level_keywords(cfg), **impulse_keywords(cfg), **mend_keywords(cfg), **kw)
        report = _dead_report(cfg, out, scale)
        if mend_keywords(cfg):                                                     # gaps.json gains the count by status
            report["mended"] = mended_report(out["mended"]) if joint else [mended_report(one) for one in out["mended"]]
            print(f"Mended runs of at most {cfg.detect_mend['mend_ms']} ms, by status: {report['mended']}")
        found = [(out["gaps"], out["skipped"])] if joint else list(zip(out["gaps"], out["skipped"]))
        for c, (gaps_c, skipped_c) in enumerate(found):
            who = "all channels" if joint else f"channel {c}"
            for k, (pos, lm) in enumerate(gaps_c):
                print(f"Detected gap {k} of {who} = frames [{pos}, {pos + lm}) = {pos * 0.02:.2f} s .. {(pos + lm) * 0.02:.2f} s")
            for pos, lm, why in skipped_c:
                print(f"Skipped quiet run of {who} = frames [{pos}, {pos + lm}) = {pos * 0.02:.2f} s .. {(pos + lm) * 0.02:.2f} s: {why}")
        lists = lambda v: [list(g) for g in v] if joint else [[list(g) for g in one] for one in v]
        with open(os.path.join(save_dir, "gaps.json"), "w") as f:
            json.dump({"gaps": lists(out["gaps"]), "skipped": lists(out["skipped"]), **report, **clips16_keywords(cfg)}, f)
        per = [out["gaps"]] * ch if joint else out["gaps"]
    else:
        per = [sorted(cfg.gaps) if cfg.gaps is not None else [(cfg.mask_pos, cfg.mask_frames)]] * ch
        out = engine.patch_file(dev, sr_file, channel_gaps=per, **kw)
    write(os.path.join(save_dir, "orig.wav"), x, sr_file)
    masked = x.copy()
    for c in range(ch):
        for s, l in G.file_spans(per[c], sr_file):
            masked[s:s + l, c] = 0                                                 # the file samples whose time lies in the gap's frames
    write(os.path.join(save_dir, "masked.wav"), masked, sr_file)
    labels, off, coff = out["labels"].tolist(), out["label_off"], out["channel_off"]
    for c in range(ch):
        for k, (pos, lm) in enumerate(sorted(per[c])):
            print(f"Predicted codewords, channel {c}, gap {k} = frames [{pos}, {pos + lm}): ", labels[off[coff[c] + k]:off[coff[c] + k + 1]])
    write(os.path.join(save_dir, "patched.wav"), out["patched"].cpu().numpy(), sr_file)
    print("wrote", save_dir)
    return 0


def _main_long(cfg: PredictConfig, engine: InpaintingEngine, save_dir: str) -> int:
    """The `long:` route of `main`: the file as a recording of any length, its gaps on its own time axis."""
    if cfg.long_rate == "file":
        return _main_long_file(cfg, engine, save_dir)
    raw, sr_file = audio.read_wav(cfg.wave_path)
    if ceiling_keywords(cfg, 1.0) and sr_file != 22050:                            # the resample below would smear the damage
        raise ValueError(f"{cfg.wave_path}: `detect: {{kind: invalid}}` on a {sr_file} Hz file needs `long: {{rate: file, feed: contexts}}` (the "
                         f"22.05 kHz route resamples the whole file, which spreads an invalid sample over every output within the filter's reach)")
    wave_22 = engine.resample(torch.from_numpy(raw)[None].to(engine.device), sr_file, 22050)[0].contiguous()
    fade = cfg.patch_fade if cfg.patch_fade is not None else 110
    clip_frames, min_context = int(round(cfg.long["clip_s"] * 50)), int(round(cfg.long["context_s"] * 50))
    if cfg.detect is not None:                                                     # optional `detect:` mapping: the gaps are found
        gap_list = _detect_gaps(cfg, engine, raw, sr_file, wave_22.numel(), fade, clip_frames, min_context, save_dir)
    else:
        gap_list = sorted(cfg.gaps) if cfg.gaps is not None else [(cfg.mask_pos, cfg.mask_frames)]
    audio.write_wav(os.path.join(save_dir, "orig.wav"), engine.to_int16(wave_22).cpu().numpy(), 22050)
    masked = wave_22.clone()
    for pos, lm in gap_list:
        masked[pos * 441:(pos + lm) * 441] = 0                                     # gaps.spans22: frame p = samples [441 p, 441 (p + 1))
    audio.write_wav(os.path.join(save_dir, "masked.wav"), engine.to_int16(masked).cpu().numpy(), 22050)
    out = engine.patch_recording(wave_22, gap_list, fade=fade, clip_frames=clip_frames, min_context=min_context, batch=cfg.long["batch"], pcm=True,
                                 **ceiling_keywords(cfg, 1.0))
    labels, off = out["labels"].tolist(), out["label_off"]
    for k, (pos, lm) in enumerate(gap_list):
        print(f"Predicted codewords, gap {k} = frames [{pos}, {pos + lm}): ", labels[off[k]:off[k + 1]])
    audio.write_wav(os.path.join(save_dir, "patched.wav"), out["patched_pcm"].cpu().numpy(), 22050)
    print("wrote", save_dir)
    return 0


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    cfg = load_predict_config(argv[0] if argv else "predict.yaml")
    device = choose_device(cfg.device_index)
    print("Current device:", device)
    engine = build_engine(cfg, device)
    wave_name = cfg.wave_path.split("/")[-1].split(".")[0]
    save_dir = os.path.join(cfg.save_pred, wave_name)
    os.makedirs(save_dir, exist_ok=True)
    if cfg.long is not None:                                                       # optional `long:` mapping: a recording of any length
        return _main_long(cfg, engine, save_dir)
    raw, sr_file = audio.read_wav(cfg.wave_path)                                   # predict.py:79-80 (librosa.load x 2): one read,
    raw_dev = torch.from_numpy(raw)[None].to(engine.device)                        # both rates on the GPU with librosa 0.9.1's own
    wave_22 = engine.resample(raw_dev, sr_file, 22050)                             # resampler (resampy kaiser_best); they STAY there
    wave_16 = engine.resample(raw_dev, sr_file, 16000)
    audio.write_wav(os.path.join(save_dir, "orig.wav"), wave_16[0].cpu().numpy(), 16000)
    # one `mask:` (the reference's schema) or a `masks:` list: the same steps per gap
    multi = cfg.gaps is not None
    gap_list = sorted(cfg.gaps) if multi else [(cfg.mask_pos, cfg.mask_frames)]
    masked_16 = wave_16[0].clone()
    for pos, lm in gap_list:
        masked_16[pos * 320 + 80:(pos + lm) * 320 + 79 - 80] = 0                   # predict.py:133
    audio.write_wav(os.path.join(save_dir, "masked.wav"), masked_16.cpu().numpy(), 16000)

    labels_path = os.path.join(cfg.path2centroids, wave_name + "_labels.pt")
    labels = None
    if os.path.exists(labels_path):                                                # predict.py:160-161
        all_labels = torch.load(labels_path, map_location="cpu").t().reshape(-1)
        labels = torch.cat([all_labels[pos:pos + lm] for pos, lm in gap_list]).long()
    patch = cfg.patch_fade is not None                                             # optional `patch:` mapping: also write patched.wav
    fade = cfg.patch_fade if patch else 110
    if multi:
        out = predict_resident(engine, wave_16, wave_22, gaps=[gap_list], mask22=[cfg.spans22], diagnostics=True, target_labels=labels,
                               patch=patch, fade=fade)
        out["labels"] = out["labels"][None]
    else:
        pos, lm = gap_list[0]
        span22 = (cfg.start_sample * 22050 // 16000, cfg.end_sample * 22050 // 16000)   # predict.py:99-100
        out = predict_resident(engine, wave_16, wave_22, [pos], lm, mask22=[span22], diagnostics=True,
                               target_labels=None if labels is None else labels[None], patch=patch, fade=fade)
        if patch:
            out["labels"] = out["labels"][None]
    pcm = lambda w: engine.to_int16(w[0]).cpu().numpy()                            # predict.py:204-206 on the GPU (si_pcm16)
    # hifi_masked.wav: the vocoder on the masked mel alone (predict.py:123-128)
    audio.write_wav(os.path.join(save_dir, "hifi_masked.wav"), pcm(out["hifi_masked"]), 22050)
    if labels is not None:                                                         # predict.py:171-189,198-201
        audio.write_wav(os.path.join(save_dir, "expected_inpaint.wav"), pcm(out["expected_inpaint"]), 22050)
        print("Loss:", float(out["loss"]))
        print("Average Cosine Similarity: ", float(out["cos_pred_target"].mean()))
        print("Target codewords: ", labels.tolist())
    print("Predicted codewords: ", out["labels"][0].tolist())
    audio.write_wav(os.path.join(save_dir, "inpainted.wav"), pcm(out["wave"]), 22050)
    if patch:                                                                      # the recording itself, only the gaps filled
        audio.write_wav(os.path.join(save_dir, "patched.wav"), pcm(out["patched"]), 22050)
    print("wrote", save_dir)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
