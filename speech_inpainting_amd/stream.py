"""Request front of the path: everything `I_ea/predict.py` does around the three replaced
subsystems for ONE file -- `librosa.load` at both rates (:79-80), masking + normalisation + log-mel (:99-106,132-141), the model
calls, `audio * 32768` + int16 (:204-206) -- as a pipelined batch service on the GPU:

    host clips (file rate, float32) --pinned H2D (its own stream)--> resample to 22.05 / 16 kHz (resampy kaiser_best, si_resample_sinc)
        -> masked log-mel (si_mel_frontend) -> encoder -> arg-max / splice -> vocoder -> int16 PCM (si_pcm16)
        --async D2H (its own stream)--> pinned host PCM

Batches are double-buffered over two copy streams: while batch i computes, batch i + 1's clips cross PCIe and batch i - 1's PCM comes back, so the
end-to-end rate is the compute rate as long as PCIe is the shorter leg (32 x 4 s: 11 MB in, 5.6 MB out per 12 ms step).
Clips of one batch may have different lengths: they then share every launch through the library's ragged-batch entry points.
PyTorch owns the streams, events and pinned buffers; all arithmetic is the HIP library's.  No CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Iterable, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import audio
from . import gaps as G
from .engine import InpaintingEngine


@dataclass
class Request:
    """One batch of clips at the FILE's sample rate (what `sf.read` / `librosa.load(sr=None)` yields: float32 in [-1, 1])."""
    clips: Sequence[np.ndarray]
    mask_pos: Sequence[int] = ()            # first masked 20 ms frame per clip (ignored when blind or when gaps are given)
    mask_frames: int = 10
    blind: bool = False
    tag: object = None
    gaps: Optional[Sequence[Sequence[Sequence[int]]]] = None   # per clip a list of (first frame, frame count): several gaps per clip,
                                                               # one pass (replaces mask_pos / mask_frames; not with blind)
    patch: bool = False                     # patch mode: Result.pcm is the clip's OWN 22.05 kHz samples with only the gaps filled
    fade: int = 110                         # (cross-fade of `fade` 22.05 kHz samples around each gap); not with blind


@dataclass
class Result:
    pcm: List[np.ndarray]                   # int16 at 22.05 kHz, one array per clip, cut to the clip's own length (the generator's
                                            # wave_len; with Request.patch the INPUT's 22.05 kHz length len22)
    labels: torch.Tensor                    # (B, Lm) predicted codewords (host); with gaps: flat (F,), clip b = [label_off[b], label_off[b + 1])
    tag: object = None
    label_off: Optional[List[int]] = None


@dataclass
class _Slot:
    pin_in: Optional[torch.Tensor] = None
    dev_in: Optional[torch.Tensor] = None
    pin_out: Optional[torch.Tensor] = None
    pin_lab: Optional[torch.Tensor] = None
    pin_tab: Optional[torch.Tensor] = None  # the gap tables of a Request with gaps (int32): pinned, and their device copy
    dev_tab: Optional[torch.Tensor] = None
    ev_h2d: torch.cuda.Event = field(default_factory=torch.cuda.Event)
    ev_done: torch.cuda.Event = field(default_factory=torch.cuda.Event)
    ev_d2h: torch.cuda.Event = field(default_factory=torch.cuda.Event)
    keep: tuple = ()                        # device tensors of the batch in flight (alive until its PCM is back)
    meta: Optional[dict] = None


class RequestFront:
    """Pipelined `predict` service over one engine.  `run(requests)` yields one Result per Request, in order."""

    def __init__(self, engine: InpaintingEngine, sr_in: int = 22050, depth: int = 2):
        self.engine, self.sr_in, self.depth = engine, int(sr_in), max(1, int(depth))
        self.dev = engine.device
        # two copy streams: batch i + 1's clips must not queue behind batch i's PCM, which waits for batch i's compute
        self.h2d = torch.cuda.Stream(self.dev)
        self.d2h = torch.cuda.Stream(self.dev)
        self.slots = [_Slot() for _ in range(self.depth)]

    # ---- sizes of librosa.load's outputs (librosa.resample: ceil(n * ratio) after fix_length): the resampler's own rule, so that
    # a clip is as long for the front as for engine.resample and for the unpipelined path
    def _len_at(self, n: int, sr: int) -> int:
        return audio.resampled_len(n, self.sr_in, sr)

    def _ensure(self, s: _Slot, B: int, n_in: int, n_out: int, lm: int, n_tab: int = 0):
        # flat, persistent buffers per slot.  The copy stream is not ordered with the compute stream's frees: a block the caching
        # allocator hands out here may be one that temporaries of the batch in flight gave back on the host while kernels still queued
        # on the compute stream read it.  So after an allocation -- and only then -- the copy stream waits ONCE for what the compute
        # stream holds at this moment, before the first copy into the new block.  From then on the block is the slot's own: a request
        # that grows nothing makes the copy stream wait for nothing, and batch i + 1's upload overlaps batch i's compute.
        grown = False
        if s.pin_in is None or s.pin_in.numel() < B * n_in:
            s.pin_in = torch.empty(B * n_in, dtype=torch.float32).pin_memory()
            s.dev_in = torch.empty(B * n_in, dtype=torch.float32, device=self.dev)
            grown = True
        if s.pin_out is None or s.pin_out.numel() < B * n_out:
            s.pin_out = torch.empty(B * n_out, dtype=torch.int16).pin_memory()
        if s.pin_lab is None or s.pin_lab.numel() < B * max(lm, 1):
            s.pin_lab = torch.empty(B * max(lm, 1), dtype=torch.int64).pin_memory()
        if n_tab and (s.pin_tab is None or s.pin_tab.numel() < n_tab):
            s.pin_tab = torch.empty(n_tab, dtype=torch.int32).pin_memory()
            s.dev_tab = torch.empty(n_tab, dtype=torch.int32, device=self.dev)
            grown = True
        if grown:
            self.h2d.wait_stream(torch.cuda.current_stream(self.dev))

    def _submit(self, s: _Slot, rq: Request):
        eng, dev = self.engine, self.dev
        B = len(rq.clips)
        lens = [len(c) for c in rq.clips]
        n_in = max(lens)
        ragged = min(lens) != n_in
        len22 = [self._len_at(n, 22050) for n in lens]
        len16 = [self._len_at(n, 16000) for n in lens]
        mel_len = [eng.ctx.mel_frames(n) for n in len22]
        frames = [eng.ctx.num_frames(n) for n in len16]
        if rq.gaps is not None and rq.blind:
            raise ValueError("Request: blind mode takes no gaps")
        if rq.patch and rq.blind:
            raise ValueError("Request: patch=True with blind=True: blind mode replaces every frame, there is nothing of the recording to keep")
        rq_gaps = rq.gaps
        if rq.patch and rq_gaps is None:                             # the single gap, as one gap per clip on the multi-gap route
            rq_gaps = [[(int(p), int(rq.mask_frames))] for p in rq.mask_pos]
        lm = max(min(t, m) for t, m in zip(frames, mel_len)) if rq.blind else int(rq.mask_frames)
        n_tab = 0
        gaps = None
        if rq_gaps is not None:
            # validated BEFORE any slot buffer is sized from them: a refused request (ValueError naming clip and gap) leaves the slot as it was
            if len(rq_gaps) != B:
                raise ValueError(f"Request: gaps for {len(rq_gaps)} clips, batch of {B}")
            gaps = G.normalize_gaps(rq_gaps, [min(t, m) for t, m in zip(frames, mel_len)])
            # label buffer: all masked frames of the batch, flat; table buffer: two span tables (off (B + 1), start, len, one spare
            # word each) and the frame table (clip, frame per masked frame)
            F = sum(l for clip in gaps for _, l in clip)
            lm = -(-F // B)
            S = sum(len(clip) for clip in gaps)
            n_tab = 2 * (B + 2 + 2 * S) + 2 * F
            if rq.patch:
                # the patch tables ride in the same buffer: at most one window per span -- PatchTable (3 W + S + B + fade + 1 words),
                # the gather's window table (3 W) and the clips' 22.05 kHz lengths (B)
                if int(rq.fade) < 0:
                    raise ValueError(f"Request: fade = {rq.fade} samples is negative")
                n_tab += 7 * S + 2 * B + int(rq.fade) + 1
        n_wave = max(len22) if rq.patch else eng.ctx.vocoder_samples(max(mel_len), True)
        self._ensure(s, B, n_in, n_wave, lm, n_tab)
        # host -> pinned (zero tail for shorter clips), pinned -> device on the copy stream
        # (numpy views of the pinned buffers: plain memcpy.  torch CPU ops here would each wake the intra-op thread pool, whose
        #  spinning workers burn the job's CPU quota until the cgroup is throttled -- measured: 70-280 ms stalls per request)
        pin = s.pin_in[:B * n_in].view(B, n_in)
        pin_np = pin.numpy()
        for i, c in enumerate(rq.clips):
            np.copyto(pin_np[i, :lens[i]], np.asarray(c, dtype=np.float32))
            if lens[i] < n_in:
                pin_np[i, lens[i]:] = 0.0
        compute = torch.cuda.current_stream(dev)
        raw = s.dev_in[:B * n_in].view(B, n_in)
        tables = None
        with torch.cuda.stream(self.h2d):
            raw.copy_(pin, non_blocking=True)
        if rq_gaps is not None:
            # the span tables (16 kHz and 22.05 kHz) and the frame table are validated and built on the host, into the slot's pinned
            # buffer, and cross on the copy stream behind the clips: no copy of this request waits on the compute stream
            # (patch mode: its window and patch tables too, in the same copy)
            tables = eng.gap_tables(gaps, len16, len22, staging=(s.pin_tab, s.dev_tab, self.h2d), patch_fade=int(rq.fade) if rq.patch else None)
        s.ev_h2d.record(self.h2d)
        compute.wait_event(s.ev_h2d)
        # librosa.load x 2 (I_ea/predict.py:79-80): the file's samples at 22.05 kHz and at 16 kHz
        w22 = raw if self.sr_in == 22050 else eng.resample(raw, self.sr_in, 22050, lens=lens if ragged else None)
        w16 = raw if self.sr_in == 16000 else eng.resample(raw, self.sr_in, 16000, lens=lens if ragged else None)
        if rq_gaps is not None:
            if rq.patch:
                # orig = the clip at 22.05 kHz (resampled when the file's rate is another); the int16 conversion is fused into the compose
                out = eng.patch_multigap_batch(w16, w22, gaps, fade=int(rq.fade), len16=len16 if ragged else None,
                                               len22=len22 if ragged else None, tables=tables, pcm=True)
                wave_len, pcm = len22, out["patched_pcm"]
            else:
                out = eng.predict_multigap_batch(w16, w22, gaps, len16=len16 if ragged else None, len22=len22 if ragged else None,
                                                 tables=tables)
                wave_len = out["wave_len"] if ragged else [out["wave"].shape[1]] * B
                pcm = eng.to_int16(out["wave"])
            self._finish(s, compute, pcm, out["labels"], (w22, w16, out, pcm), B=B, wave_len=wave_len, n_lab=out["labels"].numel(), tag=rq.tag,
                         label_off=out["label_off"], tables=tables)
            return
        pos = torch.tensor([int(p) for p in rq.mask_pos], dtype=torch.int32).to(dev, non_blocking=True)
        if rq.blind:
            s22 = e22 = None
        else:
            sp = [clip[0] for clip in G.spans22([[(int(p), lm)] for p in rq.mask_pos], len22)]
            s22 = torch.tensor([a for a, _ in sp], dtype=torch.int32).to(dev)
            e22 = torch.tensor([a + l for a, l in sp], dtype=torch.int32).to(dev)
        if ragged:
            mel = eng.mel_ragged(w22, len22, s22, e22)
            out = eng.predict_ragged_batch(w16, len16, mel, mel_len, pos, lm, blind=rq.blind)
            wave_len = out["wave_len"]
        else:
            mel = eng.mel(w22, s22, e22)
            out = eng.predict_batch(w16, mel, pos, lm, blind=rq.blind)
            wave_len = [out["wave"].shape[1]] * B
        pcm = eng.to_int16(out["wave"])                              # B6 on the device
        self._finish(s, compute, pcm, out["labels"], (w22, w16, mel, out, pcm, pos, s22, e22), B=B, wave_len=wave_len,
                     n_lab=out["labels"].shape[1], tag=rq.tag)

    def _finish(self, s: _Slot, compute, pcm: torch.Tensor, labels: torch.Tensor, keep: tuple, **meta):
        """The tail of a submitted batch: once the compute stream is done, PCM and labels (flat) go to the slot's pinned buffers on the
        device-to-host stream; `keep` (the batch's device tensors) stays alive until those copies have run."""
        s.ev_done.record(compute)
        self.d2h.wait_event(s.ev_done)
        with torch.cuda.stream(self.d2h):
            s.pin_out[:pcm.numel()].view(pcm.shape).copy_(pcm, non_blocking=True)
            s.pin_lab[:labels.numel()].copy_(labels.reshape(-1), non_blocking=True)
            s.ev_d2h.record(self.d2h)
        s.keep = keep
        s.meta = dict(n_wave=pcm.shape[1], **meta)

    def _collect(self, s: _Slot) -> Result:
        s.ev_d2h.synchronize()
        m = s.meta
        po = s.pin_out.numpy()[:m["B"] * m["n_wave"]].reshape(m["B"], m["n_wave"])
        pcm = [po[i, :m["wave_len"][i]].copy() for i in range(m["B"])]
        if m.get("label_off") is not None:
            lab = torch.from_numpy(s.pin_lab.numpy()[:m["n_lab"]].copy())
        else:
            lab = torch.from_numpy(s.pin_lab.numpy()[:m["B"] * m["n_lab"]].reshape(m["B"], m["n_lab"]).copy())
        s.keep, s.meta = (), None
        return Result(pcm, lab, m["tag"], m.get("label_off"))

    def _drain(self, streams: bool = False):
        """Every slot synchronised and empty: the copies of a batch still in flight have run, its device tensors are released and its
        result is dropped.  streams: also wait for the copy streams and the compute stream (a request that raised part-way)."""
        for s in self.slots:
            if s.meta is not None:
                s.ev_d2h.synchronize()
            s.keep, s.meta = (), None
        if streams:
            self.h2d.synchronize()
            torch.cuda.current_stream(self.dev).synchronize()
            self.d2h.synchronize()

    def run(self, requests: Iterable[Request]) -> Iterator[Result]:
        """One Result per Request, in order.  However the run ends -- exhausted, the generator closed or dropped early, a request
        refused by `_submit` (its exception leaves `run` unchanged) -- every slot ends synchronised with `meta = None` and `keep = ()`,
        and the same front serves the next `run`, which also starts from clean slots.  Results of batches in flight when a run ends
        early are DROPPED, not yielded: their copies are waited for and their buffers released."""
        self._drain()
        inflight: List[_Slot] = []
        done = False
        try:
            for i, rq in enumerate(requests):
                s = self.slots[i % self.depth]
                if s.meta is not None:                               # the slot's previous batch: its PCM must be out before reuse
                    inflight.remove(s)
                    yield self._collect(s)
                self._submit(s, rq)
                inflight.append(s)
            while inflight:
                yield self._collect(inflight.pop(0))
            done = True
        finally:
            self._drain(streams=not done)


def predict_stream(engine: InpaintingEngine, requests: Iterable[Request], sr_in: int = 22050, depth: int = 2) -> Iterator[Result]:
    """`predict` over a stream of batches with transfers overlapped (see RequestFront)."""
    return RequestFront(engine, sr_in, depth).run(requests)
