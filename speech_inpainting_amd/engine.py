"""Host-side mirror of the reference's module interface over the HIP library.

The reference's seam is Python duck-typing at three calls; the classes below keep those
names, argument meanings and shapes, and forward to libsi_hip.so:

    model(input_values (B, N), attention_mask)      -> (B, T, 80)        I_ea/model.py:80-89
    generator(feats (B, 80, T'))                     -> (B, 1, T' * 256)  I_ea/hifi_gan/models.py:107-123
    loss.cos_sim(values, labels)[1]                  -> predicted labels  I_ea/loss_fn.py:44-47

plus `InpaintingEngine.predict_batch`, the batched form of the script body I_ea/predict.py:130-207, which is what the
benchmark times.  Nothing here computes on the CPU: a missing library or a CPU device raises.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence, Tuple

import torch

from .arch import HubertArch, VocoderArch
from .checkpoint import flatten_checkpoint
from . import gaps as G
from . import native
from .native import NativeContext, PatchTable, RateTable, RegionTable, SpanTable, make_desc


def mask_samples_from_frames(frame_pos: int, frame_len: int):
    """Sample span zeroed for a frame-level mask: [pos*320+80, (pos+len)*320+79-80) (I_ea/predict.py:133)."""
    s = frame_pos * 320 + 80
    e = (frame_pos + frame_len) * 320 + 79 - 80
    return s, max(e - s, 0)


def ida_match_lengths(n_audio: int, n_code: int, n_f0: int, code_hop: int = 320, f0_hop: int = 80):
    """Length bookkeeping of I_da's `inpainting()` (I_da/scripts/inpainting.py:219-255): `match_length` over (audio, 1),
    (audio_mask, 1), (code, code_hop), (fo, f0_hop) -- whole units of lcm(hops) samples, the minimum count over the series
    (I_da/src/multiseries.py:33-52) -- then `audio % (16 * 80)` samples' worth removed from every tail (:243-255).  The script
    matches `code` but not `code_inpainting`, which is only tail-trimmed.  -> (audio samples, code frames, code_inpainting
    frames, f0 frames)."""
    import math
    unit = math.lcm(code_hop, f0_hop)
    n_unit = min(n_audio // unit, n_code // (unit // code_hop), n_f0 // (unit // f0_hop))
    a, c, ci, f = n_unit * unit, n_unit * (unit // code_hop), n_code, n_unit * (unit // f0_hop)
    to_remove = a % (16 * 80)
    if to_remove % code_hop:
        raise AssertionError(f"to_remove={to_remove} is not a multiple of code_hop_size={code_hop} (I_da/scripts/inpainting.py:245)")
    if to_remove:
        a, c, ci, f = a - to_remove, c - to_remove // code_hop, ci - to_remove // code_hop, f - to_remove // 80
    if min(c, ci, f) <= 0:
        raise ValueError(f"clip too short for I_da's length matching: audio {n_audio}, code {n_code}, f0 {n_f0} frames")
    return a, c, ci, f


class _Unset(float):
    """A keyword's default that can be told from the same number passed in: it compares and prints as the float."""


_WIN_MS = _Unset(2.0)                      # win_ms "not given": 2 ms at kinds level and burst as ever, 23 ms at kind impulse


class InpaintingEngine:
    """One model pair (HuBERT + head, codebook, HiFi-GAN generator) resident on one GPU."""

    def __init__(self, harch: HubertArch, varch: VocoderArch, num_clusters: int, device="cuda:0",
                 encoder_dtype: str = "fp32", vocoder_dtype: str = "fp32", vocoder_chunk: int = 0):
        self.harch, self.varch = harch, varch
        self.device = torch.device(device)
        self.encoder_dtype, self.vocoder_dtype = encoder_dtype, vocoder_dtype
        self.ctx = NativeContext(make_desc(harch, varch, num_clusters, encoder_dtype, vocoder_dtype, vocoder_chunk), self.device)
        self._resamplers = {}

    # ---- weights
    def load_state(self, hubert_sd: Mapping[str, torch.Tensor], gen_sd: Mapping[str, torch.Tensor], codebook: Optional[torch.Tensor] = None):
        """hubert_sd: a CustomModel state dict, or the encoder alone (a HuggingFace directory / an I_da feature reader has no
        `final_layers`).  codebook (K, codebook_dim) or None (I_da: the unit codebook lives in HuBERT feature space and is passed
        per call).  An engine without a trained head or without a codebook serves the encoder-only entry points
        (`extract_features`, `ida_inpaint_batch`) and the vocoder; the I_ea calls that need the missing part (`encode`,
        `predict_batch`, `splice`, `codebook_metrics`, ...) raise instead of computing on placeholders -- the reference's predict
        path always loads the CustomModel .pt with its head (I_ea/predict.py:149) and its k-means model (:66-70)."""
        from .checkpoint import fresh_final_layers, normalize_hubert_keys
        hubert_sd = normalize_hubert_keys(hubert_sd)
        self._has_head = "final_layers.1.weight" in hubert_sd
        if not self._has_head:
            hubert_sd.update(fresh_final_layers(self.harch))          # placeholder so that the packed layout is complete; never served
        self._has_codebook = codebook is not None
        if codebook is None:
            codebook = torch.zeros(self.ctx.desc.num_clusters, self.harch.codebook_dim)
        blob, index = flatten_checkpoint(hubert_sd, gen_sd, codebook)
        self.ctx.load_weights(blob, index)
        # what this checkpoint held travels WITH the blob, in the header's reserved word (the library writes 0 there and never reads
        # it): a rank that receives the bytes by broadcast learns it in weights_check(), without a collective of its own
        word = self._FLAGS_VALID | (self._FLAG_HEAD if self._has_head else 0) | (self._FLAG_CODEBOOK if self._has_codebook else 0)
        self.ctx.weights_tensor()[24:32].copy_(torch.tensor(list(word.to_bytes(8, "little")), dtype=torch.uint8))
        return self

    _FLAGS_VALID, _FLAG_HEAD, _FLAG_CODEBOOK = 1, 2, 4             # bits of the blob header's reserved word (bytes 24..31)

    def alloc_weights(self, has_head: bool = True, has_codebook: bool = True):
        """Receiving rank of the weight broadcast: the flags say what the SOURCE rank's checkpoint held.  They only stand until
        weights_check(), which replaces them by what the received blob itself records."""
        self.ctx.alloc_weights()
        self._has_head, self._has_codebook = bool(has_head), bool(has_codebook)
        return self

    def _need(self, head: bool = False, codebook: bool = False, what: str = "this call"):
        if head and not getattr(self, "_has_head", True):
            raise RuntimeError(f"{what} needs the trained `final_layers` head, but the loaded checkpoint held the encoder only "
                               "(load the CustomModel .pt, I_ea/predict.py:149)")
        if codebook and not getattr(self, "_has_codebook", True):
            raise RuntimeError(f"{what} needs the k-means codebook, but none was loaded (load_state(..., codebook=...))")

    def weights_tensor(self) -> torch.Tensor:
        return self.ctx.weights_tensor()

    def weights_check(self) -> None:
        """After the weight broadcast: the blob in this context carries the fingerprint of THIS context's layout (raises otherwise),
        and this engine serves what the source rank's checkpoint held -- no trained head or no codebook there means `_need` raises
        here too, instead of serving the placeholder head or the zero codebook."""
        self.ctx.weights_check()
        word = int.from_bytes(bytes(self.ctx.weights_tensor()[24:32].cpu().tolist()), "little")
        if word & self._FLAGS_VALID:
            self._has_head, self._has_codebook = bool(word & self._FLAG_HEAD), bool(word & self._FLAG_CODEBOOK)

    # ---- the three stages
    def encode(self, wave16: torch.Tensor, mask_start: Optional[torch.Tensor] = None, mask_len: Optional[torch.Tensor] = None,
               normalize: bool = True, valid_len: Optional[torch.Tensor] = None, spans: Optional[SpanTable] = None) -> torch.Tensor:
        """valid_len (B,) int32: real samples per clip of a RIGHT-PADDED batch (the reference's attention_mask.sum(-1)).
        spans: a SpanTable of 16 kHz sample spans -- several zeroed spans per clip -- instead of mask_start / mask_len."""
        self._need(head=True, what="encode")
        if spans is not None:
            if mask_start is not None or mask_len is not None or valid_len is not None:
                raise ValueError("encode: `spans` replaces mask_start / mask_len and is not combined with valid_len")
            return self.ctx.hubert_forward_spans(wave16, spans, normalize)
        return self.ctx.hubert_forward(wave16, mask_start, mask_len, normalize, valid_len)

    def extract_features(self, wave16: torch.Tensor, output_layer: int, normalize="layer_norm",
                         mask_start: Optional[torch.Tensor] = None, mask_len: Optional[torch.Tensor] = None,
                         pre_mask_add: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`HubertFeatureReader.get_feats` for a batch (I_da/src/hubert_feature_reader.py:44-67): (B, N) raw clips ->
        (B, T, H) hidden state after `output_layer` transformer layers; see NativeContext.hubert_extract_features."""
        return self.ctx.hubert_extract_features(wave16, output_layer, normalize, mask_start, mask_len, pre_mask_add)

    def ida_inpaint_batch(self, wave16: torch.Tensor, frame_start, mask_size: int, centroids: torch.Tensor,
                          generator: "CodeGenerator", f0: torch.Tensor, emb: Optional[torch.Tensor] = None,
                          output_layer: int = 6, normalize: bool = True, code_hop_size: int = 320, f0_hop: int = 80) -> Dict[str, torch.Tensor]:
        """`inpainting()` of I_da/scripts/inpainting.py:151-266 for a batch of equal-length clips, on this GPU end to end:
        corruption `(y + 1e-6) * mask` (:186-192) fused into the encoder's first conv, HuBERT features of the clean and the
        corrupted clips at `output_layer` (:195-198; ONE encoder pass over 2B clips), k-means units (:204-205, GPU instead of
        sklearn on the host), unit splice (:209-214), the script's length bookkeeping (:219-255), and `generate` for both unit
        series (:258-259; one CodeGenerator pass over 2B series).
        wave16 (B, N) fp32 at 16 kHz; frame_start int or (B,) int tensor (samples; the script uses 1.5 s, :188); mask_size
        samples; centroids (K, H) the k-means model's `cluster_centers_`; generator a `CodeGenerator` over this engine (with
        its `F0Quantizer`); f0 (B, 1, Tf0) the normalised F0 track (YAAPT + normalize_nonzero, :216-217, is third-party CPU code
        outside the path); emb (B, E) speaker embedding or None.
        -> dict(code (B, F), code_inpainting (B, F'), audio_gen (B, F * hop), audio_inp (B, F' * hop), feats (2B, T, H))."""
        dev = self.device
        B, N = wave16.shape
        fs = torch.as_tensor(frame_start, dtype=torch.int32, device=dev).reshape(-1).expand(B).contiguous()
        zi = torch.zeros(B, dtype=torch.int32, device=dev)
        ms = torch.cat([zi, fs])
        ml = torch.cat([zi, torch.full((B,), int(mask_size), dtype=torch.int32, device=dev)])
        add = torch.cat([torch.zeros(B, dtype=torch.float64, device=dev), torch.full((B,), 1e-6, dtype=torch.float64, device=dev)])
        if generator.f0_quantizer is None:
            raise ValueError("ida_inpaint_batch: the CodeGenerator needs its F0Quantizer (the fixed F0 VQ-VAE, I_da/src/model.py:160-166)")
        # The F0 VQ-VAE's conv encoder (one workgroup per track: 16 of the chip's 256 CUs for ~0.35 ms) depends on nothing the HuBERT
        # encoder computes: it runs on a side stream UNDER the encoder and is joined before its bottleneck's arg-min.
        _, nc, nci, nf = ida_match_lengths(N, self.ctx.num_frames(N), f0.shape[-1], code_hop_size, f0_hop)
        f0 = f0.to(dev, torch.float32)[..., :nf].contiguous()
        main = torch.cuda.current_stream(dev)
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(dev)
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            f0_feats = generator.f0_quantizer.features(f0)
        both = torch.cat([wave16, wave16]).contiguous()
        hid = self.extract_features(both, output_layer, "layer_norm" if normalize else None, ms, ml, add)       # (2B, T, H)
        T, H = hid.shape[1], hid.shape[2]
        units = self.ctx.kmeans_assign(hid.reshape(2 * B * T, H), centroids.to(dev, torch.float32).contiguous()).reshape(2 * B, T)
        code = units[:B].contiguous()
        first = torch.div(fs, code_hop_size, rounding_mode="floor").to(torch.int32)
        last = torch.div(fs + int(mask_size), code_hop_size, rounding_mode="floor").to(torch.int32)
        code_inp = self.ctx.code_splice(code, units[B:].contiguous(), first, last)
        main.wait_stream(self._side)
        f0_feats.record_stream(main)
        z_p = generator.f0_quantizer.codes(f0_feats)                                   # the same F0 track conditions both outputs
        code, code_inp = code[:, :nc].contiguous(), code_inp[:, :nci].contiguous()
        if nc == nci:
            wav = generator(code=torch.cat([code, code_inp]), f0_code=torch.cat([z_p, z_p]),
                            emb=None if emb is None else torch.cat([emb, emb]))[:, 0]
            gen, inp = wav[:B], wav[B:]
        else:                                   # the script trims `code` but not `code_inpainting` (:219-227): two shapes
            gen = generator(code=code, f0_code=z_p, emb=emb)[:, 0]
            inp = generator(code=code_inp, f0_code=z_p, emb=emb)[:, 0]
        return {"code": code, "code_inpainting": code_inp, "audio_gen": gen, "audio_inp": inp, "feats": hid}

    def splice(self, feats: torch.Tensor, frame_pos: torch.Tensor, lm: int, mel: torch.Tensor) -> torch.Tensor:
        self._need(codebook=True, what="splice")
        return self.ctx.codebook_splice(feats, frame_pos, lm, mel)

    def splice_labels(self, labels: torch.Tensor, frame_pos: torch.Tensor, mel: torch.Tensor) -> None:
        """`expected_inpaint`'s splice (I_ea/predict.py:177-189): the raw centroids of GIVEN labels (B, Lm) into mel, in place."""
        self._need(codebook=True, what="splice_labels")
        self.ctx.codebook_splice_labels(labels, frame_pos, mel)

    # ---- several gaps per clip: the three codebook calls over a frame table (gaps.frame_table: clip index and frame, int32 (F) each)
    def splice_spans(self, feats: torch.Tensor, frame_clip: torch.Tensor, frame_pos: torch.Tensor, mel: torch.Tensor) -> torch.Tensor:
        """`splice` at the frames of a frame table, `mel` in place -> labels (F,) int64 in table order."""
        self._need(codebook=True, what="splice_spans")
        return self.ctx.codebook_splice_spans(feats, frame_clip, frame_pos, mel)

    def splice_labels_spans(self, labels: torch.Tensor, frame_clip: torch.Tensor, frame_pos: torch.Tensor, mel: torch.Tensor) -> None:
        """`splice_labels` at the frames of a frame table: the raw centroids of GIVEN labels (F,) into mel, in place."""
        self._need(codebook=True, what="splice_labels_spans")
        self.ctx.codebook_splice_labels_spans(labels, frame_clip, frame_pos, mel)

    def codebook_metrics_spans(self, feats: torch.Tensor, frame_clip: torch.Tensor, frame_pos: torch.Tensor, target: torch.Tensor):
        """`codebook_metrics` at the frames of a frame table, target (F,) int64; every per-frame output is flat (F,)."""
        self._need(codebook=True, what="codebook_metrics_spans")
        loss, terms, pred, cpt = self.ctx.codebook_metrics_spans(feats, frame_clip, frame_pos, target)
        return {"loss": loss[0], "loss_terms": terms, "pred_labels": pred, "cos_pred_target": cpt,
                "accuracy": (pred == target).float().mean()}

    def vocode(self, mel: torch.Tensor, stretch: bool = True) -> torch.Tensor:
        return self.ctx.hifigan_forward(mel, stretch)

    # ---- the script's three generator passes (I_ea/predict.py:123-128,196-207) differ only around the mask
    def receptive_radius(self) -> int:
        """Output samples (one side) an input frame of the generator can reach, from the architecture: conv_pre (k 7) 3 frames,
        per stage the transposed conv (ceil(k / u) + 1 input rows) and the widest ResBlock (sum over its dilations of (k - 1) / 2 *
        (d + 1) rows for ResBlock1, (k - 1) / 2 * d for ResBlock2), conv_post 3 samples; conservative (whole rows)."""
        v = self.varch
        hop = 1
        for u in v.upsample_rates:
            hop *= u
        r, per_row = 3 * hop, hop                                    # conv_pre at the frame rate
        two = str(v.resblock) == "1"
        for u, k in zip(v.upsample_rates, v.upsample_kernel_sizes):
            r += (-(-k // u) + 1) * per_row                           # the transposed conv, in rows of its input
            per_row //= u
            r += max(sum((rk - 1) // 2 * (d + (1 if two else 0)) for d in dil) for rk, dil in zip(v.resblock_kernel_sizes, v.resblock_dilation_sizes)) * per_row
        return r + 3

    def vocode_window(self, wave_base: torch.Tensor, mel_var: torch.Tensor, frame_pos: Sequence[int], lm: int) -> torch.Tensor:
        """The waveform of `mel_var` (B, 80, Tm), which differs from the mel that produced `wave_base` ONLY in frames
        [frame_pos[b], frame_pos[b] + lm): the generator runs on a window of the stretched frames around the change (as a ragged
        batch: a window clamped at a clip edge keeps that edge's real zero padding) and the samples the change can reach are spliced
        into a copy of `wave_base`.  Every output sample of the generator is the same fixed-order sum wherever its tile falls, so
        the result is BIT-IDENTICAL to a full pass (asserted per vocoder mode in tests/test_gpu_configs.py).
        This is `vocode_windows` with one range per clip: gaps.plan_windows on one range and gaps.kept_region give the window and
        the kept samples."""
        return self.vocode_windows(wave_base, mel_var, [[(int(p), int(lm))] for p in frame_pos])

    def _stretch(self, mel: torch.Tensor, hop: int, mel_len: Optional[Sequence[int]] = None, windowed: Sequence = ()) -> Tuple[torch.Tensor, list]:
        """The x441/256 stretched mel (B, D, Tout) the windows are cut from, and each clip's own stretched frames.  mel_len: per-clip
        mel frames of a ragged batch -- the stretch of a shorter clip clamps at ITS last frame, so the rows of a shorter clip that
        has windows (windowed[b] non-empty) come from the clip stretched alone."""
        ext = self.ctx.extend_mel(mel.contiguous())
        B, _, Tout = ext.shape
        if mel_len is None:
            return ext, [Tout] * B
        touts = [self.ctx.vocoder_samples(int(m), True) // hop for m in mel_len]
        for b in range(B):
            if touts[b] < Tout and windowed[b]:
                ext[b, :, :touts[b]] = self.ctx.extend_mel(mel[b:b + 1, :, :int(mel_len[b])].contiguous())[0]
        return ext, touts

    def _vocode_gathered(self, ext: torch.Tensor, wins, tab=None) -> torch.Tensor:
        """The windows `wins` = (clip, w0, w1) of the stretched mel -> their waveforms, one row per window: one gather launch and one
        ragged stretch=False generator pass over all of them.  tab: the window table where the caller staged it (gather_windows)."""
        return self.vocode_ragged(self.ctx.gather_windows(ext, wins, tab=tab), [w1 - w0 for _, w0, w1 in wins], stretch=False)

    def vocode_windows(self, wave_base: torch.Tensor, mel_var: torch.Tensor, ranges: Sequence[Sequence[Sequence[int]]],
                       mel_len: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The waveform of `mel_var`, which differs from the mel that produced `wave_base` only in the frame ranges `ranges[b]` =
        (pos, len) pairs of clip b (none, one or several, any lengths).  gaps.plan_windows merges a clip's
        windows where they overlap or touch; ALL windows of ALL clips go through the generator as one ragged stretch=False batch,
        and each window's kept region (its output without the rf frames at an edge that is not a clip edge) is spliced into a
        copy of `wave_base` -- the single-window rule, so the result is bit-identical to a full pass as well.
        mel_len: per-clip mel frames of a ragged batch (the stretch and the windows stop at the clip's own end)."""
        B, hop = mel_var.shape[0], self.ctx.vocoder_samples(1, False)
        Rf = -(-self.receptive_radius() // hop)
        ext, touts = self._stretch(mel_var, hop, mel_len, ranges)
        wins = [(b, w0, w1) for b in range(B) for w0, w1 in G.plan_windows(ranges[b], touts[b], Rf)]
        wave = wave_base.clone()
        if not wins:
            return wave
        out = self._vocode_gathered(ext, wins)
        for i, (b, w0, w1) in enumerate(wins):
            k0, k1 = G.kept_region(w0, w1, touts[b], Rf)
            wave[b, k0 * hop:k1 * hop] = out[i, (k0 - w0) * hop:(k1 - w0) * hop]
        return wave

    def mel(self, wave22: torch.Tensor, mask_start: Optional[torch.Tensor] = None, mask_end: Optional[torch.Tensor] = None,
            normalize: bool = True, spans: Optional[SpanTable] = None) -> torch.Tensor:
        """Vocoder-side front-end (I_ea/predict.py:99-106): zero [mask_start, mask_end) of each raw 22.05 kHz clip,
        peak-normalise * 0.95, log-mel -> (B, 80, Tm).  spans: a SpanTable of 22.05 kHz sample spans instead of the one span."""
        if spans is not None:
            if mask_start is not None or mask_end is not None:
                raise ValueError("mel: `spans` replaces mask_start / mask_end")
            return self.ctx.mel_frontend_spans(wave22, spans, normalize)
        return self.ctx.mel_frontend(wave22, mask_start, mask_end, normalize)

    def resample(self, x: torch.Tensor, sr_in: int, sr_out: int, kind: str = "kaiser_best", lens=None) -> torch.Tensor:
        """(B, n) fp32 clips at sr_in -> (B, audio.resampled_len(n, sr_in, sr_out)) at sr_out on the GPU: the resampling of
        `librosa.load(..., sr=...)` (I_ea/predict.py:79-80).  kind="kaiser_best" (default): resampy's band-limited interpolation, what librosa 0.9.1 runs --
        pinned bit for bit by the reference-held LJ001-0001 22k / 16k pair (si_resample_sinc).  kind="poly": the polyphase Kaiser
        FIR with scipy.signal.resample_poly's arithmetic (si_resample_poly; a different filter).  lens: per-clip sample counts of a
        ragged batch (kaiser_best only): clip b's output is zero past int(lens[b] * ratio)."""
        from . import audio
        if sr_in == sr_out:
            return x.clone()
        if kind == "kaiser_best":
            # one entry per rate pair, whatever lengths pass through: win / dwin once, and ONE time-register table
            # as long as the longest output seen -- time_reg[t] does not depend on the clip's length (repeated addition from 0), and
            # the kernel reads it for t < n_out only, so a longer table serves every shorter clip with the same bits
            f = self._sinc_tables(sr_in, sr_out)
            n_out = audio.resampled_len(int(x.shape[1]), sr_in, sr_out)
            if f["time_reg"] is None or f["time_reg"].numel() < n_out:
                f["time_reg"] = torch.from_numpy(audio.time_registers(sr_in, sr_out, n_out)).to(self.device)
            n_len = None if lens is None else torch.as_tensor(list(lens), dtype=torch.int32).to(self.device)
            return self.ctx.resample_sinc(x.contiguous(), f, n_out, n_len)
        if kind != "poly":
            raise ValueError(f"resample kind {kind!r}: 'kaiser_best' or 'poly'")
        if lens is not None:
            raise ValueError("ragged batches are resampled with kind='kaiser_best'")
        key = (kind, int(sr_in), int(sr_out), int(x.shape[1]))
        if key not in self._resamplers:
            taps, up, down, pre, n_out = audio.design_resampler(sr_in, sr_out, x.shape[1])
            self._resamplers[key] = (torch.from_numpy(taps).to(self.device), up, down, pre, n_out)
        taps, up, down, pre, n_out = self._resamplers[key]
        return self.ctx.resample_poly(x.contiguous(), taps, up, down, pre, n_out)

    def _sinc_tables(self, sr_in: int, sr_out: int) -> Dict[str, object]:
        """audio.design_kaiser_best(sr_in, sr_out, .) once per rate pair: win / dwin on the device and the scalars; time_reg (None until
        resample needs it) grows to the longest output seen.  resample, _rate_filter and _feed_filter share these device tables."""
        from . import audio
        key = ("kaiser_best", int(sr_in), int(sr_out))
        if key not in self._resamplers:
            f = audio.design_kaiser_best(int(sr_in), int(sr_out), 1)
            f.pop("n_out")
            f["time_reg"] = None
            f["reach"] = G.rate_reach(f["win"].size, f["step"])                      # taps per wing
            for k in ("win", "dwin"):
                f[k] = torch.from_numpy(f[k]).to(self.device)
            self._resamplers[key] = f
        return self._resamplers[key]

    def to_int16(self, wave: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """B6 on the GPU (I_ea/predict.py:204-206): fp32 waveform -> int16 PCM, `* 32768` truncated toward zero (si_pcm16)."""
        return self.ctx.pcm16(wave.contiguous(), out)

    def get_mel(self, x: torch.Tensor) -> torch.Tensor:
        """`get_mel(x)` of I_ea/dataset/mel_dump.py:96-98: x (B, n) already normalised -> (B, 80, Tm) log-mel."""
        return self.ctx.mel_frontend(x, None, None, normalize=False)

    def codebook_metrics(self, feats: torch.Tensor, frame_pos: torch.Tensor, lm: int, target: torch.Tensor):
        """Loss half of the reference's cos_sim on the masked frames of `feats` (B, T, 80) against target labels
        (B, Lm): -> dict(loss, loss_terms, pred_labels, cos_pred_target, accuracy)."""
        self._need(codebook=True, what="codebook_metrics")
        loss, terms, pred, cpt = self.ctx.codebook_metrics(feats, frame_pos, lm, target)
        return {"loss": loss[0], "loss_terms": terms, "pred_labels": pred, "cos_pred_target": cpt,
                "accuracy": (pred == target).float().mean()}

    # ---- ragged batches (BASELINE configs[4]): clips of different lengths in ONE set of launches
    def encode_ragged(self, wave16: torch.Tensor, len16, mask_start: Optional[torch.Tensor] = None,
                      mask_len: Optional[torch.Tensor] = None, normalize: bool = True, spans: Optional[SpanTable] = None) -> torch.Tensor:
        """wave16 (B, Nmax): clip b = the first len16[b] samples of its row -> (B, Tmax, 80); each clip's frames equal that clip
        encoded alone (the reference handles one file per run, I_ea/predict.py:76-207); rows past a clip's frames are zero."""
        self._need(head=True, what="encode_ragged")
        if spans is not None:
            if mask_start is not None or mask_len is not None:
                raise ValueError("encode_ragged: `spans` replaces mask_start / mask_len")
            return self.ctx.hubert_forward_spans(wave16, spans, normalize, sample_len=len16)
        return self.ctx.hubert_forward_varlen(wave16, len16, mask_start, mask_len, normalize)

    def mel_ragged(self, wave22: torch.Tensor, len22, mask_start: Optional[torch.Tensor] = None,
                   mask_end: Optional[torch.Tensor] = None, normalize: bool = True, spans: Optional[SpanTable] = None) -> torch.Tensor:
        """`mel` for clips of different lengths: (B, N22max) + per-clip sample counts -> (B, 80, Tm_max), zero frames past a clip's own."""
        if spans is not None:
            if mask_start is not None or mask_end is not None:
                raise ValueError("mel_ragged: `spans` replaces mask_start / mask_end")
            return self.ctx.mel_frontend_spans(wave22, spans, normalize, sample_len=len22)
        return self.ctx.mel_frontend_varlen(wave22, len22, mask_start, mask_end, normalize)

    def vocode_ragged(self, mel: torch.Tensor, mel_len, stretch: bool = True) -> torch.Tensor:
        return self.ctx.hifigan_forward_varlen(mel, mel_len, stretch)

    def predict_ragged_batch(self, wave16: torch.Tensor, len16, mel: torch.Tensor, mel_len, frame_pos: torch.Tensor, frame_len: int,
                             blind: bool = False, mask_start: Optional[torch.Tensor] = None,
                             mask_len: Optional[torch.Tensor] = None) -> Dict[str, object]:
        """`predict_batch` for clips of DIFFERENT lengths sharing every launch: wave16 (B, Nmax) / mel (B, 80, Tm_max) hold clip b in
        the first len16[b] samples / mel_len[b] frames of its row (host int sequences).  Every clip's outputs equal that clip's
        alone.  -> feats (B, Tmax, 80), labels (B, Lm) (-1 past a clip's own count in blind mode), mel, wave (B, Lmax; zero past a
        clip's own samples), wave_len / frames / mel_len: per-clip valid extents (lists)."""
        self._need(head=True, codebook=True, what="predict_ragged_batch")
        B = wave16.shape[0]
        len16 = [int(n) for n in len16]
        mel_len = [int(n) for n in mel_len]
        frames = [self.ctx.num_frames(n) for n in len16]
        if blind:
            feats = self.encode_ragged(wave16, len16)
            pos = torch.zeros(B, dtype=torch.int32, device=self.device)
            cnt_h = [min(t, m) for t, m in zip(frames, mel_len)]                   # predict_batch's `min(T, Tm)`, per clip
        else:
            if mask_start is None:
                mask_start = frame_pos * 320 + 80                                   # predict.py:133
                mask_len = torch.full_like(frame_pos, max(frame_len * 320 - 81, 0))
            feats = self.encode_ragged(wave16, len16, mask_start.to(torch.int32), mask_len.to(torch.int32))
            pos, cnt_h = frame_pos, [int(frame_len)] * B
        lm = max(cnt_h)
        cnt = torch.tensor(cnt_h, dtype=torch.int32, device=self.device)
        mel2 = mel.clone()
        labels = self.ctx.codebook_splice_varlen(feats, pos, cnt, lm, mel2)
        wav = self.vocode_ragged(mel2, mel_len, stretch=True)
        return {"feats": feats, "labels": labels, "mel": mel2, "wave": wav, "frames": frames, "mel_len": mel_len, "label_cnt": cnt_h,
                "wave_len": [self.ctx.vocoder_samples(m, True) for m in mel_len]}

    # ---- several gaps per clip, one pass
    def gap_tables(self, gaps, n16: Sequence[int], n_mel: Sequence[int], mel_frames: bool = False, spans22=None, staging=None,
                   patch_fade: Optional[int] = None) -> Dict[str, object]:
        """Validate `gaps` (per clip a list of (first frame, frame count)) against each clip's min(T, Tm) and build what one multi-gap
        pass needs: gaps (sorted), tab16 (SpanTable of the 16 kHz spans), tab22 (SpanTable of the 22.05 kHz spans: the gaps' by
        I_ea/predict.py:99-100, or `spans22[b]` = [start, end) sample pairs; None when n_mel counts mel frames), frame_clip /
        frame_pos (device int32 (F)), label_off (B + 1, host list).
        n16: 16 kHz samples per clip; n_mel: 22.05 kHz samples per clip, or mel frames when mel_frames=True.
        staging = (pinned int32 tensor, device int32 tensor, stream): all tables are written into the pinned buffer and cross in ONE
        asynchronous copy on `stream` (the request front's host-to-device stream); the caller orders that stream before the compute
        stream and keeps both buffers untouched until the pass is done.  Default: pageable copies on the current stream.
        patch_fade (22.05 kHz samples; raw clips only): also plan patch mode (`plan_patch`) -- entry "patch"; with `staging` its
        tables ride in the same buffer and the same copy."""
        if patch_fade is not None and mel_frames:
            raise ValueError("gap_tables: patch mode needs the 22.05 kHz samples, not a mel")
        if not (len(gaps) == len(n16) == len(n_mel)):
            raise ValueError(f"gaps for {len(gaps)} clips, batch of {len(n16)}")
        lim = [min(self.ctx.num_frames(int(a)), int(m) if mel_frames else self.ctx.mel_frames(int(m))) for a, m in zip(n16, n_mel)]
        g = G.normalize_gaps(gaps, lim)
        ci, fp, off = G.frame_table(g)
        s16 = G.spans16(g)
        s22 = None if mel_frames else (G.spans22(g, n_mel) if spans22 is None else G.clamp_spans22(spans22, n_mel))
        F = len(ci)
        plan = None if patch_fade is None else self.plan_patch(s22, n_mel, patch_fade)
        if staging is None:
            tab = torch.tensor([ci, fp], dtype=torch.int32).to(self.device)
            tb = {"gaps": g, "tab16": SpanTable(s16, self.device), "tab22": None if s22 is None else SpanTable(s22, self.device),
                  "frame_clip": tab[0].contiguous(), "frame_pos": tab[1].contiguous(), "label_off": off}
            if plan is not None:
                tb["patch"] = self._patch_tables(plan)
            return tb
        pin, dbuf, stream = staging
        w16, w22 = SpanTable.words(s16), 0 if s22 is None else SpanTable.words(s22)
        wp = 0 if plan is None else self.patch_words(plan)
        total = w16 + w22 + 2 * F + wp
        if total > min(pin.numel(), dbuf.numel()):
            raise ValueError(f"gap_tables: the staging buffers hold {min(pin.numel(), dbuf.numel())} words, the tables need {total}")
        hp = pin.numpy()
        tab16 = SpanTable(s16, self.device, staged=(hp[:w16], dbuf[:w16]))
        tab22 = None if s22 is None else SpanTable(s22, self.device, staged=(hp[w16:w16 + w22], dbuf[w16:w16 + w22]))
        o = w16 + w22
        hp[o:o + F] = ci
        hp[o + F:o + 2 * F] = fp
        if plan is not None:
            self._patch_tables(plan, staged=(hp[o + 2 * F:total], dbuf[o + 2 * F:total]))
        with torch.cuda.stream(stream):
            dbuf[:total].copy_(pin[:total], non_blocking=True)
        tb = {"gaps": g, "tab16": tab16, "tab22": tab22, "frame_clip": dbuf[o:o + F], "frame_pos": dbuf[o + F:o + 2 * F], "label_off": off}
        if plan is not None:
            tb["patch"] = plan
        return tb

    # ---- patch mode: the generated audio of the gaps spliced into the caller's own 22.05 kHz samples
    def plan_patch(self, spans22: Sequence[Sequence[Sequence[int]]], n22: Sequence[int], fade: int, regions=None) -> Dict[str, object]:
        """Host planning of one patched batch: per clip the blend regions of its 22.05 kHz spans (start, len) and the generator
        windows that hold them (gaps.blend_regions / gaps.plan_patch_windows with this generator's hop and receptive radius).
        -> fade, hop, wins = (clip, w0, w1) of all windows, windows (per clip), span_win (flat, the span table's order), lim and
        n22 (per clip).  regions (per clip, per span a [a, b) sample range or None): the samples each span's window must KEEP, in
        place of its blend region -- patch_file's regions widened by the interpolation's reach (gaps.reach_regions22)."""
        hop = self.ctx.vocoder_samples(1, False)
        if hop != 256:
            # extend_mel centres stretched frame t at input sample (t + 0.5) * 256: generator sample n is input sample n only at hop 256
            raise ValueError(f"patch mode needs a generator of hop 256 (the x441/256 stretch's identity time map), this one has hop {hop}")
        rf = -(-self.receptive_radius() // hop)
        wins, span_win, lim, per_clip = [], [], [], []
        for b, (spans, n) in enumerate(zip(spans22, n22)):
            n_out = self.ctx.vocoder_samples(self.ctx.mel_frames(int(n)), True)
            w, which = G.plan_patch_windows(G.blend_regions(spans, int(n), n_out, fade) if regions is None else regions[b], n_out // hop, hop, rf)
            span_win += [len(wins) + k if k >= 0 else -1 for k in which]
            wins += [(b, w0, w1) for w0, w1 in w]
            per_clip.append(w)
            lim.append(min(int(n), n_out))
        return {"fade": int(fade), "hop": hop, "wins": wins, "windows": per_clip, "span_win": span_win, "lim": lim, "n22": [int(n) for n in n22]}

    @staticmethod
    def patch_words(plan: Dict[str, object]) -> int:
        """int32 words the tables of a plan take in a staging buffer: the PatchTable, the window table of the gather, the lengths."""
        W, B = len(plan["wins"]), len(plan["lim"])
        return PatchTable.words(W, len(plan["span_win"]), B, plan["fade"]) + 3 * W + B

    def _patch_tables(self, plan: Dict[str, object], staged=None) -> Dict[str, object]:
        """Adds the device tables to a plan: table (PatchTable), gwin (the gather's window words, host + device) and len22 (device
        int32 (B)).  staged = (host, dev) views of `patch_words(plan)` words that the CALLER copies."""
        wins, hop, B = plan["wins"], plan["hop"], len(plan["lim"])
        W = len(wins)
        rows = [(b, w0 * hop, (w1 - w0) * hop) for b, w0, w1 in wins]
        if staged is None:
            plan["table"] = PatchTable(rows, plan["span_win"], plan["lim"], plan["fade"], self.device)
            plan["gwin"] = None
            plan["len22"] = torch.tensor(plan["n22"], dtype=torch.int32).to(self.device)
            return plan
        hp, dv = staged
        wt = PatchTable.words(W, len(plan["span_win"]), B, plan["fade"])
        plan["table"] = PatchTable(rows, plan["span_win"], plan["lim"], plan["fade"], self.device, staged=(hp[:wt], dv[:wt]))
        hp[wt:wt + 3 * W] = self.ctx.window_words(wins)
        hp[wt + 3 * W:wt + 3 * W + B] = plan["n22"]
        plan["gwin"] = (hp[wt:wt + 3 * W], dv[wt:wt + 3 * W])
        plan["len22"] = dv[wt + 3 * W:wt + 3 * W + B]
        return plan

    def _compose(self, wave22: torch.Tensor, tab22: SpanTable, table: PatchTable, gen: Optional[torch.Tensor], len22_host, len22_dev,
                 pcm: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        # the front-end divided by this peak and multiplied by 0.95 (I_ea/predict.py:104): the generated audio goes back by peak / 0.95
        gain = self.ctx.wave_peak(wave22, tab22, len22_dev) / 0.95
        return self.ctx.patch_compose(wave22, tab22, table, gen, gain, sample_len=len22_host, f32=True, pcm=pcm)

    def patch_multigap_batch(self, wave16: torch.Tensor, wave22: torch.Tensor, gaps, fade: int = 110, len16: Optional[Sequence[int]] = None,
                             len22: Optional[Sequence[int]] = None, spans22: Optional[Sequence[Sequence[Sequence[int]]]] = None,
                             tables: Optional[Dict[str, object]] = None, pcm: bool = False) -> Dict[str, object]:
        """`predict_multigap_batch` on RAW 22.05 kHz clips whose output is the caller's own recording with only the gaps filled:
        `patched` (B, N22) fp32 equals wave22 BIT FOR BIT outside a cross-fade of `fade` samples (22.05 kHz; 110 ~ 5 ms; 0 = hard
        splice) around each gap, and inside the gaps it is the generator's audio at the recording's level (the front-end's peak
        normalisation undone).  The generator runs only over the windows of the stretched mel those samples need
        (gaps.plan_patch_windows), as one ragged stretch=False batch -- bit-identical there to a full pass.  A clip without gaps comes
        back as an exact copy.  tables: `gap_tables(..., patch_fade=fade)`'s result.
        -> predict_multigap_batch's dictionary WITHOUT `wave`, plus patched, patched_pcm (int16, with pcm=True), patch_windows
        (per clip the (w0, w1) stretched-frame windows that were vocoded)."""
        if wave22.dim() != 2:
            raise ValueError("patch_multigap_batch: patch mode keeps the caller's samples, so it needs the raw (B, N22) 22.05 kHz clips")
        B = wave16.shape[0]
        ragged = len16 is not None
        if ragged and len22 is None:
            raise ValueError("patch_multigap_batch: a ragged batch needs len22")
        n16 = [int(n) for n in len16] if ragged else [wave16.shape[1]] * B
        n22 = [int(n) for n in len22] if len22 is not None else [wave22.shape[1]] * B
        tb = tables if tables is not None else self.gap_tables(gaps, n16, n22, spans22=spans22, patch_fade=fade)
        plan = tb.get("patch")
        if plan is None or plan["fade"] != int(fade):
            raise ValueError("patch_multigap_batch: `tables` were not built by gap_tables(..., patch_fade=fade) for this fade")
        out = self.predict_multigap_batch(wave16, wave22, gaps, len16=len16, len22=len22 if ragged else None, tables=tb, vocode=False)
        wins, gen = plan["wins"], None
        if wins:
            ext, _ = self._stretch(out["mel"], plan["hop"], out["mel_len"] if ragged else None, plan["windows"])
            gen = self._vocode_gathered(ext, wins, plan["gwin"])
        patched, ppcm = self._compose(wave22, tb["tab22"], plan["table"], gen, n22 if ragged else None, plan["len22"] if ragged else None, pcm)
        out.update(patched=patched, patch_windows=plan["windows"])
        if pcm:
            out["patched_pcm"] = ppcm
        return out

    def patch_from_wave(self, wave22: torch.Tensor, wave: torch.Tensor, tab22: SpanTable, fade: int = 110, len22: Optional[Sequence[int]] = None,
                        wave_len: Optional[Sequence[int]] = None, pcm: bool = False):
        """The same composition from a FULL generator pass `wave` (B, L) of the spliced mel (for callers who also want `wave`, and
        the reference the windowed route is tested against): one window per clip, starting at sample 0.  tab22: the 22.05 kHz
        SpanTable the mel front-end read; len22 / wave_len: per-clip samples of a ragged batch.  -> (patched, patched_pcm or None)."""
        B, L = wave.shape
        n22 = [int(n) for n in len22] if len22 is not None else [wave22.shape[1]] * B
        wl = [int(n) for n in wave_len] if wave_len is not None else [L] * B
        spans = tab22.spans()
        rows = [(b, 0, min(wl[b], wave22.shape[1])) for b in range(B)]
        table = PatchTable(rows, [b for b in range(B) for _ in spans[b]], [min(n, w) for n, w in zip(n22, wl)], fade, self.device)
        l22 = None if len22 is None else torch.tensor(n22, dtype=torch.int32).to(self.device)
        return self._compose(wave22.contiguous(), tab22, table, wave.contiguous(), n22 if len22 is not None else None, l22, pcm)

    # ---- recordings longer than one clip: context clips cut from, and patched back into, the one recording
    def _region_table(self, ctxs: Sequence[dict], plan: Dict[str, object], spans22: Sequence[Sequence[Sequence[int]]]) -> RegionTable:
        """One batch of contexts, their own 22.05 kHz spans (local samples) and the `plan_patch` of those spans -> the RegionTable on
        the recording's sample axis: every local sample shifted by 441 * the context's first frame."""
        hop, fade = plan["hop"], plan["fade"]
        off = [441 * int(c["start"]) for c in ctxs]
        spans, regions, k = [], [], 0
        for b, clip in enumerate(spans22):
            for (s, l), reg in zip(clip, G.blend_regions(clip, plan["n22"][b], plan["lim"][b], fade)):
                if reg is not None:
                    spans.append((off[b] + s, l, plan["span_win"][k], off[b] + plan["lim"][b]))
                    regions.append((off[b] + reg[0], off[b] + reg[1]))
                k += 1
        wins = [(b, off[b] + w0 * hop, (w1 - w0) * hop) for b, w0, w1 in plan["wins"]]
        return RegionTable(spans, wins, G.region_chunks(regions), len(ctxs), fade, self.device)

    def patch_recording(self, wave22, gaps, wave16=None, fade: int = 110, clip_frames: int = 200, min_context: int = 50, batch: int = 32,
                        pcm: bool = False, ceiling: Optional[float] = None) -> Dict[str, object]:
        """Patch mode for a recording of ANY length: wave22 (N22,) is the recording at 22.05 kHz (tensor or array, host or device),
        gaps = (first frame, frame count) pairs on ITS 20 ms grid (frame p = samples [441 p, 441 (p + 1))).  gaps.plan_contexts groups
        the gaps into context clips of clip_frames frames that start on the recording's frame grid; per batch of at most `batch`
        contexts the clips are cut on the device (si_cut_clips; from wave16 (N16,), the same recording at 16 kHz, at 320 f when it is
        given, else the cut 22.05 kHz clips are resampled), go through ONE multi-gap pass with every gap they hold masked (their own
        and the neighbours' that fall into them), the generator runs over the windows of the OWN gaps only, and one si_patch_regions
        launch writes the blended samples into `patched`, a copy of the recording.  Every written sample is the one
        patch_multigap_batch gives for that context clip; every other sample is wave22's, bit for bit.
        -> patched (N22,) fp32, patched_pcm (N22,) int16 with pcm=True, contexts (the plan), labels (flat, int64) / label_off
        (gaps + 1): the predicted codewords per gap in sorted gap order, each from the context that owns the gap.
        A recording without gaps comes back as an exact copy and no model kernel is launched.
        ceiling: None is the calls above.  A float > 0, +inf included, cuts every clip through si_cut_clips_valid -- the
        clips of wave16 too, under the same number: both are fp32 in full-scale units -- so that a sample that is NaN, +-inf or above
        the ceiling reaches the model as +0.0 and stays inside its gap.  `patched` still starts as a copy of wave22 and is blended
        against wave22: a sample of weight 0 keeps its bits, NaN payload included; only the clips are cleaned, and no copy of the
        recording's length is made for it."""
        self._need(head=True, codebook=True, what="patch_recording")
        ceiling = InpaintingEngine._ceiling(ceiling, "patch_recording")
        as1d = lambda x: torch.as_tensor(x).to(self.device, torch.float32).reshape(-1).contiguous()
        wave22 = as1d(wave22)
        wave16 = None if wave16 is None else as1d(wave16)
        fade, batch = int(fade), int(batch)
        if batch <= 0:
            raise ValueError(f"patch_recording: batch = {batch}")
        patched = wave22.clone()
        out: Dict[str, object] = {"patched": patched}
        if pcm:
            out["patched_pcm"] = self.to_int16(wave22)

        def write(cb, tb, res, w22, L22):
            own22 = G.spans22([c["own"] for c in cb], [L22] * len(cb))
            plan = self.plan_patch(own22, [L22] * len(cb), fade)
            if plan["wins"]:
                ext, _ = self._stretch(res["mel"], plan["hop"], None, plan["windows"])
                gen = self._vocode_gathered(ext, plan["wins"])
                # the front-end divided by this peak and multiplied by 0.95 (I_ea/predict.py:104), with ALL gaps of the context zeroed
                gain = self.ctx.wave_peak(w22, tb["tab22"]) / 0.95
                self.ctx.patch_regions(wave22, self._region_table(cb, plan, own22), gen, gain, patched, out.get("patched_pcm"))

        cut = lambda cb, L: self.ctx.cut_clips(wave22, [441 * c["start"] for c in cb], L, ceiling=ceiling)
        out.update(self._recording_passes(wave22.numel(), cut, wave16, gaps, max(-(-fade // 441), 1), clip_frames, min_context, batch, write,
                                          ceiling=ceiling))
        return out

    @staticmethod
    def _ceiling(ceiling, fn: str) -> Optional[float]:
        """The `ceiling` argument of the patch calls: None, or a float > 0 (+inf allowed) that is not NaN."""
        if ceiling is None:
            return None
        c = float(ceiling)
        if not c > 0.0:
            raise ValueError(f"{fn}: ceiling = {ceiling} is not above 0, or is NaN (+inf, the samples that are not finite, is allowed)")
        return c

    def _recording_passes(self, N22: int, cut, wave16: Optional[torch.Tensor], gaps, fade_frames: int, clip_frames: int,
                          min_context: int, batch: int, write, channel_gaps=None, cut16=None, ceiling: Optional[float] = None) -> Dict[str, object]:
        """What patch_recording and patch_file share: the context plan of a recording of N22 samples at 22.05 kHz and, per batch of
        at most `batch` contexts, the cut -- cut(cb, L22) -> the (B, L22) clips of the contexts cb, which start at 22.05 kHz samples
        441 * start, on the device --, the one multi-gap pass with every gap the clips hold masked, and the labels of the own gaps.
        write(cb, tb, res, w22, L22) -- the contexts of the pass, their gap tables, the pass's result (vocode=False), the cut
        22.05 kHz clips (B, L22) -- plans the generator windows of the own gaps, runs the generator over them and writes the blended
        samples.  -> contexts, labels, label_off.
        channel_gaps: one gap list per channel of an interleaved file in place of `gaps`.  Every channel is planned
        as a recording of its own (gaps.plan_channel_contexts), the contexts follow in (channel, start) order with a "channel" key, the
        batches fill across channels, and labels / label_off run over the gaps in (channel, gap) order; + channel_off.
        cut16: cut16(cb, L22, L16) -> (the (B, L22) clips, the (B, L16) clips at 16 kHz, which start at samples 320 *
        start), both from the cutter, in place of `cut` and of the resampling of its clips; wave16 is None then.
        ceiling: cuts the clips of a supplied wave16 through si_cut_clips_valid; `cut` / `cut16` clean their own."""
        N22, clip_frames, batch = int(N22), int(clip_frames), int(batch)
        n_rec = N22 // 441
        whole = n_rec <= clip_frames                                   # one context: the whole recording, with its true sample counts
        L22 = N22 if whole else clip_frames * 441
        if wave16 is not None:
            L16 = wave16.numel() if whole else clip_frames * 320
        else:
            L16 = -(-L22 * 16000 // 22050)
        out: Dict[str, object] = {}
        lim = min(self.ctx.num_frames(L16), self.ctx.mel_frames(L22)) if L16 > 0 and L22 > 0 else 0
        if channel_gaps is None:
            ctxs = G.plan_contexts(gaps, n_rec, clip_frames, min_context, lim_frames=lim, fade_frames=int(fade_frames))
        else:
            ctxs, out["channel_off"] = G.plan_channel_contexts(channel_gaps, n_rec, clip_frames, min_context, lim_frames=lim,
                                                               fade_frames=int(fade_frames))
        n_gaps = sum(len(c["own"]) for c in ctxs)
        out["contexts"] = ctxs
        labels = []
        for i in range(0, len(ctxs), batch):
            cb = ctxs[i:i + batch]
            B = len(cb)
            if cut16 is not None:
                w22, w16 = cut16(cb, L22, L16)
            else:
                w22 = cut(cb, L22)
                if wave16 is None:
                    w16 = self.resample(w22, 22050, 16000)
                else:
                    w16 = self.ctx.cut_clips(wave16, [320 * c["start"] for c in cb], L16, ceiling=ceiling)
            tb = self.gap_tables([c["own"] + c["foreign"] for c in cb], [L16] * B, [L22] * B)
            res = self.predict_multigap_batch(w16, w22, None, tables=tb, vocode=False)
            write(cb, tb, res, w22, L22)
            # labels of the own gaps: clip b's gaps lie sorted in the flat label vector, gap by gap
            idx = []
            for b, c in enumerate(cb):
                o = tb["label_off"][b]
                for p, l in tb["gaps"][b]:
                    if (p, l) in c["own"]:
                        idx += range(o, o + l)
                    o += l
            labels.append(res["labels"][torch.tensor(idx, dtype=torch.int64).to(self.device)])
        out["labels"] = torch.cat(labels) if labels else torch.zeros(0, dtype=torch.int64, device=self.device)
        out["label_off"] = G.gap_label_off(ctxs, n_gaps)
        return out

    # ---- repair at the file's own sample rate: the recording stays at `sr` in its own sample type
    def _rate_filter(self, sr: int) -> Dict[str, object]:
        """audio.design_kaiser_best(22050, sr, .) with win / dwin on the device (time_reg is not used) + reach = taps per wing: the
        tables resample(., 22050, sr) runs on, held once."""
        return self._sinc_tables(22050, sr)

    def plan_rate(self, ctxs: Sequence[dict], L22: int, sr: int, n_file: int, fade_f: int, reach: int) -> Dict[str, object]:
        """Host planning of one pass of patch_file: the own gaps of the contexts `ctxs` (clips of L22 samples at 22.05 kHz) as spans
        and blend regions on the FILE's sample axis (gaps.file_spans / file_lim / file_regions), those regions mapped to the 22.05 kHz
        samples their interpolation reads (gaps.reach_regions22, `reach` taps per wing), and the generator windows that keep them
        (plan_patch).  -> plan_patch's dictionary + spans ((start, len, window, lim_f) rows), regions (file samples), rows ((context,
        first 22.05 kHz sample, samples, lim22) per window): what RateTable takes; span_ctx: per row of spans the context it belongs to.  A ValueError names a gap whose interpolation reaches
        in front of its context (a gap within `reach` samples of a context's start that is not the recording's)."""
        hop = self.ctx.vocoder_samples(1, False)
        n_out = self.ctx.vocoder_samples(self.ctx.mel_frames(int(L22)), True)
        lim_loc = min(int(L22), n_out)
        spans, regions, local, lim22 = [], [], [], []
        for b, c in enumerate(ctxs):
            off = 441 * int(c["start"])
            lim22.append(off + lim_loc)
            lim_f = G.file_lim(off + lim_loc, sr, n_file)
            sp = G.file_spans([(c["start"] + p, l) for p, l in c["own"]], sr)
            regs = G.file_regions(sp, [lim_f] * len(sp), fade_f)
            r22 = G.reach_regions22(regs, sr, reach, 0 if off == 0 else -2 ** 62, off + lim_loc)
            for (p, l), r in zip(c["own"], r22):
                if r is not None and r[0] < off:
                    raise ValueError(f"patch_file: the interpolation of the gap at frames [{c['start'] + p}, {c['start'] + p + l}) reads 22.05 kHz sample {r[0]}, "
                                     f"its context starts at {off} (reach {reach} samples): raise min_context")
            local.append([None if r is None else (r[0] - off, r[1] - off) for r in r22])
            spans.append([(s, l, lim_f) for s, l in sp])
            regions.append(regs)
        plan = self.plan_patch([[(0, 0)] * len(c["own"]) for c in ctxs], [int(L22)] * len(ctxs), int(fade_f), regions=local)
        rows, flat_regions, span_ctx, k = [], [], [], 0
        for b in range(len(ctxs)):
            for (s, l, lim_f), reg in zip(spans[b], regions[b]):
                if reg is not None:
                    rows.append((s, l, plan["span_win"][k], lim_f))
                    flat_regions.append(reg)
                    span_ctx.append(b)
                k += 1
        plan["spans"], plan["regions"], plan["span_ctx"] = rows, flat_regions, span_ctx
        plan["rows"] = [(b, 441 * int(ctxs[b]["start"]) + w0 * hop, (w1 - w0) * hop, lim22[b]) for b, w0, w1 in plan["wins"]]
        return plan

    def _feed_filter16(self, sr: int) -> Optional[Dict[str, object]]:
        """audio.design_kaiser_best(sr, 16000, .) with win / dwin on the device: what si_cut_pair takes for its 16 kHz rows (DESIGN.md
        4.26) -- the tables resample(., sr, 16000) runs on, from the same cache.  None for a 16 kHz file: its samples are the rows."""
        return None if int(sr) == 16000 else self._sinc_tables(sr, 16000)

    def _feed_filter(self, sr: int) -> Dict[str, object]:
        """audio.design_kaiser_best(sr, 22050, .) with win / dwin on the device (time_reg is not used): what si_cut_rate takes -- the
        tables resample(., sr, 22050) runs on, held once."""
        return self._sinc_tables(sr, 22050)

    @staticmethod
    def _file_samples(x: torch.Tensor, fn: str) -> Tuple[bool, int]:
        """(s24, sample dimensions) of a file x: packed 24-bit PCM is a uint8 tensor whose last dimension is the
        sample's 3 bytes, (n, 3) mono or (n, ch, 3) interleaved -- np.frombuffer(data, np.uint8).reshape(n, ch, 3) of a WAV data chunk;
        the sample dimensions are those in front of it.  Any other uint8 shape is refused here, before any launch."""
        if x.dtype != torch.uint8:
            return False, x.dim()
        if x.dim() not in (2, 3) or x.shape[-1] != 3:
            raise ValueError(f"{fn}: a uint8 input is packed 24-bit PCM, (n, 3) mono or (n, ch, 3) interleaved, not {tuple(x.shape)}")
        return True, x.dim() - 1

    @staticmethod
    def _file_on_device(x: torch.Tensor, device) -> torch.Tensor:
        """x on `device` in the sample type it is read in: int16 and packed 24-bit bytes as they are, anything else as fp32."""
        return x.to(device, x.dtype if x.dtype in (torch.int16, torch.uint8) else torch.float32)

    def patch_file(self, x, sr: int, gaps=None, fade_ms: float = 5.0, clip_frames: int = 200, min_context: int = 50, batch: int = 32,
                   return_windows: bool = False, feed: str = "recording", channel_gaps=None, clips16: str = "resampled",
                   ceiling: Optional[float] = None) -> Dict[str, object]:
        """patch_recording for a file at ITS OWN sample rate and in its own sample type: x (n,) is the recording at `sr` Hz, fp32 in
        full-scale units or int16 PCM (tensor or array, host or device), gaps = (first frame, frame count) pairs on its 20 ms grid.
        The recording is resampled to 22.05 kHz here (`resample`) only to FEED the model; the contexts, the multi-gap passes and the
        labels are patch_recording's (one shared body).  The generator runs over windows widened by the interpolation's reach, and one
        si_patch_rate launch per pass carries its samples to `sr` by band-limited interpolation at the exact time i * 22050 / sr and
        blends them into `patched`, a copy of x: every sample outside a cross-fade of fade_ms around a gap is x's, bit for bit.
        sr = 22050 is patch_recording itself, bit for bit.
        feed="contexts"  feeds the model without that whole-file resample: per pass one si_cut_rate launch cuts the
        context clips straight from x at its own rate and in its own sample type (an int16 file is read as int16), interpolating at
        the exact time j * sr / 22050 with the file's real neighbours at the clip edges; nothing of the recording's length is
        created but `patched`.  The clips differ from the slices of the whole-file resample by at most an fp32 rounding, except at
        exactly-integer times and in the recording's last sample (4.17 (a), (b)); everything after the cut is the same code.
        -> patched (n,) in x's dtype, contexts, labels, label_off as patch_recording; return_windows=True adds passes: per pass its
        contexts, gen (W, Lrow), gain (C,), table (RateTable), plan and clips22 (the cut 22.05 kHz clips).  No gaps: an exact copy,
        no model kernel launched.
        An INTERLEAVED file x (n, ch), 1 <= ch <= 8, as a WAV stores it: every channel is a mono recording to the
        model, repaired exactly as patch_file repairs x[:, c] alone -- byte for byte -- and the contexts of all channels share the
        passes.  `gaps` is one list for every channel; channel_gaps is one list per channel instead (an empty one: that channel comes
        back as the file's).  x is never flattened, and with feed="contexts" never de-interleaved: si_cut_rate_ch and si_patch_rate_ch
        read and write channel c in place, one launch each per channel present in a pass.  -> patched (n, ch), contexts with a
        "channel" key in (channel, start) order, labels / label_off over the gaps in (channel, gap) order, channel_off (ch + 1): the
        gaps of channel c are [channel_off[c], channel_off[c + 1]); with return_windows a pass holds tables ((channel, RateTable)
        pairs) in place of table.  (n, 1) is the mono route with patched reshaped.  A file at sr = 22050 goes channel by channel
        through patch_recording, as the mono file does: feed and return_windows are not read there and no `passes` come back.
        clips16: "resampled" (the default) makes the encoder's 16 kHz clips from the cut 22.05 kHz clips, each clip
        resampled as a file of its own; "file" (needs feed="contexts") cuts them straight from x as well, at the exact 16 kHz times with
        the file's real neighbours at the clip edges, as the reference's second load of the file does (I_ea/predict.py:80): one
        si_cut_pair launch per pass -- si_cut_pair_ch per channel present in a pass -- yields both clip sets, the 22.05 kHz ones with
        si_cut_rate's bytes, and no resample_sinc runs.  A 16 kHz file's own samples reach the encoder.  return_windows then adds clips16
        per pass.  At sr = 22050 it is not read, as feed is not.
        PACKED 24-BIT PCM: x uint8, (n, 3) mono or (n, ch, 3) interleaved, the bytes of a WAV data chunk.  It needs
        feed="contexts": the clips are cut from the bytes (a sample enters as v * 2^-23, exact) and si_patch_rate writes the three
        bytes of each blended sample -- trunc(w * 2^23), clamped -- into `patched`, a uint8 copy of x's shape; no fp32 image of the
        file exists.  Everything else above holds as for int16.  A 22.05 kHz s24 file is refused.
        ceiling: None is everything above, call for call.  A float > 0 in x's own units (full scale for fp32, the
        file's steps for PCM; +inf = the samples that are not finite) cuts every clip of every pass through si_cut_rate_valid or
        si_cut_pair_valid, which stage a sample that is NaN, +-inf or above the ceiling as +0.0: it no longer leaves its gap through the
        interpolation's taps.  It needs feed="contexts" at sr != 22050 -- the whole-file resample would smear the damage before anything
        could clean it -- and at sr = 22050 it is patch_recording's.  `patched` still starts as a copy of x and is blended against x;
        no copy of the file's length is made for the cleaning.  A non-finite sample under a cross-fade weight 0 < w < 1 stays non-finite:
        type the gap so that it covers the run (find_gaps(kind="invalid") does)."""
        self._need(head=True, codebook=True, what="patch_file")
        ceiling = InpaintingEngine._ceiling(ceiling, "patch_file")
        if feed not in ("recording", "contexts"):
            raise ValueError(f"patch_file: feed = {feed!r}: 'recording' or 'contexts'")
        if clips16 not in ("resampled", "file"):
            raise ValueError(f"patch_file: clips16 = {clips16!r}: 'resampled' or 'file'")
        sr, batch = int(sr), int(batch)
        P, Q = G.rate_ratio(sr)
        if batch <= 0:
            raise ValueError(f"patch_file: batch = {batch}")
        if ceiling is not None and sr != 22050 and feed != "contexts":
            raise ValueError(f"patch_file: ceiling = {ceiling} needs feed=\"contexts\" at {sr} Hz (feed = {feed!r} resamples the whole file, which "
                             f"smears an invalid sample over every output within the filter's reach before anything could clean it)")
        x = torch.as_tensor(x)
        s24, sdim = InpaintingEngine._file_samples(x, "patch_file")
        if s24 and feed != "contexts":
            raise ValueError(f"patch_file: packed 24-bit PCM needs feed = 'contexts' (feed = {feed!r} resamples an fp32 image of the whole file)")
        if s24 and sr == 22050:
            raise ValueError("patch_file: packed 24-bit PCM at 22050 Hz is not served: that file goes through patch_recording as fp32")
        if gaps is not None and channel_gaps is not None:
            raise ValueError("patch_file: both gaps and channel_gaps: one list for every channel, or one list per channel")
        if sdim == 2:
            per = G.channel_gap_lists(gaps, channel_gaps, x.shape[1])
            kw = dict(fade_ms=fade_ms, clip_frames=clip_frames, min_context=min_context, batch=batch, return_windows=return_windows, feed=feed,
                      clips16=clips16)
            if ceiling is not None:
                kw["ceiling"] = ceiling
            if x.shape[1] == 1:
                out = self.patch_file(x.reshape(-1, 3) if s24 else x.reshape(-1), sr, per[0], **kw)
                out["patched"] = out["patched"].reshape(x.shape)
                return out
            return self._patch_file_channels(x, sr, per, **kw)
        if gaps is None:
            raise ValueError("patch_file: a one-channel (n,) recording takes `gaps`; channel_gaps belongs to an (n, ch) file")
        pcm = x.dtype == torch.int16
        x = InpaintingEngine._file_on_device(x, self.device).contiguous() if s24 else x.to(self.device, torch.int16 if pcm else torch.float32).reshape(-1).contiguous()
        n_file = x.shape[0]
        if n_file < 1 or n_file > 2 ** 31 - 1 - 2048:
            raise ValueError(f"patch_file: a file of {n_file} samples")
        fade_f = G.file_fade(fade_ms, sr)
        if sr == 22050:
            xf = x.to(torch.float32) / 32768.0 if pcm else x           # exact: 16 bits x 2^-15
            # the ceiling of the fp32 image of an int16 file: |v| <= c <=> |v| / 32768 <= c / 32768, a power of two
            kc = {} if ceiling is None else {"ceiling": ceiling / 32768.0 if pcm else ceiling}
            out = self.patch_recording(xf, gaps, fade=fade_f, clip_frames=clip_frames, min_context=min_context, batch=batch, pcm=pcm, **kc)
            if pcm:
                out["patched"] = out.pop("patched_pcm")
            return out
        if clips16 == "file" and feed != "contexts":
            raise ValueError(f"patch_file: clips16 = 'file' needs feed = 'contexts' (with feed = {feed!r} the clips are slices of the resampled recording)")
        patched = x.clone()
        out: Dict[str, object] = {"patched": patched}
        passes = []
        gaps = list(gaps)
        if not gaps:                                                   # nothing to repair: not even the resampler runs
            out.update(contexts=[], labels=torch.zeros(0, dtype=torch.int64, device=self.device), label_off=[0])
            if return_windows:
                out["passes"] = passes
            return out
        if feed == "contexts":                                         # the clips alone, cut from x itself
            fin = self._feed_filter(sr)
            N22 = -(-n_file * P // Q)
            cut = lambda cb, L: self.ctx.cut_rate(x, sr, [441 * c["start"] for c in cb], L, fin, ceiling=ceiling)
        else:
            xf = x.to(torch.float32) / 32768.0 if pcm else x           # exact: 16 bits x 2^-15
            wave22 = self.resample(xf[None], sr, 22050)[0].contiguous()
            N22 = wave22.numel()
            cut = lambda cb, L: self.ctx.cut_clips(wave22, [441 * c["start"] for c in cb], L)
        cut16, last16 = None, {}
        if clips16 == "file":                                          # both clip sets of a pass from x itself, in one launch
            fin16 = self._feed_filter16(sr)

            def cut16(cb, L22, L16):
                w22, last16["w16"] = self.ctx.cut_pair(x, sr, [c["start"] for c in cb], L22, L16, fin, fin16, ceiling=ceiling)
                return w22, last16["w16"]
        filt = self._rate_filter(sr)

        def write(cb, tb, res, w22, L22):
            plan = self.plan_rate(cb, L22, sr, n_file, fade_f, filt["reach"])
            if plan["wins"]:
                ext, _ = self._stretch(res["mel"], plan["hop"], None, plan["windows"])
                gen = self._vocode_gathered(ext, plan["wins"])
                # the front-end divided by this peak and multiplied by 0.95 (I_ea/predict.py:104), with ALL gaps of the context zeroed
                gain = self.ctx.wave_peak(w22, tb["tab22"]) / 0.95
                table = RateTable(plan["spans"], plan["rows"], G.region_chunks(plan["regions"]), len(cb), fade_f, self.device)
                self.ctx.patch_rate(x, sr, table, gen, filt, patched, gain)
                if return_windows:
                    passes.append({"contexts": cb, "gen": gen, "gain": gain, "table": table, "plan": plan, "clips22": w22, **({"clips16": last16["w16"]} if last16 else {})})

        fade_frames = max(-(-fade_f * 50 // sr), 1)
        out.update(self._recording_passes(N22, cut, None, gaps, fade_frames, clip_frames, min_context, batch, write, cut16=cut16))
        if return_windows:
            out["passes"] = passes
        return out

    def _patch_file_channels(self, x: torch.Tensor, sr: int, channel_gaps, fade_ms: float, clip_frames: int, min_context: int, batch: int,
                             return_windows: bool, feed: str, clips16: str = "resampled", ceiling: Optional[float] = None) -> Dict[str, object]:
        """patch_file for an interleaved file x (n, ch >= 2) with one gap list per channel.  ceiling: patch_file's
        (the caller refused it with feed="recording" at this rate)."""
        n_file, ch = x.shape[:2]                                       # packed 24-bit: (n, ch, 3) bytes, feed = "contexts"
        if ch > G.MAX_CHANNELS:
            raise ValueError(f"patch_file: a file of {ch} channels, at most {G.MAX_CHANNELS}")
        pcm = x.dtype == torch.int16
        x = InpaintingEngine._file_on_device(x, self.device).contiguous()
        if n_file < 1 or n_file > 2 ** 31 - 1 - 2048:
            raise ValueError(f"patch_file: a file of {n_file} samples")
        P, Q = G.rate_ratio(sr)
        fade_f = G.file_fade(fade_ms, sr)
        if sr == 22050:                                                # patch_recording, channel by channel, as the mono file goes
            kc = {} if ceiling is None else {"ceiling": ceiling}
            outs = [self.patch_file(x[:, c].contiguous(), sr, channel_gaps[c], fade_ms=fade_ms, clip_frames=clip_frames, min_context=min_context,
                                    batch=batch, **kc) for c in range(ch)]
            off = [0]
            for o in outs:
                off.append(off[-1] + len(o["label_off"]) - 1)
            ctxs = [dict(k, channel=c, own_index=[off[c] + i for i in k["own_index"]]) for c, o in enumerate(outs) for k in o["contexts"]]
            label_off = [0]
            for o in outs:
                label_off += [label_off[-1] + v for v in o["label_off"][1:]]
            return {"patched": torch.stack([o["patched"] for o in outs], dim=1), "contexts": ctxs, "labels": torch.cat([o["labels"] for o in outs]),
                    "label_off": label_off, "channel_off": off}
        if clips16 == "file" and feed != "contexts":
            raise ValueError(f"patch_file: clips16 = 'file' needs feed = 'contexts' (with feed = {feed!r} the clips are slices of the resampled recording)")
        patched = x.clone()
        out: Dict[str, object] = {"patched": patched}
        passes = []
        if not any(channel_gaps):                                      # nothing to repair: not even the resampler runs
            out.update(contexts=[], labels=torch.zeros(0, dtype=torch.int64, device=self.device), label_off=[0], channel_off=[0] * (ch + 1))
            if return_windows:
                out["passes"] = passes
            return out
        if feed == "contexts":                                         # the clips alone, cut from x itself, channel c in place
            fin = self._feed_filter(sr)
            N22 = -(-n_file * P // Q)
            cut_rows = lambda c, starts, L, rows: self.ctx.cut_rate(x, sr, starts, L, fin, out=rows, channel=c, ceiling=ceiling)
        else:                                                          # the whole-file resample per channel: it de-interleaves
            wave22 = {}
            for c in range(ch):
                if channel_gaps[c]:
                    xc = x[:, c].contiguous()
                    xf = xc.to(torch.float32) / 32768.0 if pcm else xc   # exact: 16 bits x 2^-15
                    wave22[c] = self.resample(xf[None], sr, 22050)[0].contiguous()   # row by row: the mono call's own launch
            N22 = next(iter(wave22.values())).numel()
            cut_rows = lambda c, starts, L, rows: self.ctx.cut_clips(wave22[c], starts, L, out=rows)
        cut16, last16 = None, {}
        if clips16 == "file":                                          # both clip sets of a pass, channel c in place: one launch per channel
            fin16 = self._feed_filter16(sr)

            def cut16(cb, L22, L16):
                w22 = torch.empty(len(cb), L22, dtype=torch.float32, device=self.device)
                last16["w16"] = w16 = torch.empty(len(cb), L16, dtype=torch.float32, device=self.device)
                for c, r0, r1 in G.pass_channels(cb):
                    self.ctx.cut_pair(x, sr, [k["start"] for k in cb[r0:r1]], L22, L16, fin, fin16, out22=w22[r0:r1], out16=w16[r0:r1], channel=c,
                                      ceiling=ceiling)
                return w22, w16
        filt = self._rate_filter(sr)

        def cut(cb, L):
            w22 = torch.empty(len(cb), L, dtype=torch.float32, device=self.device)
            for c, r0, r1 in G.pass_channels(cb):                      # a channel's clips are consecutive rows of the pass
                cut_rows(c, [441 * k["start"] for k in cb[r0:r1]], L, w22[r0:r1])
            return w22

        def write(cb, tb, res, w22, L22):
            plan = self.plan_rate(cb, L22, sr, n_file, fade_f, filt["reach"])
            if plan["wins"]:
                ext, _ = self._stretch(res["mel"], plan["hop"], None, plan["windows"])
                gen = self._vocode_gathered(ext, plan["wins"])
                # the front-end divided by this peak and multiplied by 0.95 (I_ea/predict.py:104), with ALL gaps of the context zeroed
                gain = self.ctx.wave_peak(w22, tb["tab22"]) / 0.95
                tables = []
                for c, r0, r1 in G.pass_channels(cb):                  # the channel's spans and chunks, the pass's whole gen and gain
                    ks = [k for k, b in enumerate(plan["span_ctx"]) if r0 <= b < r1]
                    if not ks:
                        continue
                    table = RateTable([plan["spans"][k] for k in ks], plan["rows"], G.region_chunks([plan["regions"][k] for k in ks]), len(cb),
                                      fade_f, self.device)
                    self.ctx.patch_rate(x, sr, table, gen, filt, patched, gain, channel=c)
                    tables.append((c, table))
                if return_windows:
                    passes.append({"contexts": cb, "gen": gen, "gain": gain, "tables": tables, "plan": plan, "clips22": w22, **({"clips16": last16["w16"]} if last16 else {})})

        fade_frames = max(-(-fade_f * 50 // sr), 1)
        out.update(self._recording_passes(N22, cut, None, None, fade_frames, clip_frames, min_context, batch, write, channel_gaps=channel_gaps,
                                          cut16=cut16))
        if return_windows:
            out["passes"] = passes
        return out

    def conceal_file(self, x, sr: int, threshold: float = 0.0, min_ms: float = 5.0, max_ms: float = 400.0, pad_frames: int = 0,
                     merge_frames: Optional[int] = None, fade_ms: float = 5.0, clip_frames: int = 200, min_context: int = 50, batch: int = 32,
                     return_windows: bool = False, feed: str = "recording", detect: str = "each", kind: str = "quiet",
                     rel_threshold: float = 0.0, held_tol: float = 0.0, win_ms: float = _WIN_MS, clips16: str = "resampled",
                     impulse_order: int = 16, impulse_guard: int = 4, impulse_pad: int = 2, impulse_ratio: float = 10.0,
                     mend_ms: float = 0.0, mend_order: int = 32, mend_context: int = 512) -> Dict[str, object]:
        """File in, repaired file out, at the file's own rate and in its own sample type: find_gaps on x itself, where a dropout is
        still exact zeros, then patch_file with the gaps it found.  The usable frames are those of the recording's 22.05 kHz length
        ceil(n * 22050 / sr) (`recording_frames`), and a gap longer than the planner's budget counts as long, as in conceal_recording.
        threshold is in x's own units, as find_gaps takes it: full scale for fp32, int16 steps for an int16 file, 24-bit steps for
        packed 24-bit PCM (uint8 (n, 3) or (n, ch, 3), DESIGN.md 4.27: it needs feed="contexts" and comes back as uint8).
        feed: patch_file's ("recording" or "contexts").  clips16: patch_file's ("resampled" or "file"), passed on when
        it is off its default.  What patch_file refuses about feed="recording" at sr != 22050 -- clips16="file", and the ceiling of kind
        "invalid" -- is refused here in its words, before the detection has launched anything.
        -> patch_file's dictionary + gaps + skipped.  With nothing found: an exact copy; only the detection kernels launched.
        An interleaved file x (n, ch >= 2): detect="each" runs the detection once per channel and repairs a dropout
        in the channel it is in (gaps, skipped: one list per channel); detect="joint" runs it once over the sample times at which
        EVERY channel is quiet and repairs those gaps in every channel (gaps, skipped: one list).  A one-channel file ignores it.
        kind, rel_threshold, held_tol: find_gaps' (DESIGN.md 4.20); held_tol in x's own units, like threshold.  Off their defaults the
        dictionary gains `threshold`, the effective one (one per channel for detect="each" on an interleaved file).
        kind "level" with win_ms: find_gaps' (DESIGN.md 4.25), in the file's own samples like everything else here.
        kind "burst" with win_ms: find_gaps' (DESIGN.md 4.28), likewise: threshold = 1.15 of full scale and win_ms = 4.0 to start from.
        kind "invalid" (DESIGN.md 4.30): find_gaps' -- the samples whose VALUE is the damage: NaN, +-inf, and |x| > threshold when
        threshold != 0 (a ceiling in x's own units; 0, the default, is +inf: the non-finite samples only).  Pass min_ms=0: a single NaN
        is a run of one sample.  The same ceiling goes on to patch_file(ceiling=...), so the samples that were judged are the ones
        kept out of the clips; it needs feed="contexts" at sr != 22050.  An edge run (touching sample 0 or n) and a cover longer than
        the planner's budget are skipped by the existing rules and those samples stay in `patched`, listed in `skipped`.
        mend_ms: 0, the default, is everything above, call for call and launch for launch.  Above 0, the runs of at most
        max_len = round(mend_ms * sr / 1000) samples (at most 64) are first filled from their own neighbourhood by mend_runs(order =
        mend_order, context = mend_context) on a copy of the file; the rows it filled (status AR or LINE) leave the run list, the rest
        goes through gaps.runs_to_gaps and patch_file as before, and both feeds read the mended copy.  min_ms must lie under mend_ms.
        detect="each" mends every channel's own runs; detect="joint" mends the joint runs in every channel and a run leaves the gap
        list only if every channel filled it.  The dictionary gains `mended`: host rows (start, len, status) of every run of at most
        max_len samples, one list per channel where `gaps` is one (joint: one list; a row's status is AR or LINE when every channel
        filled it -- LINE if any did by the line -- else the first channel's status that is no fill).  An edge run stays `skipped`.
        kind "impulse" with win_ms and impulse_order / _guard / _pad / _ratio: find_gaps' -- clicks and pops of one to a
        few in-range samples.  Pass min_ms=0 (a click is a run of a few samples; the 5 ms default drops nearly all of them) and
        mend_ms=1.0: conceal_file(kind="impulse", min_ms=0, mend_ms=1.0) detects, mends in place, and hands what comes back NEAR, EDGE
        or LONG to the inpainter.  mend_ms=0 stays legal and costs a generated 20 ms frame per click."""
        sr, clip_frames, min_context = int(sr), int(clip_frames), int(min_context)
        if detect not in ("each", "joint"):
            raise ValueError(f"conceal_file: detect = {detect!r}: 'each' or 'joint'")
        if not float(mend_ms) >= 0.0:
            raise ValueError(f"conceal_file: mend_ms = {mend_ms} is negative or NaN (0 mends nothing)")
        mend = float(mend_ms) > 0.0
        if mend:
            mend_len = int(round(float(mend_ms) * sr / 1000.0))
            if mend_len > native.MEND_MAX_LEN:
                raise ValueError(f"conceal_file: mend_ms = {mend_ms} at {sr} Hz is max_len = {mend_len} samples, at most {native.MEND_MAX_LEN}: lower mend_ms "
                                 f"to {1000.0 * native.MEND_MAX_LEN / sr:.3f} or less; longer runs stay with the inpainter")
            if mend_len < 1:
                raise ValueError(f"conceal_file: mend_ms = {mend_ms} at {sr} Hz is less than one sample: raise it to {1000.0 / sr:.3f} or more, or pass 0")
            if float(min_ms) >= float(mend_ms):
                raise ValueError(f"conceal_file: min_ms = {min_ms} is not under mend_ms = {mend_ms}: no run short enough to mend would be reported; "
                                 f"lower min_ms (0 reports a single sample)")
            mend_len, mend_order, mend_context = self._mend_limits("conceal_file", mend_len, mend_order, mend_context)
        P, Q = G.rate_ratio(sr)
        x = torch.as_tensor(x)
        s24, sdim = InpaintingEngine._file_samples(x, "conceal_file")
        if s24 and feed != "contexts":
            raise ValueError(f"conceal_file: packed 24-bit PCM needs feed = 'contexts' (feed = {feed!r} resamples an fp32 image of the whole file)")
        if s24 and sr == 22050:
            raise ValueError("conceal_file: packed 24-bit PCM at 22050 Hz is not served: that file goes through conceal_recording as fp32")
        # patch_file's two rules on feed="recording", in its words, before the detection (and the mending) has launched anything for a call
        # that patch_file would refuse afterwards
        if feed == "recording" and sr != 22050:
            if kind == "invalid":
                raise ValueError(f"patch_file: ceiling = {G.invalid_ceiling(threshold)} needs feed=\"contexts\" at {sr} Hz (feed = {feed!r} resamples the whole "
                                 f"file, which smears an invalid sample over every output within the filter's reach before anything could clean it)")
            if clips16 == "file":
                raise ValueError(f"patch_file: clips16 = 'file' needs feed = 'contexts' (with feed = {feed!r} the clips are slices of the resampled recording)")
        shape = x.shape
        many = sdim == 2 and shape[1] >= 2                             # (n, 1) is the mono route, reshaped at the end
        if many and shape[1] > G.MAX_CHANNELS:
            raise ValueError(f"conceal_file: a file of {shape[1]} channels, at most {G.MAX_CHANNELS}")
        x = InpaintingEngine._file_on_device(x, self.device)
        x = x.contiguous() if many else (x.reshape(-1, 3) if s24 else x.reshape(-1)).contiguous()
        n_rec, lim = self.recording_frames(-(-x.shape[0] * P // Q), clip_frames)
        if n_rec > clip_frames:
            max_ms = min(float(max_ms), 20.0 * (clip_frames - 2 * min_context))
        fade22 = -(-G.file_fade(fade_ms, sr) * P // Q)
        find = lambda c: self.find_gaps(x, sr, threshold, min_ms, max_ms, pad_frames, merge_frames, fade22, n_rec, lim, channel=c, kind=kind,
                                        rel_threshold=rel_threshold, held_tol=held_tol, **({"win_ms": win_ms} if kind in ("level", "burst") else {}),
                                        **(self._impulse_keywords(win_ms, impulse_order, impulse_guard, impulse_pad, impulse_ratio) if kind == "impulse" else {}))
        kw = dict(fade_ms=fade_ms, clip_frames=clip_frames, min_context=min_context, batch=batch, return_windows=return_windows, feed=feed)
        if clips16 != "resampled":                                     # the default: patch_file is called as it was
            kw["clips16"] = clips16
        if kind == "invalid":                                          # no other kind hands patch_file a new keyword
            kw["ceiling"] = G.invalid_ceiling(threshold)
        if mend:
            return self._conceal_mended(x, sr, find, kw, many, detect == "each", shape, sdim, (mend_len, mend_order, mend_context),
                                        (n_rec, lim, pad_frames, merge_frames, fade22, max_ms))
        if many and detect == "each":
            found = [find(c) for c in range(shape[1])]
            out = self.patch_file(x, sr, channel_gaps=[f["gaps"] for f in found], **kw)
            out["gaps"], out["skipped"] = [f["gaps"] for f in found], [f["skipped"] for f in found]
            if "threshold" in found[0]:
                out["threshold"] = [f["threshold"] for f in found]
            return out
        found = find(-1 if many else None)
        out = self.patch_file(x, sr, found["gaps"], **kw)
        out["gaps"], out["skipped"] = found["gaps"], found["skipped"]
        if "threshold" in found:
            out["threshold"] = found["threshold"]
        if not many and sdim == 2:
            out["patched"] = out["patched"].reshape(shape)
        return out

    def _conceal_mended(self, x: torch.Tensor, sr: int, find, kw, many: bool, each: bool, shape, sdim: int, limits, rules) -> Dict[str, object]:
        """conceal_file with mend_ms > 0: detect on x, mend the short runs in a copy y, map the runs that are left onto
        the 20 ms grid with find_gaps' own arithmetic, and patch y."""
        max_len, order, context = limits
        n_rec, lim, pad_frames, merge_frames, fade22, max_ms = rules
        mf = 2 * max(-(-int(fade22) // 441), 1) if merge_frames is None else int(merge_frames)
        to_gaps = lambda rows: G.runs_to_gaps(rows, x.shape[0], sr, n_rec, lim, pad_frames, mf, max(int(float(max_ms) // 20), 1))
        filled = (native.MEND_AR, native.MEND_LINE)
        y = x.clone()

        def mend_rows(runs, channels):
            """-> (the rows of at most max_len samples with their status, the rows that stay runs)."""
            rows = [(int(s), int(l)) for s, l in runs.tolist()]
            per = [self.mend_runs(y, runs, max_len, order, context, channel=c, inplace=True)[1].tolist() for c in channels] if rows else []
            status = []
            for i in range(len(rows)):
                col = [st[i] for st in per]
                bad = [v for v in col if v not in filled]
                status.append(bad[0] if bad else native.MEND_LINE if native.MEND_LINE in col else native.MEND_AR)
            mended = [(s, l, st) for (s, l), st in zip(rows, status) if l <= max_len]
            return mended, [r for r, st in zip(rows, status) if st not in filled]

        if many and each:
            found = [find(c) for c in range(shape[1])]
            done = [mend_rows(f["runs"], [c]) for c, f in enumerate(found)]
            mapped = [to_gaps(left) for _, left in done]
            out = self.patch_file(y, sr, channel_gaps=[g for g, _ in mapped], **kw)
            out["gaps"], out["skipped"], out["mended"] = [g for g, _ in mapped], [k for _, k in mapped], [m for m, _ in done]
            if "threshold" in found[0]:
                out["threshold"] = [f["threshold"] for f in found]
            return out
        found = find(-1 if many else None)
        mended, left = mend_rows(found["runs"], list(range(shape[1])) if many else [None])
        gaps, skipped = to_gaps(left)
        out = self.patch_file(y, sr, gaps, **kw)
        out["gaps"], out["skipped"], out["mended"] = gaps, skipped, mended
        if "threshold" in found:
            out["threshold"] = found["threshold"]
        if not many and sdim == 2:
            out["patched"] = out["patched"].reshape(shape)
        return out

    # ---- dropout detection: where the gaps are, found on the device; then patch_recording as it is
    # The six find_*_runs are one shape: their own argument checks, the file view, the call, the read-back.  The three
    # helpers are called through the class, as _file_samples is: a find_*_runs also serves a stand-in that has only what the call touches.
    def _file_view(self, x, fn: str, channel: Optional[int]):
        """x as a detection call takes it -> (the device tensor, many, the channel to pass).  An interleaved (n, ch >= 2) file stays as it
        is (many) and needs `channel`, an index or -1 for joint detection; anything else is the one-channel file, flattened to (n,) --
        (n, 3) packed 24-bit -- and passed without a channel, of which only 0 and -1 exist.  A ValueError names the caller `fn`."""
        x = torch.as_tensor(x)
        s24, sdim = InpaintingEngine._file_samples(x, fn)                  # packed 24-bit PCM: uint8 (n, 3) or (n, ch, 3), 24-bit steps
        many = sdim == 2 and x.shape[1] >= 2
        if many and channel is None:
            raise ValueError(f"{fn}: an (n, {x.shape[1]}) recording needs channel = an index, or -1 for joint detection")
        if not many and channel is not None and int(channel) not in (-1, 0):
            raise ValueError(f"{fn}: channel = {channel} of a one-channel recording")
        x = InpaintingEngine._file_on_device(x, self.device)               # only now: the refusals above need no device
        x = x.contiguous() if many else (x.reshape(-1, 3) if s24 else x.reshape(-1)).contiguous()
        return x, many, int(channel) if many else None

    @staticmethod
    def _window_half(fn: str, win, half, max_half: Optional[int] = None):
        """The window of a windowed detector, given as `half` or as `win` = 2 * half + 1 -> half; held to 0 .. max_half when that is given."""
        if (win is None) == (half is None):
            raise ValueError(f"{fn}: give the window as win = its odd length in samples, or as half = (win - 1) / 2, not both")
        if win is not None:
            if int(win) != win or int(win) < 1 or int(win) % 2 == 0:
                raise ValueError(f"{fn}: win = {win}: an odd number of samples, 2 * half + 1")
            half = (int(win) - 1) // 2
        if max_half is not None and (int(half) != half or not 0 <= int(half) <= max_half):
            raise ValueError(f"{fn}: half = {half} samples, outside 0 .. {max_half}")
        return half

    @staticmethod
    def _runs_found(fn: str, noun: str, runs, words: torch.Tensor, min_len, max_runs):
        """The one D2H copy of a detection call: `words` is the device count, or {the count, T's bits} -> (the rows that were found, T or
        None).  A ValueError names both numbers when more than max_runs runs of `noun` samples qualify."""
        host = words.cpu()
        total = int(host[0])
        T = float(host[1:].view(torch.float32)[0]) if host.numel() == 2 else None
        if total > int(max_runs):
            raise ValueError(f"{fn}: {total} runs of at least {int(min_len)} {noun} samples, more than max_runs = {int(max_runs)}")
        return (runs[:total] if runs is not None else torch.zeros(0, 2, dtype=torch.int32, device=words.device)), T

    def find_quiet_runs(self, x, threshold: float = 0.0, min_len: int = 1, max_runs: int = 65536, channel: Optional[int] = None) -> torch.Tensor:
        """x (n,) fp32 or int16 (tensor or array, host or device; a device view may start anywhere) -> device int32 (R, 2): every
        maximal run of samples with |x| <= threshold of at least min_len samples, as (start, len) rows sorted by start
        (si_quiet_runs).  One D2H copy: the count.  A ValueError names both numbers when more than max_runs runs qualify.
        An interleaved x (n, ch >= 2) needs `channel`: an index for that channel's runs, -1 for the runs of sample
        times at which every channel is quiet; rows are in sample times (si_quiet_runs_ch).  x is not flattened or de-interleaved.
        Packed 24-bit PCM: x uint8, (n, 3) or (n, ch, 3); threshold in 24-bit steps."""
        x, _, channel = InpaintingEngine._file_view(self, x, "find_quiet_runs", channel)
        runs, n_runs = self.ctx.quiet_runs(x, threshold, min_len, max_runs, channel=channel)
        return InpaintingEngine._runs_found("find_quiet_runs", "quiet", runs, n_runs, min_len, max_runs)[0]

    DEAD_KINDS = {"quiet": 1, "held": 2, "any": 3}                    # SI_DEAD_QUIET, SI_DEAD_HELD and both

    def find_dead_runs(self, x, kind: str = "any", threshold: float = 0.0, rel_threshold: float = 0.0, held_tol: float = 0.0, min_len: int = 1,
                       max_runs: int = 65536, channel: Optional[int] = None, return_threshold: bool = False):
        """find_quiet_runs for dropouts that are not digital silence (si_dead_runs): a sample is dead when it is
        quiet against T = max(threshold, rel_threshold * the peak of x) (kind "quiet"), when it is HELD -- within held_tol of a
        neighbour of its own channel -- (kind "held"), or either (kind "any").  x, channel, min_len, max_runs and the rows are
        find_quiet_runs'; threshold and held_tol are in x's own units, rel_threshold is a fraction of the peak in [0, 1].
        One D2H copy: the count, which with return_threshold=True also carries T; -> runs, or (runs, T)."""
        if kind not in self.DEAD_KINDS:
            raise ValueError(f"find_dead_runs: kind = {kind!r}: 'quiet', 'held' or 'any'")
        x, _, channel = InpaintingEngine._file_view(self, x, "find_dead_runs", channel)
        words = torch.zeros(2, dtype=torch.int32, device=self.device)      # {the count, T's bits}: one copy brings both
        runs, _ = self.ctx.dead_runs(x, self.DEAD_KINDS[kind], threshold, rel_threshold, held_tol, min_len, max_runs, n_runs=words[:1],
                                     channel=channel, threshold_out=words[1:].view(torch.float32))
        runs, T = InpaintingEngine._runs_found("find_dead_runs", "dead", runs, words, min_len, max_runs)
        return (runs, T) if return_threshold else runs

    def find_level_runs(self, x, win: Optional[int] = None, half: Optional[int] = None, threshold: float = 0.0, rel_threshold: float = 0.0,
                        min_len: int = 1, max_runs: int = 65536, channel: Optional[int] = None, return_threshold: bool = False):
        """find_dead_runs for a dropout that is a noise floor (si_level_runs): a sample is dead when a window of
        2 * half + 1 samples of its channel that reaches over it has an RMS level of at most T = max(threshold, rel_threshold * the
        peak of x), and no NaN or inf.  Give the window as `half`, or as `win` = its odd length in samples; half = 0 is the sample-wise
        "quiet".  x, channel, min_len, max_runs, threshold, rel_threshold and the rows are find_dead_runs'.
        One D2H copy: the count, which with return_threshold=True also carries T; -> runs, or (runs, T)."""
        half = InpaintingEngine._window_half("find_level_runs", win, half, G.LEVEL_MAX_HALF)
        x, _, channel = InpaintingEngine._file_view(self, x, "find_level_runs", channel)
        words = torch.zeros(2, dtype=torch.int32, device=self.device)      # {the count, T's bits}: one copy brings both
        runs, _ = self.ctx.level_runs(x, int(half), threshold, rel_threshold, min_len, max_runs, n_runs=words[:1],
                                      channel=channel, threshold_out=words[1:].view(torch.float32))
        runs, T = InpaintingEngine._runs_found("find_level_runs", "dead", runs, words, min_len, max_runs)
        return (runs, T) if return_threshold else runs

    def find_burst_runs(self, x, win: Optional[int] = None, half: Optional[int] = None, threshold: float = 0.0, rel_threshold: float = 0.0,
                        min_len: int = 1, max_runs: int = 65536, channel: Optional[int] = None, return_threshold: bool = False):
        """find_level_runs for damage that is LOUDER than the speech (si_burst_runs): a block of corrupted PCM --
        random data, swapped or misaligned bytes.  A sample is dead when a window of 2 * half + 1 second differences x[k - 1] -
        2 x[k] + x[k + 1] of its channel that reaches over it has an RMS level of at least T = max(threshold, rel_threshold * the peak
        of x), and no NaN or inf under it.  The window, x, channel, min_len, max_runs, threshold and the rows are find_level_runs';
        rel_threshold lies in [0, 4] (|d| <= 4 * peak).  T = 0 makes every window hot and is the caller's to refuse (find_gaps does).
        One D2H copy: the count, which with return_threshold=True also carries T; -> runs, or (runs, T)."""
        half = InpaintingEngine._window_half("find_burst_runs", win, half, G.LEVEL_MAX_HALF)
        if not 0.0 <= float(rel_threshold) <= 4.0:
            raise ValueError(f"find_burst_runs: rel_threshold = {rel_threshold} is NaN or outside [0, 4] (a second difference is at most 4 * the peak)")
        x, _, channel = InpaintingEngine._file_view(self, x, "find_burst_runs", channel)
        words = torch.zeros(2, dtype=torch.int32, device=self.device)      # {the count, T's bits}: one copy brings both
        runs, _ = self.ctx.burst_runs(x, int(half), threshold, rel_threshold, min_len, max_runs, n_runs=words[:1],
                                      channel=channel, threshold_out=words[1:].view(torch.float32))
        runs, T = InpaintingEngine._runs_found("find_burst_runs", "dead", runs, words, min_len, max_runs)
        return (runs, T) if return_threshold else runs

    def find_impulse_runs(self, x, win: Optional[int] = None, half: Optional[int] = None, order: int = 16, guard: int = 4, pad: int = 2,
                          ratio: float = 10.0, threshold: float = 0.0, rel_threshold: float = 0.0, min_len: int = 1, max_runs: int = 65536,
                          channel: Optional[int] = None, return_threshold: bool = False):
        """find_burst_runs for clicks and pops of one to a few IN-RANGE samples (si_impulse_runs).  The signal is whitened
        by an AR model of order `order` fitted per block of 512 samples (to the block and 256 samples on either side); a sample is HOT
        when its squared prediction error is above T^2, T = max(threshold, rel_threshold * the peak of x), and above ratio^2 times the
        mean squared prediction error of the samples within `half` of it, `guard` samples on either side left out; a sample is dead
        when a hot one lies within `pad` of it.  win = 2 * half + 1.  T = 0 (the default) is allowed: the ratio test remains.  x,
        channel, min_len, max_runs and the rows are find_level_runs'; rel_threshold lies in [0, 4].
        One D2H copy: the count, which with return_threshold=True also carries T; -> runs, or (runs, T)."""
        half = InpaintingEngine._window_half("find_impulse_runs", win, half)
        G.check_impulse("find_impulse_runs", order, half, guard, pad, ratio, rel_threshold)
        x, _, channel = InpaintingEngine._file_view(self, x, "find_impulse_runs", channel)
        words = torch.zeros(2, dtype=torch.int32, device=self.device)      # {the count, T's bits}: one copy brings both
        runs, _ = self.ctx.impulse_runs(x, int(order), int(half), int(guard), int(pad), ratio, threshold, rel_threshold, min_len, max_runs,
                                        n_runs=words[:1], channel=channel, threshold_out=words[1:].view(torch.float32))
        runs, T = InpaintingEngine._runs_found("find_impulse_runs", "dead", runs, words, min_len, max_runs)
        return (runs, T) if return_threshold else runs

    def impulse_residual(self, x, order: int = 16, channel: Optional[int] = None) -> torch.Tensor:
        """The whitened signal find_impulse_runs judges (si_impulse_residual): e(t) = sum_j a_j x[t - j] under the AR
        model of t's block, as a device float64 tensor (n,) -- 0.0 for t < order, NaN in a block whose fit window holds a NaN or an
        inf.  x is find_impulse_runs'; an (n, ch >= 2) file needs channel = an index."""
        if int(order) != order or not 2 <= int(order) <= native.IMPULSE_MAX_ORDER:
            raise ValueError(f"impulse_residual: order = {order}, outside 2 .. {native.IMPULSE_MAX_ORDER}")
        x = torch.as_tensor(x)
        s24, sdim = InpaintingEngine._file_samples(x, "impulse_residual")
        many = sdim == 2 and x.shape[1] >= 2
        if many and (channel is None or not 0 <= int(channel) < x.shape[1]):
            raise ValueError(f"impulse_residual: an (n, {x.shape[1]}) recording needs channel = an index in 0 .. {x.shape[1] - 1}")
        if not many and channel is not None and int(channel) != 0:
            raise ValueError(f"impulse_residual: channel = {channel} of a one-channel recording")
        x = InpaintingEngine._file_on_device(x, self.device)
        x = x.contiguous() if many else (x.reshape(-1, 3) if s24 else x.reshape(-1)).contiguous()
        return self.ctx.impulse_residual(x, int(order), channel=int(channel) if many else None)

    @staticmethod
    def _impulse_keywords(win_ms, order, guard, pad, ratio) -> Dict[str, object]:
        """What conceal_* hand find_gaps at kind "impulse" and at no other: the four impulse_* keywords, and win_ms when it was given."""
        kw = {"impulse_order": order, "impulse_guard": guard, "impulse_pad": pad, "impulse_ratio": ratio}
        if win_ms is not _WIN_MS:
            kw["win_ms"] = win_ms
        return kw

    def find_invalid_runs(self, x, ceiling: float = float("inf"), min_len: int = 1, max_runs: int = 65536,
                          channel: Optional[int] = None) -> torch.Tensor:
        """find_quiet_runs for a file whose damage is the sample VALUES (si_invalid_runs): every maximal run of at least
        min_len samples that are NaN (any payload, either sign), +-inf or of a magnitude above `ceiling`, as device int32 (R, 2) (start,
        len) rows sorted by start.  ceiling > 0 in x's own units, +inf (the default) = the non-finite samples; an int16 or packed
        24-bit sample is invalid only under a finite ceiling (32766 marks clipped int16 samples).  x, channel (an index, or -1: the
        times at which EVERY channel is invalid), min_len, max_runs, the one D2H copy (the count) and the ValueError on overflow are
        find_quiet_runs'."""
        c = float(ceiling)
        if not c > 0.0:
            raise ValueError(f"find_invalid_runs: ceiling = {ceiling} is not above 0, or is NaN (+inf, the samples that are not finite, is allowed)")
        x, _, channel = InpaintingEngine._file_view(self, x, "find_invalid_runs", channel)
        runs, n_runs = self.ctx.invalid_runs(x, c, min_len, max_runs, channel=channel)
        return InpaintingEngine._runs_found("find_invalid_runs", "invalid", runs, n_runs, min_len, max_runs)[0]

    # ---- short runs mended in place by least-squares AR interpolation
    @staticmethod
    def _mend_limits(fn: str, max_len, order, context) -> Tuple[int, int, int]:
        """(max_len, order, context) as integers inside si_mend_runs' limits, or a ValueError that names the fix."""
        max_len, order, context = int(max_len), int(order), int(context)
        if max_len > native.MEND_MAX_LEN:
            raise ValueError(f"{fn}: max_len = {max_len} samples, at most {native.MEND_MAX_LEN}: least-squares AR interpolation is no better than a "
                             f"straight line beyond that; leave longer runs to the inpainter (lower max_len / mend_ms)")
        if max_len < 1:
            raise ValueError(f"{fn}: max_len = {max_len} samples, at least 1")
        if not 2 <= order <= native.MEND_MAX_ORDER:
            raise ValueError(f"{fn}: order = {order}, outside 2 .. {native.MEND_MAX_ORDER}")
        if not 4 * order <= context <= native.MEND_MAX_CONTEXT:
            raise ValueError(f"{fn}: context = {context} samples, outside 4 * order = {4 * order} .. {native.MEND_MAX_CONTEXT}: "
                             f"raise context or lower order")
        return max_len, order, context

    def mend_runs(self, x, runs, max_len: int = 64, order: int = 32, context: int = 512, channel: Optional[int] = None,
                  inplace: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """The runs of at most max_len samples among `runs` filled from their own neighbourhood by least-squares AR interpolation
        (si_mend_runs): an AR model of order `order` fitted to `context` intact samples on either side of a run, then the
        samples that minimise its prediction error -- for a stray NaN, a 3-sample underrun or a clipped peak, which a generated 20 ms
        frame would repair at the cost of good speech.  x takes find_quiet_runs' rules: host or device, fp32 / int16 / packed 24-bit
        (uint8 (n, 3) or (n, ch, 3)), and an interleaved (n, ch >= 2) file needs `channel` (an index: the one channel that is read and
        written).  runs: the device tensor a find_*_runs call returned, or a host list of (start, len) rows, which is checked here to be
        sorted, disjoint and inside the file (a ValueError names the row).
        -> (y, status): y is a device copy of x with the mended samples (x itself with inplace=True, which needs a device tensor in
        the sample type it is read in); status is device int32 (R,), native.MEND_* per row.  Only MEND_AR and MEND_LINE rows were
        written, and only their own samples: everything else holds x's bits."""
        max_len, order, context = self._mend_limits("mend_runs", max_len, order, context)
        x = torch.as_tensor(x)
        s24, sdim = InpaintingEngine._file_samples(x, "mend_runs")
        many = sdim == 2 and x.shape[1] >= 2
        if many and (channel is None or int(channel) < 0):
            raise ValueError(f"mend_runs: an (n, {x.shape[1]}) recording needs channel = an index (one channel is mended per call)")
        if not many and channel is not None and int(channel) != 0:
            raise ValueError(f"mend_runs: channel = {channel} of a one-channel recording")
        n = x.shape[0] if (sdim == 2 or s24) else x.numel()
        if inplace:
            if not x.is_cuda or x.dtype not in (torch.float32, torch.int16, torch.uint8) or not x.is_contiguous():
                raise ValueError("mend_runs: inplace = True needs a contiguous device tensor of fp32, int16 or packed 24-bit samples (a host input or "
                                 "another dtype is copied: pass inplace = False and use the returned y)")
            y = x
        else:
            y = InpaintingEngine._file_on_device(x, self.device)
            y = y.clone() if y.data_ptr() == x.data_ptr() else y
        shape = y.shape
        flat = y.contiguous() if many else (y.reshape(-1, 3) if s24 else y.reshape(-1)).contiguous()
        assert not inplace or flat.data_ptr() == y.data_ptr()
        if not torch.is_tensor(runs):
            rows = [(int(r[0]), int(r[1])) for r in runs]
            end = 0
            for i, (s, m) in enumerate(rows):
                if m < 1 or s < 0 or s + m > n:
                    raise ValueError(f"mend_runs: row {i} = (start {s}, len {m}) is empty or outside the file's {n} samples")
                if s < end:
                    raise ValueError(f"mend_runs: row {i} = (start {s}, len {m}) starts before row {i - 1} ends at {end}: rows are sorted and disjoint")
                end = s + m
            runs = torch.tensor(rows, dtype=torch.int32).reshape(-1, 2).to(self.device)
        runs = runs.to(self.device, torch.int32).reshape(-1, 2).contiguous()
        if runs.shape[0] > native.MEND_MAX_RUNS:
            raise ValueError(f"mend_runs: {runs.shape[0]} rows, at most {native.MEND_MAX_RUNS} in one call")
        status = self.ctx.mend_runs(flat, runs, max_len, order, context, channel=int(channel) if many else None)
        return flat.reshape(shape), status

    def recording_frames(self, n22: int, clip_frames: int = 200, n16: Optional[int] = None) -> Tuple[int, int]:
        """(n_rec_frames, lim_frames) of a recording of n22 samples at 22.05 kHz as patch_recording serves it: its 20 ms frames and
        the usable ones [0, lim) -- a context clip's min(T, Tm) (patch_recording's own arithmetic, n16 = the samples of a supplied
        16 kHz recording), counted from frame n_rec - clip_frames, where the last context starts, when there is more than one clip."""
        n22, clip_frames = int(n22), int(clip_frames)
        n_rec = n22 // 441
        whole = n_rec <= clip_frames
        L22 = n22 if whole else clip_frames * 441
        L16 = (int(n16) if whole else clip_frames * 320) if n16 is not None else -(-L22 * 16000 // 22050)
        lim = min(self.ctx.num_frames(L16), self.ctx.mel_frames(L22)) if L16 > 0 and L22 > 0 else 0
        return n_rec, max(lim, 0) + (0 if whole else n_rec - clip_frames)

    def find_gaps(self, x, sr: int = 22050, threshold: float = 0.0, min_ms: float = 5.0, max_ms: float = 400.0, pad_frames: int = 0,
                  merge_frames: Optional[int] = None, fade: int = 110, n_rec_frames: Optional[int] = None,
                  lim_frames: Optional[int] = None, channel: Optional[int] = None, kind: str = "quiet", rel_threshold: float = 0.0,
                  held_tol: float = 0.0, win_ms: float = _WIN_MS, impulse_order: int = 16, impulse_guard: int = 4, impulse_pad: int = 2,
                  impulse_ratio: float = 10.0) -> Dict[str, object]:
        """The dropouts of a recording x (n samples at `sr` Hz, fp32 in full-scale units, int16 PCM or packed 24-bit PCM): runs of at least min_ms of
        |x| <= threshold (find_quiet_runs), mapped by gaps.runs_to_gaps onto the 20 ms grid of the recording's n_rec_frames frames
        (default n * 50 // sr) with the usable frames [0, lim_frames).  merge_frames None = 2 * the frames one cross-fade of `fade`
        22.05 kHz samples reaches over; gaps of more than max_ms are skipped.
        -> gaps ((first frame, frame count), sorted: what patch_recording takes), skipped ((first frame, frame count, reason)),
        runs (device int32 (R, 2), samples at `sr`).
        An interleaved x (n, ch) takes find_quiet_runs' `channel`; n, the runs and the gaps then count sample times and frames.
        kind, rel_threshold, held_tol: find_dead_runs' (DESIGN.md 4.20).  At their defaults the runs are find_quiet_runs', the same
        launches; anything else goes to find_dead_runs, and the dictionary gains `threshold`: the effective one, T.
        kind "level" (DESIGN.md 4.25): the runs are find_level_runs' -- the RMS level of a window of win_ms milliseconds, half =
        round(win_ms * sr / 2000) samples on each side, against the threshold -- and the dictionary carries `threshold` as well.
        held_tol has no meaning there and must be 0.
        kind "burst" (DESIGN.md 4.28): the runs are find_burst_runs' -- a block of corrupted PCM, LOUDER than the speech: the RMS level of
        the second difference over a window of win_ms milliseconds at or above the threshold.  rel_threshold may reach 4 there, held_tol
        must be 0, and T = 0 (both thresholds 0) is refused: start from 1.15 of full scale with win_ms = 4.0.  `threshold` is carried
        as well.  win_ms is read at no other kind.
        kind "invalid" (DESIGN.md 4.30): the runs are find_invalid_runs' -- samples that are NaN, +-inf or, with threshold != 0, of a
        magnitude above `threshold`, the CEILING in x's own units (threshold = 0, the default, is +inf: the non-finite samples only).
        rel_threshold and held_tol must be 0; win_ms is not read.  min_ms keeps its meaning and its default: pass min_ms=0 for this
        kind, a single NaN is a run of one sample.  `threshold` carries the ceiling.
        kind "impulse" (DESIGN.md 4.33): the runs are find_impulse_runs' -- clicks and pops of one to a few IN-RANGE samples: a sample
        whose squared AR(impulse_order) prediction error stands impulse_ratio^2 over the mean squared prediction error of the samples
        within win_ms / 2 of it (23 ms when win_ms is not given, half = round(win_ms * sr / 2000)), impulse_guard samples on either side
        left out, widened by impulse_pad samples.  threshold / rel_threshold set a floor T under the prediction error (0: none);
        held_tol must be 0.  min_ms keeps its meaning and its default: pass min_ms=0 for this kind, or nearly every click is dropped.
        The impulse_* keywords are read at no other kind.  `threshold` carries T.  The defaults were chosen on 22.05 kHz int16 speech;
        other rates, fp32 material and music are unmeasured."""
        impulse = kind == "impulse"
        if win_ms is _WIN_MS:                                          # not given: 2 ms, as ever; 23 ms at kind "impulse"
            win_ms = G.IMPULSE_DEFAULTS["win_ms"] if impulse else 2.0
        x = torch.as_tensor(x)
        s24, sdim = InpaintingEngine._file_samples(x, "find_gaps")                 # packed 24-bit PCM: thresholds in 24-bit steps
        n, sr = (x.shape[0] if sdim == 2 or s24 else x.numel()), int(sr)
        if n < 1 or sr <= 0:
            raise ValueError(f"find_gaps: {n} samples at {sr} Hz")
        min_len, T = max(1, int(round(float(min_ms) * sr / 1000.0))), None
        if kind == "level":
            if float(held_tol) != 0.0:
                raise ValueError(f"find_gaps: held_tol = {held_tol} with kind = 'level' (held samples are kind 'held' or 'any')")
            runs, T = self.find_level_runs(x, half=G.level_half(win_ms, sr), threshold=threshold, rel_threshold=rel_threshold, min_len=min_len,
                                           channel=channel, return_threshold=True)
        elif kind == "burst":
            if float(held_tol) != 0.0:
                raise ValueError(f"find_gaps: held_tol = {held_tol} with kind = 'burst' (held samples are kind 'held' or 'any')")
            if not 0.0 <= float(rel_threshold) <= 4.0:
                raise ValueError(f"find_gaps: rel_threshold = {rel_threshold} with kind = 'burst' is NaN or outside [0, 4] (a second difference "
                                 f"is at most 4 * the peak)")
            if float(threshold) == 0.0 and float(rel_threshold) == 0.0:
                raise ValueError("find_gaps: kind = 'burst' with threshold = 0 and rel_threshold = 0 is T = 0: every window would be hot.  "
                                 "Start from threshold = 1.15 of full scale (1.15 * 32768 for int16, 1.15 * 2^23 for 24-bit) with win_ms = 4.0")
            runs, T = self.find_burst_runs(x, half=G.level_half(win_ms, sr), threshold=threshold, rel_threshold=rel_threshold, min_len=min_len,
                                           channel=channel, return_threshold=True)
        elif impulse:
            if float(held_tol) != 0.0:
                raise ValueError(f"find_gaps: held_tol = {held_tol} with kind = 'impulse' (held samples are kind 'held' or 'any')")
            half = G.level_half(win_ms, sr)
            G.check_impulse("find_gaps", impulse_order, half, impulse_guard, impulse_pad, impulse_ratio, rel_threshold, win_ms=win_ms, sr=sr)
            runs, T = self.find_impulse_runs(x, half=half, order=impulse_order, guard=impulse_guard, pad=impulse_pad, ratio=impulse_ratio,
                                             threshold=threshold, rel_threshold=rel_threshold, min_len=min_len, channel=channel,
                                             return_threshold=True)
        elif kind == "invalid":
            if float(rel_threshold) != 0.0:
                raise ValueError(f"find_gaps: rel_threshold = {rel_threshold} with kind = 'invalid' (the ceiling is `threshold`, in the file's own units; "
                                 f"nothing here follows the peak)")
            if float(held_tol) != 0.0:
                raise ValueError(f"find_gaps: held_tol = {held_tol} with kind = 'invalid' (held samples are kind 'held' or 'any')")
            T = G.invalid_ceiling(threshold)
            runs = self.find_invalid_runs(x, ceiling=T, min_len=min_len, channel=channel)
        elif kind == "quiet" and float(rel_threshold) == 0.0 and float(held_tol) == 0.0:
            runs = self.find_quiet_runs(x, threshold, min_len, channel=channel)
        else:
            runs, T = self.find_dead_runs(x, kind, threshold, rel_threshold, held_tol, min_len, channel=channel, return_threshold=True)
        n_rec = n * 50 // sr if n_rec_frames is None else int(n_rec_frames)
        mf = 2 * max(-(-int(fade) // 441), 1) if merge_frames is None else int(merge_frames)
        gaps, skipped = G.runs_to_gaps(runs.tolist(), n, sr, n_rec, lim_frames, pad_frames, mf, max(int(float(max_ms) // 20), 1))
        return {"gaps": gaps, "skipped": skipped, "runs": runs} if T is None else {"gaps": gaps, "skipped": skipped, "runs": runs, "threshold": T}

    def conceal_recording(self, wave22, wave16=None, detect_on=None, sr: int = 22050, threshold: float = 0.0, min_ms: float = 5.0,
                          max_ms: float = 400.0, pad_frames: int = 0, merge_frames: Optional[int] = None, fade: int = 110,
                          clip_frames: int = 200, min_context: int = 50, batch: int = 32, pcm: bool = False, kind: str = "quiet",
                          rel_threshold: float = 0.0, held_tol: float = 0.0, win_ms: float = _WIN_MS, impulse_order: int = 16,
                          impulse_guard: int = 4, impulse_pad: int = 2, impulse_ratio: float = 10.0) -> Dict[str, object]:
        """File in, repaired file out: find_gaps, then patch_recording unchanged with the gaps it found.  Detection runs on detect_on
        when given -- the file's own samples at `sr` Hz, where a dropout is still exact zeros -- else on wave22 (sr is 22050 then).
        The usable frames are patch_recording's own (its last context's min(T, Tm)), and a gap longer than the planner's budget
        clip_frames - 2 * min_context counts as long whatever max_ms says.
        kind, rel_threshold, held_tol: find_gaps' (held samples, a threshold relative to the peak).
        kind "level" with win_ms: find_gaps' too (a noise-floor dropout, by windowed RMS level).
        kind "burst" with win_ms: find_gaps' too (a block of corrupted PCM, by second-difference level).
        kind "invalid": find_gaps' too (NaN, +-inf, |x| > threshold when threshold != 0) -- pass min_ms=0.  The ceiling
        goes on to patch_recording(ceiling=...); detect_on is refused, because the samples that are fed must be the ones that were judged.
        kind "impulse" with win_ms and impulse_*: find_gaps' too (clicks and pops) -- pass min_ms=0.  Nothing is mended
        here: every click costs a generated frame (conceal_file has mend_ms).
        -> patch_recording's dictionary + gaps + skipped [+ threshold].  With nothing found: an exact copy; only the detection kernels launched."""
        if kind == "invalid" and detect_on is not None:
            raise ValueError("conceal_recording: kind = 'invalid' with detect_on: the samples that are fed to the model (wave22) must be the ones "
                             "that were judged; for a file at its own rate use conceal_file(kind='invalid', feed='contexts')")
        as1d = lambda x: torch.as_tensor(x).to(self.device, torch.float32).reshape(-1).contiguous()
        wave22 = as1d(wave22)
        wave16 = None if wave16 is None else as1d(wave16)
        clip_frames, min_context = int(clip_frames), int(min_context)
        n_rec, lim = self.recording_frames(wave22.numel(), clip_frames, None if wave16 is None else wave16.numel())
        if n_rec > clip_frames:
            max_ms = min(float(max_ms), 20.0 * (clip_frames - 2 * min_context))
        found = self.find_gaps(wave22 if detect_on is None else detect_on, 22050 if detect_on is None else sr, threshold, min_ms, max_ms,
                               pad_frames, merge_frames, fade, n_rec, lim, kind=kind, rel_threshold=rel_threshold, held_tol=held_tol,
                               **({"win_ms": win_ms} if kind in ("level", "burst") else {}),
                               **(self._impulse_keywords(win_ms, impulse_order, impulse_guard, impulse_pad, impulse_ratio) if kind == "impulse" else {}))
        kc = {"ceiling": G.invalid_ceiling(threshold)} if kind == "invalid" else {}      # no other kind hands patch_recording a new keyword
        out = self.patch_recording(wave22, found["gaps"], wave16=wave16, fade=fade, clip_frames=clip_frames, min_context=min_context,
                                   batch=batch, pcm=pcm, **kc)
        out["gaps"], out["skipped"] = found["gaps"], found["skipped"]
        if "threshold" in found:
            out["threshold"] = found["threshold"]
        return out

    def predict_multigap_batch(self, wave16: torch.Tensor, mel_or_wave22: torch.Tensor, gaps, len16: Optional[Sequence[int]] = None,
                               len22: Optional[Sequence[int]] = None, mel_len: Optional[Sequence[int]] = None,
                               spans22: Optional[Sequence[Sequence[Sequence[int]]]] = None, tables: Optional[Dict[str, object]] = None,
                               vocode: bool = True) -> Dict[str, object]:
        """`predict_batch` with 0 .. MAX_SPANS gaps per clip, different per clip, in ONE pass: all gaps are zeroed before the one
        encoder pass, all masked frames are decided and spliced by one launch, and the vocoder runs once.
        wave16 (B, N) raw 16 kHz clips; mel_or_wave22: the (B, 80, Tm) log-mel of the masked 22.05 kHz clips, or the RAW (B, N22)
        22.05 kHz clips, which are then masked (the gaps' spans by I_ea/predict.py:99-100, or `spans22[b]` = [start, end) sample
        pairs per gap) and turned into the mel here.  gaps[b] = (first 20 ms frame, frame count) pairs, any order; overlapping gaps,
        empty ones and gaps outside the clip's min(T, Tm) frames raise a ValueError naming clip and gap.
        len16 (+ len22 for raw clips / mel_len for a mel): host lengths of a RAGGED batch; every clip then equals itself alone.
        tables: what `gap_tables` returned for these gaps and lengths (a caller that staged them itself); `gaps` / `spans22` are
        then not read.  vocode=False leaves the generator pass to the caller (no `wave`).
        -> feats (B, T, 80), labels (F,) flat over clips then gaps then frames, label_off (B + 1) (clip b's labels =
        labels[label_off[b]:label_off[b + 1]]), mel (the spliced mel), mel_masked, wave, gaps (sorted) [+ wave_len, frames, mel_len]."""
        self._need(head=True, codebook=True, what="predict_multigap_batch")
        B = wave16.shape[0]
        raw22 = mel_or_wave22.dim() == 2
        ragged = len16 is not None
        n16 = [int(n) for n in len16] if ragged else [wave16.shape[1]] * B
        if raw22:
            n22 = [int(n) for n in len22] if len22 is not None else [mel_or_wave22.shape[1]] * B
            if ragged and len22 is None:
                raise ValueError("predict_multigap_batch: a ragged batch of raw 22.05 kHz clips needs len22")
            tb = tables if tables is not None else self.gap_tables(gaps, n16, n22, spans22=spans22)
            if tb["tab22"] is None:
                raise ValueError("predict_multigap_batch: raw 22.05 kHz clips need tables with the 22.05 kHz spans")
            mel = self.mel_ragged(mel_or_wave22, n22, spans=tb["tab22"]) if ragged else self.mel(mel_or_wave22, spans=tb["tab22"])
            mlen = [self.ctx.mel_frames(n) for n in n22]
        else:
            mel = mel_or_wave22
            mlen = [int(m) for m in mel_len] if mel_len is not None else [mel.shape[2]] * B
            if ragged and mel_len is None:
                raise ValueError("predict_multigap_batch: a ragged batch with a mel needs mel_len")
            tb = tables if tables is not None else self.gap_tables(gaps, n16, mlen, mel_frames=True)
        feats = self.encode_ragged(wave16, n16, spans=tb["tab16"]) if ragged else self.encode(wave16, spans=tb["tab16"])
        mel2 = mel.clone()
        labels = self.splice_spans(feats, tb["frame_clip"], tb["frame_pos"], mel2)
        out = {"feats": feats, "labels": labels, "label_off": tb["label_off"], "mel": mel2, "mel_masked": mel, "gaps": tb["gaps"],
               "frame_clip": tb["frame_clip"], "frame_pos": tb["frame_pos"]}
        if ragged:
            out.update(frames=[self.ctx.num_frames(n) for n in n16], mel_len=mlen,
                       wave_len=[self.ctx.vocoder_samples(m, True) for m in mlen])
        if vocode:
            out["wave"] = self.vocode_ragged(mel2, mlen, stretch=True) if ragged else self.vocode(mel2, stretch=True)
        return out

    def predict_batch(self, wave16: torch.Tensor, mel: torch.Tensor, frame_pos: torch.Tensor, frame_len: int,
                      blind: bool = False, mask_start: Optional[torch.Tensor] = None,
                      mask_len: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """wave16 (B, N) raw 16 kHz clips, mel (B, 80, Tm) log-mel of the masked 22.05 kHz clips, frame_pos (B,) int32
        first masked 20 ms frame, frame_len = Lm.  All tensors on this engine's GPU.  `mel` is not modified.
        blind=True replaces every frame (mask position unknown)."""
        self._need(head=True, codebook=True, what="predict_batch")
        B = wave16.shape[0]
        if blind:
            feats = self.encode(wave16, None, None)
            pos = torch.zeros(B, dtype=torch.int32, device=self.device)
            lm = min(feats.shape[1], mel.shape[2])
        else:
            if mask_start is None:
                mask_start = frame_pos * 320 + 80                                   # predict.py:133
                mask_len = torch.full_like(frame_pos, max(frame_len * 320 - 81, 0))
            feats = self.encode(wave16, mask_start.to(torch.int32), mask_len.to(torch.int32))
            pos, lm = frame_pos, frame_len
        mel2 = mel.clone()
        labels = self.splice(feats, pos, lm, mel2)
        wav = self.vocode(mel2, stretch=True)
        return {"feats": feats, "labels": labels, "mel": mel2, "wave": wav}


# ------------------------------------------------------------------------------------------------------------------
# Drop-in module wrappers (same call signatures as the reference's nn.Modules)
# ------------------------------------------------------------------------------------------------------------------
class CustomModel:
    """`CustomModel.forward(input_values, attention_mask)` (I_ea/model.py:80-89): processor-normalised input_values (B, N)
    -> (B, T, codebook_dim).  attention_mask (B, N) 0/1 marks the real samples of a RIGHT-PADDED batch (what the HF
    processor emits with padding=True): the padded frames are zeroed after the projection and excluded as attention
    keys, as modeling_hubert.py:921-932,428-437 does; the output is defined on all T frames, like the reference's."""

    def __init__(self, engine: InpaintingEngine):
        self.engine = engine

    def eval(self):
        return self

    def to(self, device):
        if torch.device(device) != self.engine.device:
            raise RuntimeError("the engine is bound to its GPU at construction")
        return self

    def __call__(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = input_values.to(self.engine.device, torch.float32).contiguous()
        valid = None
        if attention_mask is not None:
            m = attention_mask.to(self.engine.device).bool()
            if not bool(m.all()):
                if m.shape != x.shape or bool((m[:, 1:] & ~m[:, :-1]).any()):
                    raise ValueError("attention_mask must be (B, N) and right-padded (ones, then zeros), as the HF processor emits it")
                valid = m.sum(-1).to(torch.int32).contiguous()
        return self.engine.encode(x, None, None, normalize=False, valid_len=valid)

    forward = __call__


class Generator:
    """`Generator.forward` (I_ea/hifi_gan/models.py:107-123): feats (B, 80, T') -> (B, 1, T' * hop)."""

    def __init__(self, engine: InpaintingEngine):
        self.engine = engine

    def eval(self):
        return self

    def remove_weight_norm(self):
        return None            # folded at load (api.hip)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(self.engine.device, torch.float32).contiguous()
        return self.engine.vocode(x, stretch=False).unsqueeze(1)

    forward = __call__


class LossFunction:
    """`LossFunction` of I_ea/loss_fn.py over the engine's resident codebook: `cos_sim` (loss + arg-max labels, :29-47),
    `cos_sim_target_labels` (:49-62), plus the centroid splice that follows the call in the script
    (I_ea/predict.py:184-187)."""

    def __init__(self, engine: InpaintingEngine):
        self.engine = engine
        self._last = None

    def cos_sim(self, output: torch.Tensor, labels: torch.Tensor):
        """output (B, Lm, 80) gathered frames, labels (B, Lm) int64 -> (loss scalar tensor, pred_labels (B, Lm)),
        as I_ea/loss_fn.py:29-47 (called at I_ea/predict.py:171)."""
        dev = self.engine.device
        self.engine._need(codebook=True, what="LossFunction.cos_sim")
        out = output.to(dev, torch.float32).contiguous()
        lab = labels.to(dev, torch.int64).contiguous()
        pos = torch.zeros(out.shape[0], dtype=torch.int32, device=dev)
        loss, terms, pred, cpt = self.engine.ctx.codebook_metrics(out, pos, out.shape[1], lab)
        self._last = (pred, lab, cpt)
        return loss[0], pred

    def cos_sim_target_labels(self, pred_labels: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """cos(centred predicted centroid, centred target centroid) per frame, flattened (I_ea/loss_fn.py:49-62).
        Served from the `cos_sim` call that produced `pred_labels` (the script always calls the two back to back,
        I_ea/predict.py:171-173); any other label pair is an error rather than a silent host computation."""
        if self._last is None or not (torch.equal(self._last[0], pred_labels.to(self._last[0].device)) and
                                      torch.equal(self._last[1], labels.to(self._last[1].device))):
            raise ValueError("cos_sim_target_labels expects the (pred_labels, labels) pair of the preceding cos_sim call")
        return self._last[2].reshape(-1)

    def predict_and_splice(self, outputs: torch.Tensor, mask_pos: torch.Tensor, mask_len: int, mel: torch.Tensor):
        """outputs (B, T, 80), mask_pos (B,) int32, mel (B, 80, Tm) modified in place -> labels (B, Lm)."""
        return self.engine.splice(outputs.contiguous(), mask_pos.to(self.engine.device, torch.int32).contiguous(),
                                  int(mask_len), mel)


class CodeGenerator:
    """`CodeGenerator.forward` of I_da/src/model.py:124-189 in its look-up-table configuration (hubert_lut.json: content
    units + quantised F0 + speaker embedding -> 384 channels -> the unit HiFi-GAN, upsample rates 5, 4, 4, 2, 2): the
    embedding / `_upsample` / concat front is si_unit_frontend, the generator is the engine's (a VocoderArch with
    num_mels = 3 * embedding_dim).  `emb_c` / `emb_p` are the checkpoint's `emb_c.weight` / `emb_p.weight` tables.
    The reference quantises F0 with its fixed VQ-VAE inside forward (:160-166): pass `f0_quantizer=F0Quantizer(engine,
    fo_vqvae_state)` and call with `f0=`; or pass the indices directly as `f0_code=`."""

    def __init__(self, engine: InpaintingEngine, emb_c: torch.Tensor, emb_p: Optional[torch.Tensor] = None,
                 f0_quantizer: Optional["F0Quantizer"] = None):
        self.engine = engine
        dev = engine.device
        self.emb_c = emb_c.to(dev, torch.float32).contiguous()
        self.emb_p = None if emb_p is None else emb_p.to(dev, torch.float32).contiguous()
        self.f0_quantizer = f0_quantizer                               # `self.fo_vqvae` of the reference (:63-71)

    def eval(self):
        return self

    def remove_weight_norm(self):
        return None

    def __call__(self, **kwargs) -> torch.Tensor:
        """code (B, Frame) int64; f0 (B, 1, Frame_f0) fp32 as in the reference (quantised here by the fixed F0 VQ-VAE when
        the generator was built with an `F0Quantizer`) or f0_code (B, Frame_p) int64 directly; emb (B, Emb) speaker
        embedding (optional) -> (B, 1, Frame * hop) waveform."""
        dev = self.engine.device
        code = kwargs["code"].to(dev, torch.int64).contiguous()
        f0c = kwargs.get("f0_code")
        if f0c is None and kwargs.get("f0") is not None:
            if self.f0_quantizer is None:
                raise ValueError("CodeGenerator: an F0 track needs the F0 VQ-VAE (pass f0_quantizer=F0Quantizer(...)) or f0_code")
            f0c = self.f0_quantizer(kwargs["f0"])
        emb = kwargs.get("emb")
        x = self.engine.ctx.unit_frontend(code, self.emb_c,
                                          None if f0c is None else f0c.to(dev, torch.int64).contiguous(), self.emb_p,
                                          None if emb is None else emb.to(dev, torch.float32).contiguous())
        return self.engine.vocode(x, stretch=False).unsqueeze(1)

    forward = __call__


class F0Quantizer:
    """The fixed F0 VQ-VAE front that `CodeGenerator.forward` runs on the F0 track (I_da/src/model.py:160-163):
    `z_p = fo_vqvae.vq(fo_vqvae.encoder(fo))[0][0]` -- jukebox.py `Encoder` (one level) on the GPU (si_f0_encoder_forward),
    then the bottleneck's nearest-codebook arg-min (vq.py:117-127; si_kmeans_assign).  `state` is the `FoVQVAE`
    state dict (`encoder.level_blocks.0.model...`, `vq.level_blocks.0.k`)."""

    def __init__(self, engine: InpaintingEngine, state: dict, desc: Optional["native.F0EncDesc"] = None):
        from . import native
        self.engine = engine
        self.desc = desc or native.F0EncDesc()
        dev = engine.device
        self.weights = pack_f0_encoder(state, self.desc).to(dev)
        self.codebook = state["vq.level_blocks.0.k"].to(dev, torch.float32).contiguous()

    def features(self, f0: torch.Tensor) -> torch.Tensor:
        """f0 (B, 1, T) -> (B, T', 128) encoder output, channels-last."""
        return self.engine.ctx.f0_encoder(self.desc, self.weights, f0.to(self.engine.device, torch.float32).contiguous())

    def codes(self, h: torch.Tensor) -> torch.Tensor:
        """encoder output (B, T', 128) -> z_p (B, T') int64: the bottleneck's nearest-codebook arg-min (vq.py:117-127)."""
        B, Tp, E = h.shape
        return self.engine.ctx.kmeans_assign(h.reshape(B * Tp, E), self.codebook).reshape(B, Tp)

    def __call__(self, f0: torch.Tensor) -> torch.Tensor:
        """f0 (B, 1, T) -> z_p (B, T') int64, the indices `emb_p` is looked up with."""
        return self.codes(self.features(f0))


def pack_f0_encoder(state: dict, desc) -> torch.Tensor:
    """Flatten the encoder's parameters in module order (the order si_f0_encoder_forward consumes them):
    `encoder.level_blocks.0.model.<i>.0` = strided conv, `.model.<i>.1.model.<j>.model.1` / `.model.3` = the res block's
    k3 / k1 convs (resnet.py:37-42), `.model.<down_t>` = the last conv (jukebox.py:80-82)."""
    pre = "encoder.level_blocks.0.model."
    parts = []
    for i in range(desc.down_t):
        parts += [state[f"{pre}{i}.0.weight"], state[f"{pre}{i}.0.bias"]]
        for j in range(desc.depth):
            r = f"{pre}{i}.1.model.{j}.model."
            parts += [state[r + "1.weight"], state[r + "1.bias"], state[r + "3.weight"], state[r + "3.bias"]]
    parts += [state[f"{pre}{desc.down_t}.weight"], state[f"{pre}{desc.down_t}.bias"]]
    return torch.cat([p.detach().to(torch.float32).reshape(-1) for p in parts]).contiguous()


class Metrics:
    """The signal metrics of `Metrics` (I_ea/metrics.py:12-142) on the GPU: `avg_cosine_sim`, `avg_d2_dist`, `rmse` on mel
    segments (80, L) and `sisdr` on waveforms, same names and argument order.  The Whisper WER/CER and PESQ/STOI members
    are third-party CPU code outside the hot path and are not provided.  `centroids` is what the
    reference passes to the constructor: the (80,) codebook mean that `avg_cosine_sim` subtracts."""

    def __init__(self, engine: InpaintingEngine, centroids: torch.Tensor):
        self.engine = engine
        self.center = centroids.reshape(-1).to(engine.device, torch.float32).contiguous()

    def _pair(self, t1, t2):
        dev = self.engine.device
        return t1.to(dev, torch.float32).contiguous()[None], t2.to(dev, torch.float32).contiguous()[None]

    def avg_cosine_sim(self, tensor1: torch.Tensor, tensor2: torch.Tensor) -> torch.Tensor:
        a, b = self._pair(tensor1, tensor2)
        return self.engine.ctx.mel_metrics(a, b, self.center)[0, 0]

    def avg_d2_dist(self, tensor1: torch.Tensor, tensor2: torch.Tensor) -> torch.Tensor:
        a, b = self._pair(tensor1, tensor2)
        return self.engine.ctx.mel_metrics(a, b, None)[0, 1]

    def rmse(self, tensor1: torch.Tensor, tensor2: torch.Tensor) -> torch.Tensor:
        a, b = self._pair(tensor1, tensor2)
        return self.engine.ctx.mel_metrics(a, b, None)[0, 2]

    def sisdr(self, x_est, x_ref) -> float:
        dev = self.engine.device
        e = torch.as_tensor(x_est, dtype=torch.float32).reshape(1, -1).to(dev).contiguous()
        r = torch.as_tensor(x_ref, dtype=torch.float32).reshape(1, -1).to(dev).contiguous()
        return float(self.engine.ctx.sisdr(e, r)[0])
