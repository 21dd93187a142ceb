"""predict.yaml / config.yaml schema of the reference (I_ea/predict.yaml:1-60, I_ea/config.yaml:1-76).

Only the keys the predict script reads are interpreted (I_ea/predict.py:60-73,85-89,109,144-146,158-159); unknown keys
are ignored, so both shipped files load.  An optional `bench:` / `batch:` block may be added by users of this package.
Keys of this package's own: `masks:`, `patch:`, `long:` and `detect:` (see PredictConfig).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Optional, Union

import torch
import yaml

from . import gaps as G


class AttrDict(dict):
    """dict with attribute access (I_ea/hifi_gan/env.py:5-11)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def choose_device(idx: Union[int, str]) -> torch.device:
    """I_ea/utils.py:6-30: 'cpu' -> cpu; int -> that GPU, clamped to the last one; no GPU -> cpu.
    (The inpainting engine itself refuses a CPU device: there is no CPU path in this package.)"""
    if idx == "cpu":
        return torch.device("cpu")
    if torch.cuda.is_available():
        n = torch.cuda.device_count()
        if n < int(idx) + 1:
            return torch.device(f"cuda:{n - 1}")
        return torch.device(f"cuda:{int(idx)}")
    return torch.device("cpu")


@dataclass
class PredictConfig:
    dataset: str
    wave_path: str
    save_pred: str
    n_clusters: int
    km_model_path: str            # .../km_model_<K>/model.km
    path2centroids: str
    device_index: Union[int, str]
    mask_start_sec: float
    mask_end_sec: float
    hifigan_checkpoint: str
    hifigan_config: str           # config.json beside the checkpoint (I_ea/predict.py:110-111)
    hubert_type: str
    hubert_checkpoint: str
    asr_model_name: Optional[str] = None
    raw: Optional[dict] = None
    masks: Optional[list] = None  # optional `masks:` list of (start_pos_in_sec, end_pos_in_sec): several gaps in the one file
    patch_fade_ms: Optional[float] = None   # optional `patch:` mapping ({fade_ms: 5}): also write patched.wav (the recording with
                                            # only the gaps filled); None without the key
    long: Optional[dict] = None   # optional `long:` mapping ({clip_s: 4.0, context_s: 1.0, batch: 32}): the file is a recording of any
                                  # length, served as context clips (engine.patch_recording); None without the key
    long_rate: object = 22050     # `rate:` inside `long:`: 22050 (default: patched.wav is the recording resampled to 22.05 kHz) or "file"
                                  # (patched.wav keeps the file's own rate and sample type: engine.patch_file)
    long_feed: str = "recording"  # `feed:` inside `long:` (needs rate: file): "recording" (default: the whole file is resampled to 22.05 kHz
                                  # to feed the model) or "contexts" (only the context clips are, straight from the file: DESIGN.md 4.17)
    long_clips16: str = "resampled"   # `clips16:` inside `long:` (needs feed: contexts): "resampled" (default: the encoder's 16 kHz clips are
                                      # the cut 22.05 kHz clips resampled) or "file" (they too are cut straight from the file: DESIGN.md 4.26)
    long_pcm24: str = "float32"   # `pcm24:` inside `long:` (needs rate: file and feed: contexts): "float32" (default: a 24-bit PCM file is read
                                  # to float32 and written as float32, as before the key existed) or "keep" (its packed bytes go to the engine
                                  # and the three files are written 24-bit: DESIGN.md 4.27); a file that is not 24-bit PCM ignores it
    detect: Optional[dict] = None  # optional `detect:` mapping ({threshold: 0.0, min_ms: 5.0, max_ms: 400.0, pad_frames: 0}): the gaps are
                                   # found in the file itself (engine.find_gaps) instead of given as `mask:` / `masks:`; needs `long:`
    detect_channels: str = "each"  # `channels:` inside `detect:` (needs long: {rate: file}), for a multi-channel file: "each" (default:
                                   # every channel is scanned and repaired on its own) or "joint" (a gap is where ALL channels are
                                   # quiet, and is repaired in all of them: DESIGN.md 4.18)
    detect_dead: Optional[dict] = None  # `kind:`, `rel_threshold:` and `held_tol:` inside `detect:`: kind "quiet" (default),
                                        # "held" (a sample repeated, a DC level) or "any"; rel_threshold a fraction of the file's peak in
                                        # [0, 1]; held_tol in full-scale units like threshold.  {quiet, 0.0, 0.0} is the detection of 4.15.
                                        # kind "level" (DESIGN.md 4.25): the RMS level of a window of `win_ms:` against the threshold
                                        # kind "burst" (DESIGN.md 4.28): the second difference's RMS level over `win_ms:` AT OR ABOVE the
                                        # threshold -- a block of corrupted PCM; rel_threshold in [0, 4] there; start from threshold: 1.15
                                        # kind "invalid" (DESIGN.md 4.30): NaN, inf and |x| > threshold, the CEILING in full-scale units
                                        # (0 or absent: none); min_ms defaults to 0 there; rel_threshold, held_tol, win_ms are refused
    detect_level: Optional[dict] = None  # `win_ms:` inside `detect:` ({win_ms: 2.0}): the window of kind "level" in
                                         # milliseconds, and of kind "burst" ({win_ms: 4.0} there), read at no other
                                         # kind; None without `detect:`
    detect_mend: Optional[dict] = None   # `mend_ms:`, `mend_order:` and `mend_context:` inside `detect:` (needs long: {rate: file}; DESIGN.md
                                         # 4.31): runs of at most mend_ms milliseconds (at most 64 samples) are filled from their own
                                         # neighbourhood by least-squares AR interpolation instead of a generated frame; {mend_ms, mend_order:
                                         # 32, mend_context: 512}; None when `mend_ms:` is absent or 0: the run is what it was
    detect_impulse: Optional[dict] = None  # `ratio:`, `order:`, `guard:` and `pad:` inside `detect:` with `kind: impulse`: clicks
                                           # and pops by AR prediction error against its own neighbourhood's over `win_ms:` ({win_ms: 23.0}
                                           # there); {ratio: 10.0, order: 16, guard: 4, pad: 2}; None at every other kind

    # derived exactly as the script does (I_ea/predict.py:85-90)
    @property
    def mask_ms(self) -> int:
        return int((self.mask_end_sec - self.mask_start_sec) * 1000)

    @property
    def mask_frames(self) -> int:
        return self.mask_ms // 20

    @property
    def start_sample(self) -> int:
        return int(self.mask_start_sec * 16000)

    @property
    def end_sample(self) -> int:
        return int(self.mask_end_sec * 16000)

    @property
    def mask_pos(self) -> int:
        return self.start_sample // 320

    @property
    def patch_fade(self) -> Optional[int]:
        """The cross-fade of patch mode in 22.05 kHz samples (fade_ms = 5 -> 110); None without a `patch:` key."""
        return None if self.patch_fade_ms is None else int(round(self.patch_fade_ms * 22.05))

    @property
    def gaps(self):
        """`masks:` as (first frame, frame count) pairs, each by the single mask's arithmetic (I_ea/predict.py:85-90); None without it."""
        if self.masks is None:
            return None
        return [(int(a * 16000) // 320, int((b - a) * 1000) // 20) for a, b in self.masks]

    @property
    def spans22(self):
        """`masks:` as [start, end) sample spans of the 22.05 kHz clip (I_ea/predict.py:99-100); None without it."""
        if self.masks is None:
            return None
        return [(int(a * 16000) * 22050 // 16000, int(b * 16000) * 22050 // 16000) for a, b in self.masks]


def load_predict_config(path: str = "predict.yaml") -> PredictConfig:
    with open(path) as f:
        data = yaml.safe_load(f)
    try:
        ds = data["training_config"]["dataset"]
        n = int(data["km_model"]["n_clusters"])
        ck = data["hifi_gan"]["checkpoint_file"]
        mask = data.get("mask", {})
        masks = data.get("masks")
        if masks is not None:
            if "mask" in data:
                raise ValueError(f"{path}: give either `mask:` (one gap) or `masks:` (a list of gaps), not both")
            if not isinstance(masks, list) or not masks:
                raise ValueError(f"{path}: `masks:` must be a non-empty list of {{start_pos_in_sec, end_pos_in_sec}} mappings")
            masks = sorted((float(m["start_pos_in_sec"]), float(m["end_pos_in_sec"])) for m in masks)
        patch_fade_ms = None
        if "patch" in data:
            pm = data["patch"] if data["patch"] is not None else {}
            if not isinstance(pm, dict):
                raise ValueError(f"{path}: `patch:` must be a mapping (fade_ms: <milliseconds>, default 5)")
            for key in pm:
                if key != "fade_ms":
                    raise ValueError(f"{path}: unknown key `{key}` in `patch:` (it takes fade_ms)")
            patch_fade_ms = float(pm.get("fade_ms", 5))
            if patch_fade_ms < 0:
                raise ValueError(f"{path}: patch.fade_ms = {patch_fade_ms} is negative")
        long_cfg, long_rate, long_feed, long_clips16, long_pcm24 = None, 22050, "recording", "resampled", "float32"
        if "long" in data:
            lm = data["long"] if data["long"] is not None else {}
            if not isinstance(lm, dict):
                raise ValueError(f"{path}: `long:` must be a mapping (clip_s: <seconds>, context_s: <seconds>, batch: <contexts per pass>)")
            long_cfg = {"clip_s": 4.0, "context_s": 1.0, "batch": 32}
            lm = dict(lm)
            if "rate" in lm:
                long_rate = lm.pop("rate")
                if long_rate not in (22050, "file"):
                    raise ValueError(f"{path}: long.rate = {long_rate!r}: 22050 (the default) or file (the file's own rate and sample type)")
            if "feed" in lm:
                long_feed = lm.pop("feed")
                if long_feed not in ("recording", "contexts"):
                    raise ValueError(f"{path}: long.feed = {long_feed!r}: recording (the default: the whole file is resampled to feed the model) or "
                                     f"contexts (only the context clips are cut from the file, at its own rate)")
                if long_feed == "contexts" and long_rate != "file":
                    raise ValueError(f"{path}: long.feed = contexts needs `rate: file` (at rate: {long_rate} the recording is resampled as a whole)")
            if "clips16" in lm:
                long_clips16 = lm.pop("clips16")
                if long_clips16 not in ("resampled", "file"):
                    raise ValueError(f"{path}: long.clips16 = {long_clips16!r}: resampled (the default: the 16 kHz clips are the cut 22.05 kHz clips "
                                     f"resampled) or file (they are cut straight from the file as well)")
                if long_clips16 == "file" and long_feed != "contexts":
                    raise ValueError(f"{path}: long.clips16 = file needs `feed: contexts` (with feed: {long_feed} the clips are slices of the "
                                     f"resampled recording)")
            if "pcm24" in lm:
                long_pcm24 = lm.pop("pcm24")
                if long_pcm24 not in ("float32", "keep"):
                    raise ValueError(f"{path}: long.pcm24 = {long_pcm24!r}: float32 (the default: a 24-bit file is read and written as float32) or "
                                     f"keep (its packed samples are repaired in place and written 24-bit)")
                if long_pcm24 == "keep" and (long_rate != "file" or long_feed != "contexts"):
                    raise ValueError(f"{path}: long.pcm24 = keep needs `rate: file` and `feed: contexts` (with rate: {long_rate}, feed: {long_feed} "
                                     f"the recording is resampled as a whole, from a float32 copy)")
            for key, val in lm.items():
                if key not in long_cfg:
                    raise ValueError(f"{path}: unknown key `{key}` in `long:` (it takes clip_s, context_s, batch, rate, feed) and, with feed: "
                                     f"contexts, clips16 and pcm24")
                long_cfg[key] = int(val) if key == "batch" else float(val)
                if long_cfg[key] < 0:
                    raise ValueError(f"{path}: long.{key} = {long_cfg[key]} is negative")
            if long_cfg["batch"] < 1 or long_cfg["clip_s"] <= 2 * long_cfg["context_s"]:
                raise ValueError(f"{path}: `long:` needs batch >= 1 and clip_s > 2 * context_s, got {long_cfg}")
        detect_cfg, detect_channels, detect_dead, detect_level, detect_mend, detect_impulse = None, "each", None, None, None, None
        if "detect" in data:
            dm = data["detect"] if data["detect"] is not None else {}
            if not isinstance(dm, dict):
                raise ValueError(f"{path}: `detect:` must be a mapping (threshold: <full scale>, min_ms: <milliseconds>, max_ms: <milliseconds>, "
                                 f"pad_frames: <20 ms frames>)")
            if long_cfg is None:
                raise ValueError(f"{path}: `detect:` needs a `long:` mapping (the gaps it finds are served on the recording's own time axis)")
            if "mask" in data or "masks" in data:
                raise ValueError(f"{path}: give either `detect:` (the gaps are found) or `mask:` / `masks:` (the gaps are given), not both")
            detect_cfg = {"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0}
            dm = dict(dm)
            detect_dead = {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}
            if "kind" in dm:
                detect_dead["kind"] = dm.pop("kind")
                if detect_dead["kind"] not in ("quiet", "held", "any", "level", "burst", "invalid", "impulse"):
                    raise ValueError(f"{path}: detect.kind = {detect_dead['kind']!r}: quiet (the default: |x| <= the threshold), held (a sample "
                                     f"repeated, a DC level) or any, or level (the RMS level of a window of win_ms milliseconds <= the threshold), "
                                     f"or burst (the RMS level of the second difference over a window of win_ms milliseconds >= the threshold), "
                                     f"or invalid (NaN, inf and |x| > the threshold, the ceiling; 0 = no ceiling), "
                                     f"or impulse (clicks and pops: a sample's AR prediction error `ratio` times over that of its neighbourhood of win_ms milliseconds)")
            for key in ("rel_threshold", "held_tol"):
                if key in dm:
                    detect_dead[key] = float(dm.pop(key))
                    if not detect_dead[key] >= 0:
                        raise ValueError(f"{path}: detect.{key} = {detect_dead[key]} is negative")
            burst = detect_dead["kind"] == "burst"                   # a second difference reaches 4 * the peak
            invalid = detect_dead["kind"] == "invalid"               # the sample's value is the damage; threshold = the ceiling
            if invalid:
                detect_cfg["min_ms"] = 0.0                           # a single NaN is a run of one sample: the default at this kind only
                for key in ("rel_threshold", "held_tol"):
                    if detect_dead[key] != 0:
                        raise ValueError(f"{path}: detect.{key} = {detect_dead[key]} with `kind: invalid` (the ceiling is `threshold:`, in full-scale "
                                         f"units; nothing at this kind follows the peak or a neighbour)")
            impulse = detect_dead["kind"] == "impulse"               # a prediction error; the floor may reach 4 * the peak as well
            if detect_dead["rel_threshold"] > (4 if burst or impulse else 1):
                raise ValueError(f"{path}: detect.rel_threshold = {detect_dead['rel_threshold']} is a fraction of the file's peak, at most "
                                 f"{'4 with `kind: burst`' if burst else '4 with `kind: impulse`' if impulse else 1}")
            detect_level = {"win_ms": G.IMPULSE_DEFAULTS["win_ms"] if impulse else 4.0 if burst else 2.0}
            given = [key for key in ("ratio", "order", "guard", "pad") if key in dm]
            if given and not impulse:
                raise ValueError(f"{path}: detect.{given[0]} needs `kind: impulse` (kind: {detect_dead['kind']} has no prediction-error test)")
            if impulse:
                detect_impulse = {"ratio": float(dm.pop("ratio", G.IMPULSE_DEFAULTS["ratio"]))}
                for key in ("order", "guard", "pad"):
                    val = dm.pop(key, G.IMPULSE_DEFAULTS[key])
                    if isinstance(val, bool) or int(val) != val:
                        raise ValueError(f"{path}: detect.{key} = {val!r}: a whole number")
                    detect_impulse[key] = int(val)
                if not 1 <= detect_impulse["ratio"] <= 1e6:
                    raise ValueError(f"{path}: detect.ratio = {detect_impulse['ratio']} is NaN or outside [1, 1e6] (10 is the default)")
                if not 2 <= detect_impulse["order"] <= G.IMPULSE_MAX_ORDER:
                    raise ValueError(f"{path}: detect.order = {detect_impulse['order']}, outside 2 .. {G.IMPULSE_MAX_ORDER} (16 is the default)")
                if not 0 <= detect_impulse["guard"] <= G.IMPULSE_MAX_GUARD:
                    raise ValueError(f"{path}: detect.guard = {detect_impulse['guard']} samples, outside 0 .. {G.IMPULSE_MAX_GUARD} (4 is the default)")
                if not 0 <= detect_impulse["pad"] <= G.IMPULSE_MAX_PAD:
                    raise ValueError(f"{path}: detect.pad = {detect_impulse['pad']} samples, outside 0 .. {G.IMPULSE_MAX_PAD} (2 is the default)")
            if "win_ms" in dm:
                detect_level["win_ms"] = float(dm.pop("win_ms"))
                if detect_dead["kind"] not in ("level", "burst", "impulse"):
                    raise ValueError(f"{path}: detect.win_ms needs `kind: level` (kind: {detect_dead['kind']} judges sample by sample and has no window)"
                                     + (": `kind: invalid` takes threshold, min_ms, max_ms, pad_frames and channels" if invalid else ""))
                if not 0 <= detect_level["win_ms"] < float("inf"):
                    raise ValueError(f"{path}: detect.win_ms = {detect_level['win_ms']} is negative or not finite")
            if detect_dead["kind"] in ("level", "burst", "impulse") and detect_dead["held_tol"] != 0:
                raise ValueError(f"{path}: detect.held_tol = {detect_dead['held_tol']} with `kind: {detect_dead['kind']}` (held samples are kind: held or any)")
            if "channels" in dm:
                detect_channels = dm.pop("channels")
                if detect_channels not in ("each", "joint"):
                    raise ValueError(f"{path}: detect.channels = {detect_channels!r}: each (the default: every channel is scanned and repaired on its "
                                     f"own) or joint (a gap is where all channels are quiet)")
                if long_rate != "file":
                    raise ValueError(f"{path}: detect.channels needs `long: {{rate: file}}` (at rate: {long_rate} the file is mixed down to one channel)")
            given = [key for key in ("mend_ms", "mend_order", "mend_context") if key in dm]
            if given:                                                # short runs mended in place, the rest inpainted
                if long_rate != "file":
                    raise ValueError(f"{path}: detect.{given[0]} needs `long: {{rate: file}}` (short runs are mended in the file's own samples; at "
                                     f"rate: {long_rate} the file is resampled first)")
                if "mend_ms" not in dm:
                    raise ValueError(f"{path}: detect.{given[0]} without detect.mend_ms (mend_ms: <milliseconds> switches the mending on)")
                mend = {"mend_ms": float(dm.pop("mend_ms")), "mend_order": int(dm.pop("mend_order", 32)), "mend_context": int(dm.pop("mend_context", 512))}
                if not 0 <= mend["mend_ms"] < float("inf"):
                    raise ValueError(f"{path}: detect.mend_ms = {mend['mend_ms']} is negative or not finite")
                if not 2 <= mend["mend_order"] <= 32:
                    raise ValueError(f"{path}: detect.mend_order = {mend['mend_order']}, outside 2 .. 32")
                if not 4 * mend["mend_order"] <= mend["mend_context"] <= 1024:
                    raise ValueError(f"{path}: detect.mend_context = {mend['mend_context']} samples, outside 4 * mend_order = {4 * mend['mend_order']} .. 1024")
                min_ms = float(dm.get("min_ms", detect_cfg["min_ms"]))
                if mend["mend_ms"] > 0 and min_ms >= mend["mend_ms"]:
                    raise ValueError(f"{path}: detect.min_ms = {min_ms} is not under detect.mend_ms = {mend['mend_ms']}: no run short enough to mend "
                                     f"would be reported; lower min_ms (0 reports a single sample)")
                detect_mend = mend if mend["mend_ms"] > 0 else None
            for key, val in dm.items():
                if key not in detect_cfg:
                    raise ValueError(f"{path}: unknown key `{key}` in `detect:` (it takes threshold, min_ms, max_ms, pad_frames, channels, kind, rel_threshold, "
                                     f"held_tol) and, with kind: level, win_ms (kind: burst takes it too)")
                detect_cfg[key] = int(val) if key == "pad_frames" else float(val)
                if not detect_cfg[key] >= 0:
                    raise ValueError(f"{path}: detect.{key} = {detect_cfg[key]} is negative")
        return PredictConfig(
            dataset=ds,
            wave_path=data["wave"][ds]["wave_path"],
            save_pred=data["wave"][ds]["save_pred"],
            n_clusters=n,
            km_model_path=os.path.join(data["km_model"][ds]["km_model_path"], f"km_model_{n}/model.km"),
            path2centroids=os.path.join(data["km_model"][ds]["path2centroids"], f"km_model_{n}/label_dir/validation"),
            device_index=data.get("device", {}).get("index", 0),
            mask_start_sec=float(mask.get("start_pos_in_sec", 0.0)),
            mask_end_sec=float(mask.get("end_pos_in_sec", 0.0)),
            hifigan_checkpoint=ck,
            hifigan_config=os.path.join(os.path.split(ck)[0], "config.json"),
            hubert_type=str(data["hubert_model"]["type"]),
            hubert_checkpoint=data["hubert_model"][ds]["model_checkpoint"],
            asr_model_name=data.get("ASR_model", {}).get("model_name"),
            raw=data, masks=masks, patch_fade_ms=patch_fade_ms, long=long_cfg, long_rate=long_rate, long_feed=long_feed, long_clips16=long_clips16,
            long_pcm24=long_pcm24, detect=detect_cfg,
            detect_channels=detect_channels, detect_dead=detect_dead, detect_level=detect_level, detect_mend=detect_mend,
            detect_impulse=detect_impulse)
    except KeyError as e:
        raise KeyError(f"{path}: missing key {e} (schema: I_ea/predict.yaml)") from None


def load_hifigan_config(path: str) -> AttrDict:
    with open(path) as f:
        return AttrDict(json.load(f))
