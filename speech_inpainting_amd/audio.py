"""Host-side audio glue around the hot path: wav I/O and resampling (still host code).

The masking / peak normalisation / log-mel front-end of the 22.05 kHz side (row f-1) is in the HIP library
(`si_mel_frontend`, csrc/frontend_kernels.hip); nothing here computes a mel.

* resampling: `librosa.load(sr=...)` (I_ea/predict.py:79-80) uses a Kaiser-windowed sinc resampler; here scipy's
  polyphase resampler with a Kaiser window.  Not bit-identical to librosa; documented as such (librosa is absent, so
  there is no in-container oracle for it).
"""
from __future__ import annotations

import math
import numpy as np
import torch

MAX_WAV_VALUE = 32768.0


def read_wav(path: str):
    """-> (float32 mono in [-1, 1], sample_rate)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    else:
        x = data.astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=1)
    return x, int(sr)


KAISER_BETA = 14.769656459379492


def design_resampler(sr_in: int, sr_out: int, n_in: int):
    """Filter and index bookkeeping of `scipy.signal.resample_poly(x, up, down, window=("kaiser", beta))` for the GPU
    resampler (si_resample_poly): returns (taps float32 incl. resample_poly's zero pre-padding, up, down, pre_remove,
    n_out).  The filter is designed in float64 exactly as resample_poly designs it (firwin(2 * 10 * max(up, down) + 1,
    1 / max(up, down)) * up) and rounded to float32 once."""
    from scipy.signal import firwin
    g = math.gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    n_out = n_in * up
    n_out = n_out // down + bool(n_out % down)
    half_len = 10 * max(up, down)
    h = firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", KAISER_BETA)) * up
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    taps = np.concatenate([np.zeros(n_pre_pad), h]).astype(np.float32)
    return taps, up, down, n_pre_remove, n_out


KAISER_BEST = dict(num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=KAISER_BETA)


def resampled_len(n: int, sr_in: int, sr_out: int) -> int:
    """Samples of `librosa.load(path, sr=sr_out)` for a file of n samples at sr_in: librosa 0.9.1's `ceil(n * ratio)` with the ratio
    rounded to float64 FIRST (librosa/core/audio.py resample: ratio = float(target_sr) / orig_sr).  THE length rule of the resampler
    (design_kaiser_best) and of the request front; `ceil(n * float(sr_out) / sr_in)` -- the product first -- rounds differently
    (DESIGN.md 4.24).  The file-rate routes count with exact integers by their own definition."""
    if int(sr_in) == int(sr_out):
        return int(n)
    return int(math.ceil(n * (float(sr_out) / float(sr_in))))


def design_kaiser_best(sr_in: int, sr_out: int, n_in: int):
    """Tables of resampy's `kaiser_best` band-limited interpolation -- the resampler behind `librosa.load(path, sr=...)` in the
    reference's pinned librosa==0.9.1 (I_ea/predict.py:79-80; requirements.txt:3) -- for the GPU kernel (si_resample_sinc):
    win = rolloff * sinc(rolloff * t), t in [0, 64] at 512 samples per zero crossing, tapered by the right half of a Kaiser window
    (beta 14.77), scaled by the ratio when down-sampling; dwin = its forward differences; time_reg[t] = output sample t's input time,
    1 / ratio accumulated by REPEATED ADDITION in float64 as resampy's loop does (at exactly-integer times the accumulated rounding
    selects the table phase, and the phases differ because the table step is truncated to an integer).
    -> dict(win, dwin, time_reg float64 numpy; num_table, step, scale, ratio, n_out = ceil(n_in * ratio) (librosa's fix_length))."""
    from scipy.signal.windows import kaiser
    ratio = float(sr_out) / float(sr_in)
    nb = 2 ** KAISER_BEST["precision"]
    n = nb * KAISER_BEST["num_zeros"]
    r = KAISER_BEST["rolloff"]
    win = kaiser(2 * n + 1, KAISER_BEST["beta"])[n:] * (r * np.sinc(r * np.linspace(0, KAISER_BEST["num_zeros"], num=n + 1, endpoint=True)))
    if ratio < 1:
        win = win * ratio
    dwin = np.zeros_like(win)
    dwin[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    n_out = resampled_len(n_in, sr_in, sr_out)
    return dict(win=np.ascontiguousarray(win), dwin=dwin, time_reg=time_registers(sr_in, sr_out, n_out), num_table=nb, step=int(scale * nb),
                scale=scale, ratio=ratio, n_out=n_out)


def time_registers(sr_in: int, sr_out: int, n_out: int) -> np.ndarray:
    """design_kaiser_best's time_reg alone: entry t is the running float64 sum of t + 1 increments 1 / ratio (a sequential
    accumulation) less one increment, whatever n_out is -- the table for a shorter clip is, bit for bit, a prefix of the table for a
    longer one (what lets the engine keep one per rate pair)."""
    inc = 1.0 / (float(sr_out) / float(sr_in))
    tr = np.cumsum(np.full(max(n_out, 1), inc)) - inc
    tr[0] = 0.0
    return tr[:n_out].copy()


def resample(x: np.ndarray, sr_in: int, sr_out: int) -> np.ndarray:
    """Host (scipy) resampler with the same filter: the reference of the GPU one in the tests; predict.py resamples on
    the GPU (InpaintingEngine.resample)."""
    if sr_in == sr_out:
        return x.astype(np.float32)
    from scipy.signal import resample_poly
    g = math.gcd(sr_in, sr_out)
    return resample_poly(x.astype(np.float64), sr_out // g, sr_in // g, window=("kaiser", KAISER_BETA)).astype(np.float32)


def load_audio(path: str, sr: int) -> np.ndarray:
    """Stand-in for `librosa.load(path, sr=sr)` (I_ea/predict.py:79-80)."""
    x, sr_in = read_wav(path)
    return resample(x, sr_in, sr)


def to_int16_pcm(audio: torch.Tensor, clip: bool = False) -> np.ndarray:
    """B6, the script's own two statements (I_ea/predict.py:204-206): `audio * 32768` in fp32, then numpy
    `.astype('int16')` -- truncation toward zero, no rounding.  The generator ends in tanh, so the product lies in
    [-32768, 32768]; only an exact +1.0 sample (tanhf saturates for pre-activations above ~9) is out of int16's range, and a
    float -> int16 cast of 32768.0 is undefined behaviour in C and numpy (x86 scalar code gives -32768: a full-scale negative
    click).  That ONE value is pinned to 32767; everywhere the reference's cast is defined the PCM is bit-identical to it.  The
    GPU form of the same statement is `InpaintingEngine.to_int16` (si_pcm16).
    clip=True is an opt-in deviation for callers who feed waveforms that did not come out of the generator: values are
    clamped to [-32768, 32767] before the cast."""
    a = audio.detach().float().cpu() * MAX_WAV_VALUE
    a = a.clamp(-32768.0, 32767.0) if clip else a.clamp(max=32767.0)
    return a.numpy().astype("int16")


def write_wav(path: str, pcm_or_float: np.ndarray, sr: int):
    from scipy.io import wavfile
    wavfile.write(path, sr, pcm_or_float)


# ---- packed 24-bit PCM: the bytes of a WAV data chunk, kept as they are
def pack_s24(v: np.ndarray) -> np.ndarray:
    """int32 values in [-2^23, 2^23 - 1], any shape -> uint8 (..., 3): little-endian packed signed 24-bit PCM, as a WAV data chunk
    holds it.  A value outside the range raises a ValueError."""
    v = np.asarray(v)
    if v.dtype.kind not in "iu":
        raise ValueError(f"pack_s24: {v.dtype} values, integers wanted")
    v = v.astype(np.int64)
    if v.size and (v.min() < -(1 << 23) or v.max() > (1 << 23) - 1):
        raise ValueError(f"pack_s24: values in [{v.min()}, {v.max()}], outside [-8388608, 8388607]")
    u = (v & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, u >> 16], axis=-1).astype(np.uint8)


def unpack_s24(b: np.ndarray) -> np.ndarray:
    """uint8 (..., 3) packed little-endian signed 24-bit PCM -> int32 (...): byte 0 is the low one, the sign is bit 7 of byte 2."""
    b = np.asarray(b)
    if b.dtype != np.uint8 or b.ndim < 1 or b.shape[-1] != 3:
        raise ValueError(f"unpack_s24: {b.dtype} {b.shape}, uint8 (..., 3) wanted")
    w = b[..., 0].astype(np.uint32) << 8 | b[..., 1].astype(np.uint32) << 16 | b[..., 2].astype(np.uint32) << 24
    return w.view(np.int32) >> 8 if w.ndim else np.int32(np.uint32(w).view(np.int32) >> 8)


_PCM_SUBFORMAT = bytes.fromhex("0100000000001000800000aa00389b71")      # KSDATAFORMAT_SUBTYPE_PCM, the GUID of WAVE_FORMAT_EXTENSIBLE


def read_wav_pcm(path: str):
    """A small RIFF reader for the one case the file-typed routes keep packed: -> (data, sample_rate, channels).  A 24-bit PCM file
    (format tag 1, or 0xFFFE with the PCM sub-format; 3 ch bytes per block) comes back as its data chunk's own bytes, uint8
    (n, ch, 3), a trailing partial block dropped.  Everything else is left to the existing reader: data is what scipy returns for
    the file, (n,) or (n, ch) in its own dtype.  Chunks other than `fmt ` and `data` are skipped, pad bytes honoured."""
    import struct
    with open(path, "rb") as f:
        blob = f.read()
    fmt = data = None
    if len(blob) >= 12 and blob[:4] == b"RIFF" and blob[8:12] == b"WAVE":
        pos = 12
        while pos + 8 <= len(blob):
            cid, size = blob[pos:pos + 4], struct.unpack_from("<I", blob, pos + 4)[0]
            body = blob[pos + 8:pos + 8 + size]
            if cid == b"fmt " and fmt is None:
                fmt = body
            elif cid == b"data" and data is None:
                data = body
            pos += 8 + size + (size & 1)
    if fmt is not None and data is not None and len(fmt) >= 16:
        tag, ch, sr, _, align, bits = struct.unpack_from("<HHIIHH", fmt, 0)
        if tag == 0xFFFE and len(fmt) >= 40 and fmt[24:40] == _PCM_SUBFORMAT:
            tag = 1
        if tag == 1 and bits == 24 and ch >= 1 and align == 3 * ch:
            n = len(data) // align
            return np.frombuffer(data, np.uint8, n * align).reshape(n, ch, 3).copy(), int(sr), int(ch)
    from scipy.io import wavfile
    sr, arr = wavfile.read(path)
    return arr, int(sr), (arr.shape[1] if arr.ndim == 2 else 1)


def write_wav_s24(path: str, data: np.ndarray, sr: int):
    """uint8 (n, 3) mono or (n, ch, 3) interleaved packed 24-bit PCM -> a 24-bit WAV file at `sr` Hz: a plain 16-byte PCM `fmt `
    chunk (format tag 1, blockAlign 3 ch), the bytes as the data chunk, and the RIFF pad byte when 3 n ch is odd."""
    import struct
    data = np.ascontiguousarray(data)
    if data.dtype != np.uint8 or data.ndim not in (2, 3) or data.shape[-1] != 3:
        raise ValueError(f"write_wav_s24: {data.dtype} {data.shape}, uint8 (n, 3) or (n, ch, 3) wanted")
    ch = data.shape[1] if data.ndim == 3 else 1
    if not 1 <= ch <= 65535:
        raise ValueError(f"write_wav_s24: {ch} channels")
    raw = data.tobytes()
    pad = len(raw) & 1
    fmt = struct.pack("<HHIIHH", 1, ch, int(sr), int(sr) * 3 * ch, 3 * ch, 24)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(raw) + pad) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", len(raw)) + raw + b"\0" * pad)
