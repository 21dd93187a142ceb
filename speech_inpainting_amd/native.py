"""ctypes binding of libsi_hip.so (include/si_hip.h).

PyTorch is only plumbing here: it owns device memory (inputs, outputs, workspace) and the HIP stream.
There is no CPU fallback: if the shared library is absent, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np
import torch

from .arch import HubertArch, VocoderArch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SI_HIP_LIB") or os.path.join(_HERE, "libsi_hip.so")   # SI_HIP_LIB: A/B builds of the library

SI_MATH = {"fp32": 0, "f32": 0, "bf16": 1, "bf16x3": 2, "fp16": 3, "f16": 3}
SI_MAX_CONV, SI_MAX_UPS, SI_MAX_RB, SI_MAX_DIL = 8, 8, 4, 4

EXPORTS = ["si_version", "si_create", "si_destroy", "si_last_error", "si_load_weights", "si_alloc_weights",
           "si_weights_device_ptr", "si_weights_check", "si_workspace_bytes", "si_hubert_forward", "si_hubert_forward_padded", "si_hubert_forward_varlen", "si_hubert_extract_features", "si_code_splice", "si_codebook_splice",
           "si_codebook_splice_varlen", "si_hifigan_forward_varlen", "si_mel_frontend_varlen",
           "si_codebook_splice_labels", "si_codebook_metrics", "si_kmeans_assign", "si_mel_metrics", "si_sisdr", "si_unit_frontend",
           "si_f0_encoder_weight_floats", "si_f0_encoder_frames", "si_f0_encoder_workspace_bytes", "si_f0_encoder_forward",
           "si_resample_poly", "si_resample_sinc", "si_pcm16", "si_extend_mel", "si_hifigan_forward", "si_mel_frames", "si_mel_workspace_bytes", "si_mel_frontend", "si_num_frames",
           "si_vocoder_samples", "si_profile_start", "si_profile_filter", "si_profile_stop",
           "si_debug_capture", "si_debug_size", "si_debug_ws_regions",
           "si_hubert_forward_spans", "si_mel_frontend_spans", "si_codebook_splice_spans", "si_codebook_splice_labels_spans",
           "si_codebook_metrics_spans", "si_wave_peak", "si_gather_windows", "si_patch_compose",
           "si_cut_clips", "si_patch_regions", "si_quiet_runs", "si_patch_rate", "si_cut_rate",
           "si_quiet_runs_ch", "si_cut_rate_ch", "si_patch_rate_ch", "si_dead_runs", "si_level_runs", "si_cut_pair", "si_cut_pair_ch",
           "si_plan_weights", "si_pack_weights_host", "si_burst_runs",
           "si_invalid_runs", "si_cut_rate_valid", "si_cut_pair_valid", "si_cut_clips_valid", "si_mend_runs",
           "si_impulse_runs", "si_impulse_residual"]
SI_MAX_SPANS = 16
SI_MAX_CHANNELS = 8                        # channels of an interleaved file
SAMPLE_F32, SAMPLE_S16, SAMPLE_S24 = 0, 1, 2   # SI_SAMPLE_*: the file-typed calls' sample types; s24 = uint8 (..., 3)
DEAD_QUIET, DEAD_HELD = 1, 2               # SI_DEAD_QUIET, SI_DEAD_HELD: the `kind` bits of si_dead_runs
LEVEL_MAX_HALF = 1024                      # SI_LEVEL_MAX_HALF: the largest half window of si_level_runs
IMPULSE_MAX_ORDER, IMPULSE_MAX_HALF, IMPULSE_MAX_GUARD, IMPULSE_MAX_PAD = 32, 1024, 64, 16   # SI_IMPULSE_MAX_*: the limits of si_impulse_runs
MEND_MAX_LEN, MEND_MAX_ORDER, MEND_MAX_CONTEXT, MEND_MAX_RUNS = 64, 32, 1024, 65536   # SI_MEND_MAX_*: the limits of si_mend_runs
MEND_LONG, MEND_AR, MEND_LINE, MEND_EDGE, MEND_NEAR, MEND_NONFINITE, MEND_BADROW = 0, 1, 2, 3, 4, 5, 6   # SI_MEND_*: a row's status
MEND_STATUS = ("LONG", "AR", "LINE", "EDGE", "NEAR", "NONFINITE", "BADROW")                         # their names, by code
CUT_RATE_TILE = 512                        # SI_CUT_RATE_TILE: consecutive outputs of one clip per workgroup of si_cut_rate
CUT_PAIR_FRAMES = 1                        # SI_CUT_PAIR_FRAMES: consecutive 20 ms frames of one clip per workgroup of si_cut_pair


def cut_pair_lds_floats(sr: int, reach22: int, reach16: int) -> int:
    """The floats of LDS one workgroup of si_cut_pair stages at `sr` Hz: ceil(CUT_PAIR_FRAMES sr / 50) + 2 + 2 max(H22, H16), H = taps per
    wing of the two filters (H16 = 0 at 16 kHz, which has none).  The call refuses above 16384 (64 KB)."""
    return -(-CUT_PAIR_FRAMES * int(sr) // 50) + 2 + 2 * max(int(reach22), int(reach16))


class _F0EncStruct(C.Structure):
    """Mirror of si_f0enc_desc."""
    _fields_ = [(n, C.c_int32) for n in ("in_width", "out_width", "width", "n_state", "depth", "down_t", "stride_t", "dilation_growth")]


class F0EncDesc:
    """`f0_encoder_params` of I_da/configs/LJSpeech/hubert_lut.json:42-52 (one level): n_state = int(m_conv * width)."""

    def __init__(self, in_width=1, out_width=128, width=32, depth=4, down_t=4, stride_t=2, dilation_growth=3, m_conv=1.0):
        self.in_width, self.out_width, self.width, self.depth = int(in_width), int(out_width), int(width), int(depth)
        self.down_t, self.stride_t, self.dilation_growth = int(down_t), int(stride_t), int(dilation_growth)
        self.n_state = int(m_conv * width)

    def as_struct(self) -> _F0EncStruct:
        return _F0EncStruct(self.in_width, self.out_width, self.width, self.n_state, self.depth, self.down_t, self.stride_t, self.dilation_growth)

    def down_kernel(self):
        s = self.stride_t
        return (2 * s, s // 2) if s % 2 == 0 else (2 * s + 1, s // 2 + 1)          # jukebox.py:54-57


class SincFilter(C.Structure):
    """Mirror of si_sinc_filter."""
    _fields_ = [("struct_size", C.c_int32), ("nwin", C.c_int32), ("num_table", C.c_int32), ("step", C.c_int32), ("n_time", C.c_int32),
                ("reserved", C.c_int32), ("scale", C.c_double), ("ratio", C.c_double), ("win", C.c_void_p), ("dwin", C.c_void_p),
                ("time_reg", C.c_void_p)]


class SpanTableStruct(C.Structure):
    """Mirror of si_span_table."""
    _fields_ = [("struct_size", C.c_int32), ("num_clips", C.c_int32), ("num_spans", C.c_int32), ("reserved", C.c_int32),
                ("host_off", C.c_void_p), ("host_start", C.c_void_p), ("host_len", C.c_void_p),
                ("span_off", C.c_void_p), ("span_start", C.c_void_p), ("span_len", C.c_void_p)]


class SpanTable:
    """The zeroed sample spans of a batch as si_span_table takes them: `spans` = per clip a list of (start, len) in samples, sorted
    and disjoint (gaps.spans16 / gaps.spans22 build them from frame-level gaps).  Holds the host arrays the library validates and
    ONE device tensor [off | start | len] the kernels read (a single host-to-device copy); the library refuses a table that is
    unsorted, overlapping or above SI_MAX_SPANS spans per clip before it launches anything.
    staged = (host, dev): int32 views of `words(spans)` elements each -- a numpy view of a caller-owned (pinned) host buffer, which
    is filled here, and the device tensor the CALLER copies it to (on a stream of its choice, before the table is used)."""

    @staticmethod
    def words(spans) -> int:
        return len(spans) + 2 + 2 * sum(len(c) for c in spans)

    def __init__(self, spans, device, staged=None):
        from .gaps import csr
        off, st, ln = csr(spans)
        self.B, self.n = len(off) - 1, len(st)
        vals = np.array(off + st + ln + [0], dtype=np.int32)                                  # (+ 1: never an empty array)
        if staged is None:
            self.host = np.ascontiguousarray(vals)
            self.dev = torch.from_numpy(self.host).to(device, non_blocking=True)
        else:
            self.host, self.dev = staged
            if self.host.size != vals.size or self.dev.numel() != vals.size:
                raise ValueError(f"SpanTable: staged views of {self.host.size} / {self.dev.numel()} words, the table has {vals.size}")
            np.copyto(self.host, vals)

    def spans(self):
        """The table back as per-clip lists of (start, len), from the host copy."""
        B, n, h = self.B, self.n, self.host
        return [[(int(h[B + 1 + k]), int(h[B + 1 + n + k])) for k in range(int(h[b]), int(h[b + 1]))] for b in range(B)]

    def struct(self) -> SpanTableStruct:
        h, d, B, n = self.host.ctypes.data, self.dev.data_ptr(), self.B, self.n
        return SpanTableStruct(C.sizeof(SpanTableStruct), B, n, 0, h, h + 4 * (B + 1), h + 4 * (B + 1 + n),
                               d, d + 4 * (B + 1), d + 4 * (B + 1 + n))


class PatchTableStruct(C.Structure):
    """Mirror of si_patch_table."""
    _fields_ = [("struct_size", C.c_int32), ("num_clips", C.c_int32), ("num_windows", C.c_int32), ("num_spans", C.c_int32),
                ("fade", C.c_int32), ("reserved", C.c_int32),
                ("host_win_clip", C.c_void_p), ("host_win_start", C.c_void_p), ("host_win_len", C.c_void_p), ("host_span_win", C.c_void_p),
                ("host_lim", C.c_void_p),
                ("win_start", C.c_void_p), ("win_len", C.c_void_p), ("span_win", C.c_void_p), ("lim", C.c_void_p), ("ramp", C.c_void_p)]


class PatchTable:
    """Where the generated samples of each span lie, as si_patch_table takes it (the companion of the 22.05 kHz SpanTable):
    windows = (clip, first 22.05 kHz sample, samples) per generator row; span_win = per span of the SpanTable (flat, its order) the row
    that holds it (-1 for a span that is skipped); lim = per clip min(its samples, its generated samples); fade in samples.
    Like SpanTable it holds the host words the library validates and ONE device tensor
    [win_clip | win_start | win_len | span_win | lim | ramp (fp32 bits)] the kernel reads -- one array, one copy.
    staged = (host, dev) as SpanTable's: views of `words(...)` int32 elements of a caller-owned (pinned) buffer and of the device
    tensor the caller copies it to."""

    @staticmethod
    def words(n_windows: int, n_spans: int, n_clips: int, fade: int) -> int:
        return 3 * n_windows + n_spans + n_clips + fade + 1

    def __init__(self, windows, span_win, lim, fade: int, device, staged=None):
        from .gaps import fade_ramp
        self.W, self.S, self.B, self.fade = len(windows), len(span_win), len(lim), int(fade)
        cols = [[int(w[j]) for w in windows] for j in range(3)]
        ints = np.array(cols[0] + cols[1] + cols[2] + [int(k) for k in span_win] + [int(n) for n in lim], dtype=np.int32)
        vals = np.concatenate([ints, fade_ramp(self.fade).view(np.int32), np.zeros(1, np.int32)])    # (+ 1: never an empty array)
        if staged is None:
            self.host = np.ascontiguousarray(vals)
            self.dev = torch.from_numpy(self.host).to(device, non_blocking=True)
        else:
            self.host, self.dev = staged
            if self.host.size != vals.size or self.dev.numel() != vals.size:
                raise ValueError(f"PatchTable: staged views of {self.host.size} / {self.dev.numel()} words, the table has {vals.size}")
            np.copyto(self.host, vals)

    def struct(self) -> PatchTableStruct:
        h, d, W, S, B = self.host.ctypes.data, self.dev.data_ptr(), self.W, self.S, self.B
        o = [0, 4 * W, 8 * W, 12 * W, 12 * W + 4 * S, 12 * W + 4 * S + 4 * B]
        return PatchTableStruct(C.sizeof(PatchTableStruct), B, W, S, self.fade, 0, h + o[0], h + o[1], h + o[2], h + o[3], h + o[4],
                                d + o[1], d + o[2], d + o[3], d + o[4], d + o[5])


class RegionTableStruct(C.Structure):
    """Mirror of si_region_table."""
    _HOST = ("start", "len", "span_win", "span_lim", "win_ctx", "win_start", "win_len", "chunk", "k0", "k1")
    _fields_ = ([(n, C.c_int32) for n in ("struct_size", "num_contexts", "num_windows", "num_spans", "num_chunks", "fade")] +
                [("host_" + n, C.c_void_p) for n in _HOST] + [(n, C.c_void_p) for n in _HOST] + [("ramp", C.c_void_p)])


class RegionTable:
    """The blend regions of many context clips on the recording's own 22.05 kHz sample axis, as si_region_table takes them:
    spans = (start, len, window, lim) per span, sorted and disjoint (lim: the recording sample where its context's generated audio
    ends); windows = (context, first recording sample, samples) per generator row; chunks = (chunk, k0, k1) per touched chunk of 2048
    samples (gaps.region_chunks); n_contexts = entries of the gain vector; fade in samples.  Like PatchTable: the host words the
    library validates and ONE device tensor [start | len | span_win | span_lim | win_ctx | win_start | win_len | chunk | k0 | k1 |
    ramp (fp32 bits)] the kernel reads -- one array, one copy."""

    def __init__(self, spans, windows, chunks, n_contexts: int, fade: int, device):
        from .gaps import fade_ramp
        self.K, self.W, self.Q, self.C, self.fade = len(spans), len(windows), len(chunks), int(n_contexts), int(fade)
        cols = [[int(r[j]) for r in rows] for rows, n in ((spans, 4), (windows, 3), (chunks, 3)) for j in range(n)]
        ints = np.array([v for col in cols for v in col], dtype=np.int32)
        self.host = np.ascontiguousarray(np.concatenate([ints, fade_ramp(self.fade).view(np.int32), np.zeros(1, np.int32)]))   # (+ 1: never empty)
        self.dev = torch.from_numpy(self.host).to(device, non_blocking=True)

    def struct(self) -> RegionTableStruct:
        h, d, K, W, Q = self.host.ctypes.data, self.dev.data_ptr(), self.K, self.W, self.Q
        o = [4 * x for x in (0, K, 2 * K, 3 * K, 4 * K, 4 * K + W, 4 * K + 2 * W, 4 * K + 3 * W, 4 * K + 3 * W + Q, 4 * K + 3 * W + 2 * Q,
                             4 * K + 3 * W + 3 * Q)]
        return RegionTableStruct(C.sizeof(RegionTableStruct), self.C, W, K, Q, self.fade, *[h + x for x in o[:10]], *[d + x for x in o[:10]], d + o[10])


class RateTableStruct(C.Structure):
    """Mirror of si_rate_table."""
    _HOST = ("start", "len", "span_win", "span_lim", "win_ctx", "win_start", "win_len", "win_lim", "chunk", "k0", "k1")
    _fields_ = ([(n, C.c_int32) for n in ("struct_size", "num_contexts", "num_windows", "num_spans", "num_chunks", "fade")] +
                [("host_" + n, C.c_void_p) for n in _HOST] + [(n, C.c_void_p) for n in _HOST] + [("ramp", C.c_void_p)])


class RateTable:
    """RegionTable for a file at its own sample rate, as si_rate_table takes it: spans = (start, len, window, lim) per span in FILE
    samples, sorted and disjoint; windows = (context, first sample, samples, lim) per generator row in 22.05 kHz samples of the
    recording (lim: where its context's generated audio ends); chunks = (chunk, k0, k1) per touched chunk of 2048 FILE samples
    (gaps.region_chunks); fade in file samples.  One array, one copy: [start | len | span_win | span_lim | win_ctx | win_start |
    win_len | win_lim | chunk | k0 | k1 | ramp (fp32 bits)].  A value outside int32 is refused here (the library could not see it)."""

    def __init__(self, spans, windows, chunks, n_contexts: int, fade: int, device):
        from .gaps import fade_ramp
        self.K, self.W, self.Q, self.C, self.fade = len(spans), len(windows), len(chunks), int(n_contexts), int(fade)
        for what, rows, n in (("span", spans, 4), ("window", windows, 4), ("chunk", chunks, 3)):
            for k, r in enumerate(rows):
                if len(r) != n or any(not -2 ** 31 <= int(v) < 2 ** 31 for v in r):
                    raise ValueError(f"RateTable: {what} {k} = {tuple(r)} is not {n} int32 values")
        cols = [[int(r[j]) for r in rows] for rows, n in ((spans, 4), (windows, 4), (chunks, 3)) for j in range(n)]
        ints = np.array([v for col in cols for v in col], dtype=np.int32)
        self.host = np.ascontiguousarray(np.concatenate([ints, fade_ramp(self.fade).view(np.int32), np.zeros(1, np.int32)]))   # (+ 1: never empty)
        self.dev = torch.from_numpy(self.host).to(device, non_blocking=True)

    def struct(self) -> RateTableStruct:
        h, d, K, W, Q = self.host.ctypes.data, self.dev.data_ptr(), self.K, self.W, self.Q
        o = [4 * x for x in [j * K for j in range(4)] + [4 * K + j * W for j in range(4)] + [4 * K + 4 * W + j * Q for j in range(4)]]
        return RateTableStruct(C.sizeof(RateTableStruct), self.C, W, K, Q, self.fade, *[h + x for x in o[:11]], *[d + x for x in o[:11]], d + o[11])


class ExtractDesc(C.Structure):
    """Mirror of si_extract_desc."""
    _fields_ = [("struct_size", C.c_int32), ("output_layer", C.c_int32), ("normalize", C.c_int32), ("reserved", C.c_int32)]


NORMALIZE_MODES = {None: 0, False: 0, "none": 0, "processor": 1, True: 1, "layer_norm": 2}


class ProfileEntry(C.Structure):
    """Mirror of si_profile_entry."""
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int32), ("reserved", C.c_int32),
                ("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


class WsRegion(C.Structure):
    """Mirror of si_ws_region."""
    _fields_ = [("name", C.c_char * 24), ("offset", C.c_uint64), ("bytes", C.c_uint64)]


class ModelDesc(C.Structure):
    """Mirror of si_model_desc (include/si_hip.h)."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("hidden_size", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("intermediate_size", C.c_int32),
        ("num_conv", C.c_int32),
        ("conv_dim", C.c_int32 * SI_MAX_CONV), ("conv_kernel", C.c_int32 * SI_MAX_CONV), ("conv_stride", C.c_int32 * SI_MAX_CONV),
        ("conv_bias", C.c_int32), ("feat_norm_layer", C.c_int32), ("stable_layer_norm", C.c_int32),
        ("pos_conv_kernel", C.c_int32), ("pos_conv_groups", C.c_int32), ("feat_proj_layer_norm", C.c_int32),
        ("layer_norm_eps", C.c_float), ("codebook_dim", C.c_int32), ("num_clusters", C.c_int32),
        ("num_mels", C.c_int32), ("num_ups", C.c_int32),
        ("up_rates", C.c_int32 * SI_MAX_UPS), ("up_kernels", C.c_int32 * SI_MAX_UPS), ("up_initial_channel", C.c_int32),
        ("num_rb", C.c_int32), ("rb_kernels", C.c_int32 * SI_MAX_RB), ("num_dil", C.c_int32),
        ("rb_dilations", (C.c_int32 * SI_MAX_DIL) * SI_MAX_RB),
        ("encoder_math", C.c_int32), ("vocoder_math", C.c_int32), ("vocoder_chunk", C.c_int32), ("resblock_type", C.c_int32),
    ]


def make_desc(harch: HubertArch, varch: VocoderArch, num_clusters: int, encoder_math: str = "fp32",
              vocoder_math: str = "fp32", vocoder_chunk: int = 0) -> ModelDesc:
    d = ModelDesc()
    d.struct_size = C.sizeof(ModelDesc)
    d.hidden_size, d.num_layers = harch.hidden_size, harch.num_hidden_layers
    d.num_heads, d.intermediate_size = harch.num_attention_heads, harch.intermediate_size
    n = len(harch.conv_dim)
    if n > SI_MAX_CONV or not (len(harch.conv_kernel) == len(harch.conv_stride) == n):
        raise ValueError("unsupported conv stack")
    d.num_conv = n
    for i in range(n):
        d.conv_dim[i], d.conv_kernel[i], d.conv_stride[i] = harch.conv_dim[i], harch.conv_kernel[i], harch.conv_stride[i]
    d.conv_bias = int(harch.conv_bias)
    if harch.feat_extract_norm not in ("group", "layer"):
        raise ValueError(f"feat_extract_norm={harch.feat_extract_norm!r}")
    d.feat_norm_layer = int(harch.feat_extract_norm == "layer")
    d.stable_layer_norm = int(harch.do_stable_layer_norm)
    d.pos_conv_kernel, d.pos_conv_groups = harch.num_conv_pos_embeddings, harch.num_conv_pos_embedding_groups
    d.feat_proj_layer_norm = int(harch.feat_proj_layer_norm)
    d.layer_norm_eps = harch.layer_norm_eps
    d.codebook_dim, d.num_clusters = harch.codebook_dim, int(num_clusters)
    d.num_mels = varch.num_mels
    nu = len(varch.upsample_rates)
    if nu > SI_MAX_UPS or len(varch.upsample_kernel_sizes) != nu:
        raise ValueError("unsupported upsample stack")
    d.num_ups = nu
    for i in range(nu):
        d.up_rates[i], d.up_kernels[i] = varch.upsample_rates[i], varch.upsample_kernel_sizes[i]
    d.up_initial_channel = varch.upsample_initial_channel
    nr = len(varch.resblock_kernel_sizes)
    nd = len(varch.resblock_dilation_sizes[0])
    if nr > SI_MAX_RB or nd > SI_MAX_DIL or any(len(x) != nd for x in varch.resblock_dilation_sizes):
        raise ValueError("unsupported resblock shape")
    d.num_rb, d.num_dil = nr, nd
    for j in range(nr):
        d.rb_kernels[j] = varch.resblock_kernel_sizes[j]
        for k in range(nd):
            d.rb_dilations[j][k] = varch.resblock_dilation_sizes[j][k]
    d.encoder_math, d.vocoder_math = SI_MATH[encoder_math], SI_MATH[vocoder_math]
    d.vocoder_chunk = int(vocoder_chunk)
    if str(varch.resblock) not in ("1", "2"):
        raise ValueError(f"resblock={varch.resblock!r}: '1' or '2' (I_ea/hifi_gan/models.py:89)")
    d.resblock_type = int(varch.resblock)
    return d


_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libsi_hip.so and declare the prototypes.  Raises if the library has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} is missing: the HIP library has not been built (run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C speech_inpainting_amd/csrc`).  There is no CPU fallback for the inpainting path.")
    lib = C.CDLL(p)
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.si_version.restype = i32
    lib.si_create.argtypes = [C.POINTER(vp), i32, C.POINTER(ModelDesc)]
    lib.si_destroy.argtypes = [vp]
    lib.si_destroy.restype = None
    lib.si_last_error.argtypes = [vp]
    lib.si_last_error.restype = C.c_char_p
    lib.si_load_weights.argtypes = [vp, vp, sz, C.c_char_p]
    lib.si_alloc_weights.argtypes = [vp]
    lib.si_weights_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    lib.si_weights_check.argtypes = [vp]
    lib.si_workspace_bytes.argtypes = [vp, i32, i32, i32, C.POINTER(sz)]
    lib.si_hubert_forward.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_hubert_forward_padded.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_hubert_forward_varlen.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_codebook_splice_varlen.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, i32, vp, vp]
    lib.si_hifigan_forward_varlen.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_mel_frontend_varlen.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_hubert_extract_features.argtypes = [vp, C.POINTER(ExtractDesc), vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]
    lib.si_code_splice.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp]
    lib.si_codebook_splice.argtypes = [vp, vp, i32, i32, vp, i32, vp, i32, vp, vp]
    lib.si_codebook_splice_labels.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp]
    lib.si_codebook_metrics.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.si_kmeans_assign.argtypes = [vp, vp, C.c_int64, i32, vp, i32, vp, vp, vp]
    lib.si_mel_metrics.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.si_sisdr.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.si_unit_frontend.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, vp, vp]
    lib.si_f0_encoder_weight_floats.argtypes = [vp]
    lib.si_f0_encoder_weight_floats.restype = C.c_size_t
    lib.si_f0_encoder_frames.argtypes = [vp, i32]
    lib.si_f0_encoder_frames.restype = i32
    lib.si_f0_encoder_workspace_bytes.argtypes = [vp, i32, i32]
    lib.si_f0_encoder_workspace_bytes.restype = C.c_size_t
    lib.si_f0_encoder_forward.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, C.c_size_t, vp]
    lib.si_resample_poly.argtypes = [vp, vp, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.si_resample_sinc.argtypes = [vp, vp, vp, i32, i32, C.POINTER(SincFilter), i32, vp, vp]
    lib.si_pcm16.argtypes = [vp, vp, C.c_int64, vp, vp]
    lib.si_extend_mel.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.si_hifigan_forward.argtypes = [vp, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_mel_frames.argtypes = [i32]
    lib.si_mel_workspace_bytes.argtypes = [vp, i32, i32, C.POINTER(sz)]
    lib.si_mel_frontend.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_hubert_forward_spans.argtypes = [vp, vp, C.POINTER(SpanTableStruct), vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_mel_frontend_spans.argtypes = [vp, vp, C.POINTER(SpanTableStruct), vp, i32, i32, i32, vp, vp, sz, vp]
    lib.si_codebook_splice_spans.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, i32, vp, vp]
    lib.si_codebook_splice_labels_spans.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp]
    lib.si_codebook_metrics_spans.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.si_wave_peak.argtypes = [vp, vp, C.POINTER(SpanTableStruct), vp, i32, i32, vp, vp]
    lib.si_gather_windows.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp]
    lib.si_patch_compose.argtypes = [vp, vp, C.POINTER(SpanTableStruct), vp, C.POINTER(PatchTableStruct), vp, i32, vp, i32, i32, vp, vp, vp]
    lib.si_cut_clips.argtypes = [vp, vp, i32, vp, vp, i32, i32, vp, vp]
    lib.si_patch_regions.argtypes = [vp, vp, i32, C.POINTER(RegionTableStruct), vp, i32, vp, vp, vp, vp]
    lib.si_quiet_runs.argtypes = [vp, vp, i32, i32, C.c_float, i32, vp, i32, vp, vp]
    lib.si_patch_rate.argtypes = [vp, vp, i32, i32, i32, C.POINTER(RateTableStruct), vp, i32, vp, C.POINTER(SincFilter), vp, vp]
    lib.si_cut_rate.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, C.POINTER(SincFilter), vp, vp]
    lib.si_quiet_runs_ch.argtypes = [vp, vp, i32, i32, i32, i32, C.c_float, i32, vp, i32, vp, vp]
    lib.si_cut_rate_ch.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, C.POINTER(SincFilter), vp, vp]
    lib.si_patch_rate_ch.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.POINTER(RateTableStruct), vp, i32, vp, C.POINTER(SincFilter), vp, vp]
    lib.si_dead_runs.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, i32, vp, i32, vp, vp, vp]
    lib.si_level_runs.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp, vp, vp]
    lib.si_burst_runs.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp, vp, vp]
    lib.si_cut_pair.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, C.POINTER(SincFilter), C.POINTER(SincFilter), vp, vp, vp]
    lib.si_cut_pair_ch.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, C.POINTER(SincFilter), C.POINTER(SincFilter), vp, vp, vp]
    lib.si_invalid_runs.argtypes = [vp, vp, i32, i32, i32, i32, C.c_float, i32, vp, i32, vp, vp]
    lib.si_cut_rate_valid.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, C.POINTER(SincFilter), C.c_float, vp, vp]
    lib.si_cut_pair_valid.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, C.POINTER(SincFilter), C.POINTER(SincFilter), C.c_float,
                                      vp, vp, vp]
    lib.si_cut_clips_valid.argtypes = [vp, vp, i32, vp, vp, i32, i32, C.c_float, vp, vp]
    lib.si_mend_runs.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp]
    lib.si_impulse_runs.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, i32, vp, i32, vp, vp, vp]
    lib.si_impulse_residual.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.si_plan_weights.argtypes = [C.POINTER(ModelDesc), C.POINTER(sz)]
    lib.si_pack_weights_host.argtypes = [C.POINTER(ModelDesc), vp, sz, C.c_char_p, vp, sz, C.POINTER(sz), C.c_char_p, sz]
    lib.si_num_frames.argtypes = [vp, i32]
    lib.si_vocoder_samples.argtypes = [vp, i32, i32]
    lib.si_debug_capture.argtypes = [vp, C.c_char_p, vp, C.c_long]
    lib.si_debug_size.argtypes = [vp, C.c_char_p]
    lib.si_debug_size.restype = C.c_long
    lib.si_debug_ws_regions.argtypes = [vp, i32, C.POINTER(WsRegion), i32, C.POINTER(i32)]
    lib.si_profile_start.argtypes = [vp, i32]
    lib.si_profile_filter.argtypes = [vp, C.c_char_p]
    lib.si_profile_stop.argtypes = [vp, C.POINTER(ProfileEntry), i32, C.POINTER(i32)]
    for name in EXPORTS:
        if name not in ("si_destroy", "si_last_error", "si_debug_size"):
            getattr(lib, name).restype = i32
    if path is None:
        _lib = lib
    return lib


class NativeError(RuntimeError):
    pass


def plan_weights(desc: ModelDesc):
    """(return code, byte size of the packed blob, message) of si_plan_weights: the descriptor check and the plan, no device needed."""
    lib = load_library()
    n = C.c_size_t(0)
    rc = lib.si_plan_weights(C.byref(desc), C.byref(n))
    return rc, int(n.value), lib.si_last_error(None).decode()


def pack_weights_host(desc: ModelDesc, blob: np.ndarray, index: str, capacity: Optional[int] = None, slack: int = 0):
    """si_pack_weights_host on the (blob, index) pair of checkpoint.flatten_checkpoint, no device needed -> (return code, image as a
    uint8 array of capacity + slack bytes pre-filled with 0xA5, needed, message).  capacity None: what si_plan_weights reports."""
    lib = load_library()
    blob = np.ascontiguousarray(blob)
    if capacity is None:
        rc, capacity, msg = plan_weights(desc)
        if rc != 0:
            return rc, np.zeros(0, np.uint8), 0, msg
    out = np.full(int(capacity) + int(slack), 0xA5, dtype=np.uint8)
    need, err = C.c_size_t(0), C.create_string_buffer(512)
    rc = lib.si_pack_weights_host(C.byref(desc), blob.ctypes.data_as(C.c_void_p), blob.nbytes, index.encode(), out.ctypes.data_as(C.c_void_p),
                                  int(capacity), C.byref(need), err, 512)
    return rc, out, int(need.value), err.value.decode()


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dev(t: torch.Tensor, dtype: torch.dtype, dim: Optional[int] = None, n: Optional[int] = None) -> torch.Tensor:
    """What every entry point asks of a tensor argument: on the GPU, this dtype, contiguous [, this rank] [, this many elements]."""
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and (dim is None or t.dim() == dim) and (n is None or t.numel() == n)
    return t


def _f32(t: torch.Tensor, dim: Optional[int] = None) -> torch.Tensor:
    return _dev(t, torch.float32, dim)


def _i32(t: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    return _dev(t, torch.int32, None, n)


def _i64(t: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    return _dev(t, torch.int64, None, n)


def _sinc_filter(filt: dict):
    """audio.design_kaiser_best's scalars with win / dwin as float64 device tensors -> the si_sinc_filter of the calls that interpolate at
    exact times (si_patch_rate, si_cut_rate, si_cut_pair: time_reg is not read), by reference."""
    win, dwin = filt["win"], filt["dwin"]
    assert win.is_cuda and dwin.is_cuda and win.dtype == dwin.dtype == torch.float64 and win.is_contiguous() and dwin.is_contiguous()
    assert win.numel() == dwin.numel()
    return C.byref(SincFilter(C.sizeof(SincFilter), win.numel(), int(filt["num_table"]), int(filt["step"]), 0, 0, float(filt["scale"]),
                              float(filt.get("ratio", 0.0)), win.data_ptr(), dwin.data_ptr(), None))


class NativeContext:
    """One si_ctx: a model pair bound to one GPU."""

    def __init__(self, desc: ModelDesc, device: torch.device):
        self.lib = load_library()
        if device.type != "cuda":
            raise RuntimeError(f"the HIP path needs a GPU device, got {device} (no CPU fallback)")
        self.device = device
        self.desc = desc
        self._h = C.c_void_p(0)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        rc = self.lib.si_create(C.byref(self._h), idx, C.byref(desc))
        if rc != 0:
            raise NativeError(f"si_create failed ({rc}): {self.lib.si_last_error(None).decode()}")
        self._ws: Optional[torch.Tensor] = None

    def close(self):
        """Frees the context and its packed weight blob.  Any tensor from `weights_tensor()` is a VIEW of that blob and
        must not be used after this call (the holder is dropped here so a stale view cannot be handed out again)."""
        self._wholder = None
        self._ws = None
        self._ws_mel = self._ws_mel_old = None
        if getattr(self, "_h", None) and self._h.value:
            self.lib.si_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise NativeError(f"{what} failed ({rc}): {self.lib.si_last_error(self._h).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- weights
    def load_weights(self, blob: np.ndarray, index: str):
        blob = np.ascontiguousarray(blob)
        self._check(self.lib.si_load_weights(self._h, blob.ctypes.data_as(C.c_void_p), blob.nbytes, index.encode()),
                    "si_load_weights")

    def alloc_weights(self):
        self._check(self.lib.si_alloc_weights(self._h), "si_alloc_weights")

    def weights_check(self):
        """Compare the blob's layout fingerprint with this context's plan (after a broadcast); raises NativeError on a mismatch."""
        self._check(self.lib.si_weights_check(self._h), "si_weights_check")

    def weights_ptr(self):
        """(device address, byte count) of the packed blob as si_weights_device_ptr reports it."""
        p, n = C.c_void_p(0), C.c_size_t(0)
        self._check(self.lib.si_weights_device_ptr(self._h, C.byref(p), C.byref(n)), "si_weights_device_ptr")
        return int(p.value), int(n.value)

    def weights_tensor(self) -> torch.Tensor:
        """The packed device blob as a uint8 tensor VIEW (for the RCCL broadcast): it aliases library-owned memory and
        is valid only while this context is open."""
        p, n = C.c_void_p(0), C.c_size_t(0)
        self._check(self.lib.si_weights_device_ptr(self._h, C.byref(p), C.byref(n)), "si_weights_device_ptr")

        class _Holder:
            pass
        h = _Holder()
        h.__cuda_array_interface__ = {"shape": (n.value,), "typestr": "|u1", "data": (p.value, False), "version": 2}
        self._wholder = h
        t = torch.as_tensor(h, device=self.device)
        if t.data_ptr() != p.value or t.numel() != n.value:      # as_tensor must alias, never copy
            raise NativeError("weights_tensor: torch did not alias the library's weight blob")
        return t

    # ---- shapes / workspace
    def num_frames(self, n: int) -> int:
        return int(self.lib.si_num_frames(self._h, n))

    def mel_frames(self, n22: int) -> int:
        return int(self.lib.si_mel_frames(int(n22)))

    def vocoder_samples(self, tm: int, stretch: bool = True) -> int:
        return int(self.lib.si_vocoder_samples(self._h, tm, int(stretch)))

    def workspace(self, B: int, N: int, Tm: int) -> torch.Tensor:
        need = C.c_size_t(0)
        self._check(self.lib.si_workspace_bytes(self._h, B, N, Tm, C.byref(need)), "si_workspace_bytes")
        if self._ws is None or self._ws.numel() < need.value:
            self._ws = None
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        return self._ws

    # ---- forward calls (all enqueue on torch's current stream)
    def _encoder_call(self, name: str, wav: torch.Tensor, width: int, masks, mid, head=(), sample_len=None) -> torch.Tensor:
        """The encoder entry points: wav (B, N) -> (B, T, width) in the shared workspace.  They differ in the output width and in the
        arguments between `wav` and `B` -- mid(lens) -> that tuple, lens = the HOST lengths `sample_len` of a ragged batch as a pointer
        (None without) -- and `head`, what precedes `wav`.  masks: optional per-clip int32 (B) device tensors."""
        B, N = _f32(wav, 2).shape
        lens = None if sample_len is None else self._host_lens(sample_len, B)
        T = self.num_frames(N)
        if T < 1:
            raise ValueError(f"clip of {N} samples is too short")
        for m in masks:
            assert m is None or _i32(m, B) is m
        out = torch.empty(B, T, width, dtype=torch.float32, device=self.device)
        ws = self.workspace(B, N, 0)
        self._check(getattr(self.lib, name)(self._h, *head, _ptr(wav), *mid(None if lens is None else lens.ctypes.data_as(C.c_void_p)), B, N,
                                            _ptr(out), _ptr(ws), ws.numel(), self._stream()), name)
        return out

    def hubert_forward(self, wav: torch.Tensor, mask_start: Optional[torch.Tensor], mask_len: Optional[torch.Tensor],
                       normalize: bool = True, valid_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        """valid_len (B,) int32 on the device: real samples of each RIGHT-PADDED clip (None: every clip fills its row)."""
        return self._encoder_call("si_hubert_forward_padded", wav, self.desc.codebook_dim, (mask_start, mask_len, valid_len),
                                  lambda _: (_ptr(mask_start), _ptr(mask_len), _ptr(valid_len), int(normalize)))

    @staticmethod
    def _host_lens(lens, B: int):
        """HOST int32 (B) lengths of a ragged batch as a ctypes array (the library reads it during the call only)."""
        a = np.ascontiguousarray(np.asarray(lens, dtype=np.int32).reshape(-1))
        if a.size != B:
            raise ValueError(f"ragged batch: {a.size} lengths for {B} clips")
        return a

    def hubert_forward_varlen(self, wav: torch.Tensor, sample_len, mask_start: Optional[torch.Tensor] = None,
                              mask_len: Optional[torch.Tensor] = None, normalize: bool = True) -> torch.Tensor:
        """RAGGED batch: wav (B, Nmax), clip b = the first sample_len[b] samples of its row (host ints) -> (B, Tmax, D) with zero
        rows past each clip's own frames; every clip's rows equal that clip run alone (si_hubert_forward_varlen)."""
        return self._encoder_call("si_hubert_forward_varlen", wav, self.desc.codebook_dim, (mask_start, mask_len),
                                  lambda lens: (_ptr(mask_start), _ptr(mask_len), lens, int(normalize)), sample_len=sample_len)

    def codebook_splice_varlen(self, feats: torch.Tensor, frame_pos: torch.Tensor, frame_cnt: torch.Tensor, lm: int, mel: torch.Tensor) -> torch.Tensor:
        """As codebook_splice with a per-clip frame count (B,) int32 on the device; labels past a clip's count are -1."""
        B, T, Tm = self._feats_mel(feats, mel)
        labels = torch.empty(B, lm, dtype=torch.int64, device=self.device)
        self._check(self.lib.si_codebook_splice_varlen(self._h, _ptr(feats), B, T, _ptr(_i32(frame_pos, B)), _ptr(_i32(frame_cnt, B)), lm, _ptr(mel), Tm,
                                                       _ptr(labels), self._stream()), "si_codebook_splice_varlen")
        return labels

    def hifigan_forward_varlen(self, mel: torch.Tensor, mel_len, stretch: bool = True) -> torch.Tensor:
        """RAGGED batch: mel (B, D, Tm_max), clip b = its first mel_len[b] frames (host ints) -> (B, Lmax), the first
        vocoder_samples(mel_len[b]) samples of row b equal that clip's waveform alone, the rest is zero."""
        assert mel.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous() and mel.dim() == 3
        B, D, Tm = mel.shape
        assert D == self.desc.num_mels
        lens = self._host_lens(mel_len, B)
        L = self.vocoder_samples(Tm, stretch)
        out = torch.empty(B, L, dtype=torch.float32, device=self.device)
        ws = self.workspace(B, 0, Tm)
        self._check(self.lib.si_hifigan_forward_varlen(self._h, _ptr(mel), lens.ctypes.data_as(C.c_void_p), B, Tm, int(stretch), _ptr(out),
                                                       _ptr(ws), ws.numel(), self._stream()), "si_hifigan_forward_varlen")
        return out

    def mel_frontend_varlen(self, wave22: torch.Tensor, sample_len, mask_start: Optional[torch.Tensor] = None,
                            mask_end: Optional[torch.Tensor] = None, normalize: bool = True) -> torch.Tensor:
        """RAGGED batch: wave22 (B, N22max), clip b = its first sample_len[b] samples -> (B, 80, Tm_max), zero frames past a clip's own."""
        return self._mel_call("si_mel_frontend_varlen", wave22, (mask_start, mask_end),
                              lambda lens: (_ptr(mask_start), _ptr(mask_end), lens, int(normalize)), sample_len)

    # ---- several gaps per clip (si_span_table / frame tables)
    def hubert_forward_spans(self, wav: torch.Tensor, spans: "SpanTable", normalize: bool = True, sample_len=None) -> torch.Tensor:
        """hubert_forward / hubert_forward_varlen (sample_len: host ints) with every span of `spans` (16 kHz samples) zeroed."""
        t = spans.struct()
        return self._encoder_call("si_hubert_forward_spans", wav, self.desc.codebook_dim, (), lambda lens: (C.byref(t), lens, int(normalize)),
                                  sample_len=sample_len)

    def mel_frontend_spans(self, wave22: torch.Tensor, spans: "SpanTable", normalize: bool = True, sample_len=None) -> torch.Tensor:
        """mel_frontend / mel_frontend_varlen (sample_len: host ints) with every span of `spans` (22.05 kHz samples) zeroed."""
        t = spans.struct()
        return self._mel_call("si_mel_frontend_spans", wave22, (), lambda lens: (C.byref(t), lens, int(normalize)), sample_len)

    # ---- patch mode
    def wave_peak(self, wave22: torch.Tensor, spans: Optional["SpanTable"] = None, sample_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        """max |x| per clip with the spans zeroed: the divisor of mel_frontend's normalisation (si_wave_peak).  sample_len: DEVICE int32 (B)."""
        assert wave22.is_cuda and wave22.dtype == torch.float32 and wave22.dim() == 2 and wave22.is_contiguous()
        B, N = wave22.shape
        assert sample_len is None or (sample_len.is_cuda and sample_len.dtype == torch.int32 and sample_len.numel() == B and sample_len.is_contiguous())
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        t = None if spans is None else spans.struct()
        self._check(self.lib.si_wave_peak(self._h, _ptr(wave22), None if t is None else C.byref(t), _ptr(sample_len), B, N, _ptr(out), self._stream()),
                    "si_wave_peak")
        return out

    @staticmethod
    def window_words(wins) -> np.ndarray:
        """(clip, w0, w1) triples -> the int32 words [clip (W) | w0 (W) | w1 (W)] si_gather_windows reads."""
        return np.array([[int(w[j]) for w in wins] for j in range(3)], dtype=np.int32).reshape(-1)

    def gather_windows(self, ext: torch.Tensor, wins, wmax: Optional[int] = None, tab=None) -> torch.Tensor:
        """ext (B, D, Tout) + wins = (clip, w0, w1) triples -> (W, D, Wmax), zero past each window's own frames (si_gather_windows).
        tab = (host int32 numpy view, device int32 tensor) holding `window_words(wins)` ALREADY (a caller that staged the table with
        its other tables, one copy); default: built and copied here."""
        assert ext.is_cuda and ext.dtype == torch.float32 and ext.dim() == 3 and ext.is_contiguous() and ext.shape[1] == self.desc.num_mels
        B, D, Tout = ext.shape
        W = len(wins)
        if tab is None:
            host = self.window_words(wins)
            dev = torch.from_numpy(host).to(self.device, non_blocking=True)
        else:
            host, dev = tab
            assert host.size == 3 * W and dev.numel() == 3 * W and dev.dtype == torch.int32
        if wmax is None:
            wmax = max(int(w1) - int(w0) for _, w0, w1 in wins)
        out = torch.empty(W, D, int(wmax), dtype=torch.float32, device=self.device)
        self._check(self.lib.si_gather_windows(self._h, _ptr(ext), B, Tout, host.ctypes.data_as(C.c_void_p), _ptr(dev), W, int(wmax), _ptr(out),
                                               self._stream()), "si_gather_windows")
        return out

    def patch_compose(self, orig: torch.Tensor, spans: "SpanTable", patch: "PatchTable", gen: Optional[torch.Tensor], gain: Optional[torch.Tensor] = None,
                      sample_len=None, f32: bool = True, pcm: bool = False, out: Optional[torch.Tensor] = None, out_pcm: Optional[torch.Tensor] = None):
        """orig (B, N22) with the generated rows gen (W, Lrow) cross-faded in around every span (si_patch_compose) -> (fp32 or None,
        int16 or None), each (B, N22).  gain (B,) fp32 on the device or None; sample_len: host ints of a ragged batch."""
        assert orig.is_cuda and orig.dtype == torch.float32 and orig.dim() == 2 and orig.is_contiguous()
        B, N = orig.shape
        assert gen is None or (gen.is_cuda and gen.dtype == torch.float32 and gen.dim() == 2 and gen.is_contiguous() and gen.shape[0] == patch.W)
        assert gain is None or (gain.is_cuda and gain.dtype == torch.float32 and gain.numel() == B and gain.is_contiguous())
        lens = None if sample_len is None else self._host_lens(sample_len, B)
        if f32 and out is None:
            out = torch.empty(B, N, dtype=torch.float32, device=self.device)
        if pcm and out_pcm is None:
            out_pcm = torch.empty(B, N, dtype=torch.int16, device=self.device)
        for o, dt in ((out, torch.float32), (out_pcm, torch.int16)):
            assert o is None or (o.is_cuda and o.dtype == dt and o.is_contiguous() and o.numel() == B * N)
        ts, tp = spans.struct(), patch.struct()
        self._check(self.lib.si_patch_compose(self._h, _ptr(orig), C.byref(ts), None if lens is None else lens.ctypes.data_as(C.c_void_p), C.byref(tp),
                                              _ptr(gen), 0 if gen is None else gen.shape[1], _ptr(gain), B, N, _ptr(out), _ptr(out_pcm), self._stream()),
                    "si_patch_compose")
        return out, out_pcm

    # ---- long recordings
    def _start_table(self, starts, empty: bool = False):
        """starts (host ints) -> (host int32, device int32): what a feed validates and what its kernel reads; a value outside int32 is
        clipped to its ends, which every feed refuses.  No device copy of an empty table unless `empty`."""
        host = np.ascontiguousarray(np.asarray(list(starts), dtype=np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32))
        return host, torch.from_numpy(host).to(self.device, non_blocking=True) if host.size or empty else None

    def _clip_rows(self, out: Optional[torch.Tensor], Cn: int, L: int) -> torch.Tensor:
        """out, or a new tensor: (Cn, max(L, 0)) fp32 on the device."""
        if out is None:
            out = torch.empty(Cn, max(L, 0), dtype=torch.float32, device=self.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == Cn * max(L, 0)
        return out

    def cut_clips(self, src: torch.Tensor, starts, L: int, out: Optional[torch.Tensor] = None, ceiling: Optional[float] = None) -> torch.Tensor:
        """src (n,) fp32 + starts (host ints) -> (C, L): row c = src[starts[c] : starts[c] + L] (si_cut_clips).  A start table that
        leaves the source is refused before the launch.  ceiling: a sample that is invalid(., ceiling) is copied as +0.0
        (si_cut_clips_valid)."""
        assert src.is_cuda and src.dtype == torch.float32 and src.dim() == 1 and src.is_contiguous()
        host, dev = self._start_table(starts, empty=True)
        Cn, L = host.size, int(L)
        out = self._clip_rows(out, Cn, L)
        entry = "si_cut_clips" if ceiling is None else "si_cut_clips_valid"
        self._check(getattr(self.lib, entry)(self._h, _ptr(src), min(src.numel(), 2 ** 31 - 1), host.ctypes.data_as(C.c_void_p), _ptr(dev), Cn, L,
                                             *(() if ceiling is None else (float(ceiling),)), _ptr(out), self._stream()), entry)
        return out

    def patch_regions(self, orig: torch.Tensor, table: "RegionTable", gen: Optional[torch.Tensor], gain: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, out_pcm: Optional[torch.Tensor] = None) -> None:
        """The blended samples of `table`'s regions written IN PLACE into out (N22) fp32 and / or out_pcm (N22) int16, which hold the
        caller's copy of the recording `orig` (N22) everywhere else (si_patch_regions).  gen (W, Lrow); gain (C,) fp32 or None."""
        assert orig.is_cuda and orig.dtype == torch.float32 and orig.dim() == 1 and orig.is_contiguous()
        N = orig.numel()
        assert gen is None or (gen.is_cuda and gen.dtype == torch.float32 and gen.dim() == 2 and gen.is_contiguous() and gen.shape[0] == table.W)
        assert gain is None or (gain.is_cuda and gain.dtype == torch.float32 and gain.numel() == table.C and gain.is_contiguous())
        for o, dt in ((out, torch.float32), (out_pcm, torch.int16)):
            assert o is None or (o.is_cuda and o.dtype == dt and o.is_contiguous() and o.numel() == N and o.data_ptr() != orig.data_ptr())
        t = table.struct()
        self._check(self.lib.si_patch_regions(self._h, _ptr(orig), min(N, 2 ** 31 - 1), C.byref(t), _ptr(gen), 0 if gen is None else gen.shape[1], _ptr(gain), _ptr(out),
                                              _ptr(out_pcm), self._stream()), "si_patch_regions")

    # ---- repair at the file's own sample rate
    @staticmethod
    def _interleaved(x: torch.Tensor, channel: Optional[int]) -> Tuple[int, int]:
        """(sample times, channels) of x as a call with `channel` takes it: (n,) for channel None, else (n, ch) interleaved (DESIGN.md
        4.18).  Channel counts and indices the C ABI would refuse are passed on, so that it is the one that refuses them."""
        assert x.is_cuda and x.dtype in (torch.float32, torch.int16, torch.uint8) and x.is_contiguous()
        byte = int(x.dtype == torch.uint8)                             # packed 24-bit: a trailing dimension of the 3 bytes
        assert not byte or x.shape[-1] == 3
        if channel is None:
            assert x.dim() == 1 + byte
            return min(x.shape[0], 2 ** 31 - 1), 0
        assert x.dim() == 2 + byte
        return min(x.shape[0], 2 ** 31 - 1), x.shape[1]

    @staticmethod
    def _sample_format(x: torch.Tensor) -> int:
        """The file-typed calls' is_pcm16 argument for x: SI_SAMPLE_F32 / _S16 / _S24."""
        return SAMPLE_S24 if x.dtype == torch.uint8 else SAMPLE_S16 if x.dtype == torch.int16 else SAMPLE_F32

    def patch_rate(self, orig: torch.Tensor, sr: int, table: "RateTable", gen: Optional[torch.Tensor], filt: dict, out: torch.Tensor,
                   gain: Optional[torch.Tensor] = None, channel: Optional[int] = None) -> None:
        """The blended samples of `table`'s regions written IN PLACE into out (n_file,), which holds the caller's copy of the file
        `orig` (n_file,) at `sr` Hz everywhere else (si_patch_rate).  orig / out: fp32 or int16, the same type, device views that may
        start anywhere.  gen (W, Lrow) fp32 at 22.05 kHz; gain (C,) fp32 or None; filt: audio.design_kaiser_best(22050, sr, .) with win /
        dwin as float64 device tensors.
        channel = c: orig / out are (n_file, ch) interleaved and only channel c of out is written, the table's spans and chunks being
        sample times of that channel (si_patch_rate_ch); the table may name windows and contexts of other channels."""
        n_file, ch = self._interleaved(orig, channel)
        assert out.is_cuda and out.dtype == orig.dtype and out.shape == orig.shape and out.is_contiguous()
        assert gen is None or (gen.is_cuda and gen.dtype == torch.float32 and gen.dim() == 2 and gen.is_contiguous() and gen.shape[0] == table.W)
        assert gain is None or (gain.is_cuda and gain.dtype == torch.float32 and gain.numel() == table.C and gain.is_contiguous())
        t = table.struct()
        entry, file = self._file_entry("si_patch_rate", orig, n_file, ch, channel)
        self._check(getattr(self.lib, entry)(*file, int(sr), C.byref(t), _ptr(gen), 0 if gen is None else gen.shape[1], _ptr(gain), _sinc_filter(filt),
                                             _ptr(out), self._stream()), entry)

    def _file_entry(self, name: str, x: torch.Tensor, n_file: int, ch: int, channel: Optional[int], ceiling: Optional[float] = None):
        """(the C entry point, its leading arguments) of a file-typed call on x as _interleaved read it: `name` for a file without
        `channel`, `name`_ch with one; under a ceiling the one entry `name`_valid, which takes the file without `channel` as channels = 1,
        channel = 0."""
        file = (self._h, _ptr(x), self._sample_format(x), n_file)
        if ceiling is not None:
            return name + "_valid", file + ((ch, int(channel)) if channel is not None else (1, 0))
        return (name + "_ch", file + (ch, int(channel))) if channel is not None else (name, file)

    # ---- context clips cut at the file's own sample rate
    def cut_rate(self, x: torch.Tensor, sr: int, starts, L: int, filt: dict, out: Optional[torch.Tensor] = None,
                 channel: Optional[int] = None, ceiling: Optional[float] = None) -> torch.Tensor:
        """x (n_file,) at `sr` Hz, fp32 or int16, a device view that may start anywhere + starts (host ints, 22.05 kHz samples) ->
        (C, L) fp32: row c = samples [starts[c], starts[c] + L) of the recording's 22.05 kHz axis, interpolated at the exact time
        j * sr / 22050 straight from the file's samples (si_cut_rate).  filt: audio.design_kaiser_best(sr, 22050, .) with win / dwin as
        float64 device tensors.  A start table that leaves the recording's ceil(n_file * 22050 / sr) samples is refused before the
        launch.  channel = c: x is (n_file, ch) interleaved and the clips are cut from its channel c (si_cut_rate_ch).  ceiling: see
        cut_rate_valid (si_cut_rate_valid)."""
        n_file, ch = self._interleaved(x, channel)
        host, dev = self._start_table(starts)
        Cn, L = host.size, int(L)
        out = self._clip_rows(out, Cn, L)
        entry, file = self._file_entry("si_cut_rate", x, n_file, ch, channel, ceiling)
        self._check(getattr(self.lib, entry)(*file, int(sr), host.ctypes.data_as(C.c_void_p), _ptr(dev), Cn, L, _sinc_filter(filt),
                                             *(() if ceiling is None else (float(ceiling),)), C.c_void_p(out.data_ptr()), self._stream()), entry)
        return out

    # ---- both clip sets of a pass cut straight from the file, in one launch
    def cut_pair(self, x: torch.Tensor, sr: int, frames, L22: int, L16: int, filt22: dict, filt16: Optional[dict],
                 out22: Optional[torch.Tensor] = None, out16: Optional[torch.Tensor] = None, channel: Optional[int] = None,
                 ceiling: Optional[float] = None):
        """x (n_file,) at `sr` Hz, fp32 or int16, a device view that may start anywhere + frames (host ints, 20 ms frames) ->
        (out22 (C, L22), out16 (C, L16)) fp32: row c = 22.05 kHz samples 441 frames[c] + [0, L22) -- si_cut_rate's bytes -- and 16 kHz
        samples 320 frames[c] + [0, L16), interpolated at the exact time j * sr / 16000 straight from the file's samples, zero at and past
        the recording's ceil(n_file * 16000 / sr) samples (si_cut_pair: one launch for both).  filt22 / filt16:
        audio.design_kaiser_best(sr, 22050 / 16000, .) with win / dwin as float64 device tensors; at sr = 16000 filt16 is None and the
        16 kHz rows are the file's own samples.  channel = c: x is (n_file, ch) interleaved (si_cut_pair_ch).  ceiling: see
        cut_pair_valid (si_cut_pair_valid)."""
        n_file, ch = self._interleaved(x, channel)
        host, dev = self._start_table(frames)
        Cn, L22, L16 = host.size, int(L22), int(L16)
        out22, out16 = self._clip_rows(out22, Cn, L22), self._clip_rows(out16, Cn, L16)
        entry, file = self._file_entry("si_cut_pair", x, n_file, ch, channel, ceiling)
        self._check(getattr(self.lib, entry)(*file, int(sr), host.ctypes.data_as(C.c_void_p), _ptr(dev), Cn, L22, L16, _sinc_filter(filt22),
                                             None if filt16 is None else _sinc_filter(filt16), *(() if ceiling is None else (float(ceiling),)),
                                             C.c_void_p(out22.data_ptr()), C.c_void_p(out16.data_ptr()), self._stream()), entry)
        return out22, out16

    # ---- dropout detection; one call shape for every detector (4.34)
    def _runs_call(self, name: str, x: torch.Tensor, args, min_len, max_runs, runs, n_runs, channel, threshold_out=None, takes_channels: bool = True,
                   takes_threshold_out: bool = True):
        """The run-list entry point `name`: (ctx, x, format, n, [channels, channel,] *args, min_len, runs, max_runs, n_runs, [threshold_out,]
        stream).  `args` are the detector's own, already int / float.  Allocates runs (max_runs, 2) and n_runs (1,) when they are not given;
        an x without `channel` is the one-channel file, channels = 1.  -> (runs, n_runs)."""
        n, ch = self._interleaved(x, channel)
        max_runs = int(max_runs)
        if runs is None and max_runs > 0:
            runs = torch.empty(max_runs, 2, dtype=torch.int32, device=self.device)
        if n_runs is None:
            n_runs = torch.empty(1, dtype=torch.int32, device=self.device)
        assert runs is None or (runs.is_cuda and runs.dtype == torch.int32 and runs.is_contiguous() and runs.numel() >= 2 * max_runs)
        assert n_runs.is_cuda and n_runs.dtype == torch.int32 and n_runs.numel() == 1
        assert threshold_out is None or (threshold_out.is_cuda and threshold_out.dtype == torch.float32 and threshold_out.numel() == 1)
        file = (ch if channel is not None else 1, int(channel) if channel is not None else 0) if takes_channels else ()
        out = (_ptr(threshold_out),) if takes_threshold_out else ()
        self._check(getattr(self.lib, name)(self._h, _ptr(x), self._sample_format(x), n, *file, *args, int(min_len), _ptr(runs), max_runs, _ptr(n_runs),
                                            *out, self._stream()), name)
        return runs, n_runs

    def quiet_runs(self, x: torch.Tensor, threshold: float = 0.0, min_len: int = 1, max_runs: int = 65536, runs: Optional[torch.Tensor] = None,
                   n_runs: Optional[torch.Tensor] = None, channel: Optional[int] = None):
        """x (n,) fp32 or int16 on the device (a view may start anywhere) -> (runs (max_runs, 2) int32, n_runs (1,) int32), both on
        the device: the maximal runs of |x| <= threshold of at least min_len samples as (start, len) rows sorted by start, and how
        many there are in all (si_quiet_runs).  Rows at and past min(n_runs, max_runs) are not written; max_runs = 0 counts only.
        channel = c: x is (n, ch) interleaved and the runs are channel c's, in sample times; channel = -1: the runs of sample times at
        which EVERY channel is quiet (si_quiet_runs_ch)."""
        name = "si_quiet_runs_ch" if channel is not None else "si_quiet_runs"          # the mono entry point has no channels
        return self._runs_call(name, x, (float(threshold),), min_len, max_runs, runs, n_runs, channel, takes_channels=channel is not None,
                               takes_threshold_out=False)

    # ---- held-sample and peak-relative dropouts
    def dead_runs(self, x: torch.Tensor, kind: int = DEAD_QUIET | DEAD_HELD, threshold: float = 0.0, rel_threshold: float = 0.0,
                  held_tol: float = 0.0, min_len: int = 1, max_runs: int = 65536, runs: Optional[torch.Tensor] = None,
                  n_runs: Optional[torch.Tensor] = None, channel: Optional[int] = None, threshold_out: Optional[torch.Tensor] = None):
        """quiet_runs with si_dead_runs' predicate: a sample is dead when |x| <= T = max(threshold, rel_threshold * peak) (kind &
        DEAD_QUIET) or when it is within held_tol of a neighbour of its own channel (kind & DEAD_HELD).  x (n,) or, with `channel`,
        (n, ch) interleaved; -> (runs, n_runs) as quiet_runs returns them.  threshold_out: a device fp32 word that receives T.
        n_runs may be one word of a longer int32 tensor (the engine reads count and T in one copy)."""
        return self._runs_call("si_dead_runs", x, (int(kind), float(threshold), float(rel_threshold), float(held_tol)), min_len, max_runs, runs, n_runs,
                               channel, threshold_out)

    # ---- dropouts by windowed RMS level
    def level_runs(self, x: torch.Tensor, half: int = 0, threshold: float = 0.0, rel_threshold: float = 0.0, min_len: int = 1,
                   max_runs: int = 65536, runs: Optional[torch.Tensor] = None, n_runs: Optional[torch.Tensor] = None,
                   channel: Optional[int] = None, threshold_out: Optional[torch.Tensor] = None):
        """dead_runs with si_level_runs' predicate: a sample is dead when a window of 2 * half + 1 samples of its channel within half
        samples of it has an RMS level of at most T = max(threshold, rel_threshold * peak) and no NaN or inf in it.  x, channel, runs,
        n_runs and threshold_out are dead_runs'; -> (runs, n_runs)."""
        return self._runs_call("si_level_runs", x, (int(half), float(threshold), float(rel_threshold)), min_len, max_runs, runs, n_runs, channel,
                               threshold_out)

    # ---- corrupted blocks by second-difference level
    def burst_runs(self, x: torch.Tensor, half: int = 0, threshold: float = 0.0, rel_threshold: float = 0.0, min_len: int = 1,
                   max_runs: int = 65536, runs: Optional[torch.Tensor] = None, n_runs: Optional[torch.Tensor] = None,
                   channel: Optional[int] = None, threshold_out: Optional[torch.Tensor] = None):
        """level_runs with si_burst_runs' predicate: a sample is dead when a window of 2 * half + 1 second differences x[k - 1] -
        2 x[k] + x[k + 1] of its channel within half samples of it has an RMS level of AT LEAST T = max(threshold, rel_threshold *
        peak) and no NaN or inf under it.  x, channel, runs, n_runs and threshold_out are dead_runs'; -> (runs, n_runs)."""
        return self._runs_call("si_burst_runs", x, (int(half), float(threshold), float(rel_threshold)), min_len, max_runs, runs, n_runs, channel,
                               threshold_out)

    # ---- NaN, inf and out-of-range samples
    def invalid_runs(self, x: torch.Tensor, ceiling: float = float("inf"), min_len: int = 1, max_runs: int = 65536,
                     runs: Optional[torch.Tensor] = None, n_runs: Optional[torch.Tensor] = None, channel: Optional[int] = None):
        """dead_runs with si_invalid_runs' predicate: a sample is dead when its VALUE is invalid -- NaN, +-inf or |x| > ceiling (fp32);
        |x| > ceiling in the file's own steps for int16 / packed 24-bit PCM, so only under a finite ceiling.  ceiling > 0, +inf (the
        default) = "not finite".  x, channel (-1: every channel invalid), runs and n_runs are dead_runs'; no threshold comes back.
        -> (runs, n_runs)."""
        return self._runs_call("si_invalid_runs", x, (float(ceiling),), min_len, max_runs, runs, n_runs, channel, takes_threshold_out=False)

    # ---- clicks and pops by locally scaled AR prediction error
    def impulse_runs(self, x: torch.Tensor, order: int = 16, half: int = 256, guard: int = 4, pad: int = 2, ratio: float = 10.0,
                     threshold: float = 0.0, rel_threshold: float = 0.0, min_len: int = 1, max_runs: int = 65536,
                     runs: Optional[torch.Tensor] = None, n_runs: Optional[torch.Tensor] = None, channel: Optional[int] = None,
                     threshold_out: Optional[torch.Tensor] = None):
        """level_runs with si_impulse_runs' predicate: a sample is dead when a sample within `pad` of it is HOT -- its squared prediction
        error under an AR model of order `order`, fitted per block of 512 samples, is above T^2, T = max(threshold, rel_threshold *
        peak), and above ratio^2 times the mean squared prediction error of the samples within `half` of it, `guard` samples on either
        side left out.  x, channel, runs, n_runs and threshold_out are dead_runs'; -> (runs, n_runs)."""
        return self._runs_call("si_impulse_runs", x, (int(order), int(half), int(guard), int(pad), float(ratio), float(threshold), float(rel_threshold)),
                               min_len, max_runs, runs, n_runs, channel, threshold_out)

    def impulse_residual(self, x: torch.Tensor, order: int = 16, channel: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The prediction error si_impulse_runs judges, sample by sample (si_impulse_residual): x (n,) or, with channel = c >= 0, channel c
        of the interleaved (n, ch) file -> e (n,) device float64, 0.0 below `order` and NaN at a sample of a block whose fit window
        holds a NaN or an inf."""
        n, ch = self._interleaved(x, channel)
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=self.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == n
        self._check(self.lib.si_impulse_residual(self._h, _ptr(x), self._sample_format(x), n, ch if channel is not None else 1,
                                                 int(channel) if channel is not None else 0, int(order), _ptr(out), self._stream()),
                    "si_impulse_residual")
        return out

    # ---- short runs mended in place by least-squares AR interpolation
    def mend_runs(self, x: torch.Tensor, runs: Optional[torch.Tensor], max_len: int = 64, order: int = 32, context: int = 512,
                  status: Optional[torch.Tensor] = None, channel: Optional[int] = None, n_runs: Optional[int] = None) -> torch.Tensor:
        """The rows (start, len) of `runs` -- device int32 (R, 2), sorted and disjoint, as the detectors return them -- of at most max_len
        samples filled IN PLACE in x by least-squares AR interpolation of order `order` over `context` intact samples on either side
        (si_mend_runs).  x (n,) fp32 / int16, (n, 3) packed 24-bit, or with channel = c >= 0 the interleaved (n, ch[, 3]) file of which
        only channel c is read and written; a device view may start anywhere.  -> status, device int32 (R,): MEND_* per row; only
        MEND_AR and MEND_LINE rows were written, and only their own samples.  No rows: nothing is launched."""
        n, ch = self._interleaved(x, channel)
        R = (0 if runs is None else runs.shape[0]) if n_runs is None else int(n_runs)
        assert runs is None or (runs.is_cuda and runs.dtype == torch.int32 and runs.is_contiguous() and runs.numel() >= 2 * R)
        if status is None:
            status = torch.empty(max(R, 0), dtype=torch.int32, device=self.device)
        assert status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() >= R
        self._check(self.lib.si_mend_runs(self._h, _ptr(x), self._sample_format(x), n, ch if channel is not None else 1,
                                          int(channel) if channel is not None else 0, _ptr(runs), R, int(max_len), int(order), int(context),
                                          _ptr(status), self._stream()), "si_mend_runs")
        return status

    def cut_rate_valid(self, x: torch.Tensor, sr: int, starts, L: int, filt: dict, ceiling: float, out: Optional[torch.Tensor] = None,
                       channel: Optional[int] = None) -> torch.Tensor:
        """cut_rate with a file sample that is invalid(., ceiling) -- NaN, +-inf, |x| > ceiling in the file's own units -- staged as +0.0
        (si_cut_rate_valid): byte for byte cut_rate on the file with those samples replaced by +0.0, without that copy.  channel = c:
        x is (n_file, ch) interleaved; None: the mono file (channels = 1 of the one C entry)."""
        return self.cut_rate(x, sr, starts, L, filt, out=out, channel=channel, ceiling=float(ceiling))

    def cut_pair_valid(self, x: torch.Tensor, sr: int, frames, L22: int, L16: int, filt22: dict, filt16: Optional[dict], ceiling: float,
                       out22: Optional[torch.Tensor] = None, out16: Optional[torch.Tensor] = None, channel: Optional[int] = None):
        """cut_pair with a file sample that is invalid(., ceiling) staged as +0.0 (si_cut_pair_valid): both outputs are cut_pair's on the
        file with those samples replaced by +0.0, the unfiltered 16 kHz row of a 16 kHz file included.  channel as cut_rate_valid's."""
        return self.cut_pair(x, sr, frames, L22, L16, filt22, filt16, out22=out22, out16=out16, channel=channel, ceiling=float(ceiling))

    def cut_clips_valid(self, src: torch.Tensor, starts, L: int, ceiling: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """cut_clips with a sample that is invalid(., ceiling) copied as +0.0 (si_cut_clips_valid); every other sample keeps its bits."""
        return self.cut_clips(src, starts, L, out=out, ceiling=float(ceiling))

    @staticmethod
    def _feats_mel(feats: torch.Tensor, mel: torch.Tensor):
        """feats (B, T, D) and the mel (B, D, Tm) it is spliced into -> B, T, Tm."""
        B, T, D = _f32(feats, 3).shape
        assert _f32(mel, 3).shape[0] == B and mel.shape[1] == D
        return B, T, mel.shape[2]

    @staticmethod
    def _frame_table(frame_clip: torch.Tensor, frame_pos: torch.Tensor) -> int:
        F = frame_clip.numel()
        assert _i32(frame_clip, F).dim() == 1 and _i32(frame_pos, F).dim() == 1
        return F

    def _metrics_out(self, *shape: int):
        """loss (1,), loss_terms, pred_labels (int64) and cos_pred_target of a codebook_metrics call, the last three of `shape`."""
        f32 = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=self.device)
        return f32(1), f32(*shape), torch.empty(*shape, dtype=torch.int64, device=self.device), f32(*shape)

    def codebook_splice_spans(self, feats: torch.Tensor, frame_clip: torch.Tensor, frame_pos: torch.Tensor, mel: torch.Tensor) -> torch.Tensor:
        """In-place splice into `mel` (B, D, Tm) of the frames of a frame table (clip, frame: int32 (F) each); labels (F,) int64."""
        B, T, Tm = self._feats_mel(feats, mel)
        F = self._frame_table(frame_clip, frame_pos)
        labels = torch.empty(F, dtype=torch.int64, device=self.device)
        self._check(self.lib.si_codebook_splice_spans(self._h, _ptr(feats), B, T, _ptr(frame_clip), _ptr(frame_pos), F, _ptr(mel), Tm,
                                                      _ptr(labels), self._stream()), "si_codebook_splice_spans")
        return labels

    def codebook_splice_labels_spans(self, labels: torch.Tensor, frame_clip: torch.Tensor, frame_pos: torch.Tensor, mel: torch.Tensor) -> None:
        """In-place splice of the raw centroids of GIVEN labels (F,) int64 at the frames of a frame table."""
        F = self._frame_table(frame_clip, frame_pos)
        self._check(self.lib.si_codebook_splice_labels_spans(self._h, _ptr(_i64(labels, F)), _f32(mel, 3).shape[0], _ptr(frame_clip), _ptr(frame_pos), F,
                                                             _ptr(mel), mel.shape[2], self._stream()), "si_codebook_splice_labels_spans")

    def codebook_metrics_spans(self, feats: torch.Tensor, frame_clip: torch.Tensor, frame_pos: torch.Tensor, target: torch.Tensor):
        """-> (loss (1,), loss_terms (F,), pred_labels (F,) int64, cos_pred_target (F,)) over the frames of a frame table."""
        B, T, D = _f32(feats, 3).shape
        F = self._frame_table(frame_clip, frame_pos)
        loss, terms, pred, cpt = self._metrics_out(F)
        self._check(self.lib.si_codebook_metrics_spans(self._h, _ptr(feats), B, T, _ptr(frame_clip), _ptr(frame_pos), F, _ptr(_i64(target, F)),
                                                       _ptr(terms), _ptr(loss), _ptr(pred), _ptr(cpt), self._stream()), "si_codebook_metrics_spans")
        return loss, terms, pred, cpt

    def hubert_extract_features(self, wav: torch.Tensor, output_layer: int, normalize="layer_norm",
                                mask_start: Optional[torch.Tensor] = None, mask_len: Optional[torch.Tensor] = None,
                                pre_mask_add: Optional[torch.Tensor] = None) -> torch.Tensor:
        """wav (B, N) fp32 -> (B, T, H) fp32: the hidden state after `output_layer` transformer layers (fairseq
        `extract_features(output_layer=...)`, I_da/src/hubert_feature_reader.py:60-65).  normalize: "layer_norm" (I_da:
        F.layer_norm over the clip, eps 1e-5), "processor" (I_ea: eps 1e-7) or None.  mask_start / mask_len int32 (B) and
        pre_mask_add float64 (B): `(y + add) * mask` in front of it (I_da/scripts/inpainting.py:186-192)."""
        assert pre_mask_add is None or _dev(pre_mask_add, torch.float64, None, wav.shape[0]) is pre_mask_add
        if normalize not in NORMALIZE_MODES:
            raise ValueError(f"normalize={normalize!r}: expected one of {list(NORMALIZE_MODES)}")
        x = ExtractDesc(C.sizeof(ExtractDesc), int(output_layer), NORMALIZE_MODES[normalize], 0)
        return self._encoder_call("si_hubert_extract_features", wav, self.desc.hidden_size, (mask_start, mask_len),
                                  lambda _: (_ptr(mask_start), _ptr(mask_len), _ptr(pre_mask_add)), head=(C.byref(x),))

    def code_splice(self, code_clean: torch.Tensor, code_masked: torch.Tensor, first: torch.Tensor, last: torch.Tensor) -> torch.Tensor:
        """(B, T) int64 unit series of the clean and the corrupted clip -> the corrupted clip's units inside frames
        [first[b], last[b]), the clean clip's elsewhere (I_da/scripts/inpainting.py:209-214)."""
        for c in (code_clean, code_masked):
            assert c.is_cuda and c.dtype == torch.int64 and c.dim() == 2 and c.is_contiguous()
        assert code_clean.shape == code_masked.shape
        B, T = code_clean.shape
        for m in (first, last):
            assert m.is_cuda and m.dtype == torch.int32 and m.numel() == B and m.is_contiguous()
        out = torch.empty_like(code_masked)
        self._check(self.lib.si_code_splice(self._h, _ptr(code_clean), _ptr(code_masked), _ptr(first), _ptr(last), B, T, _ptr(out),
                                            self._stream()), "si_code_splice")
        return out

    def codebook_splice(self, feats: torch.Tensor, frame_pos: torch.Tensor, lm: int, mel: torch.Tensor) -> torch.Tensor:
        """In-place splice into `mel` (B, D, Tm); returns labels (B, Lm) int64."""
        B, T, Tm = self._feats_mel(feats, mel)
        labels = torch.empty(B, lm, dtype=torch.int64, device=self.device)
        self._check(self.lib.si_codebook_splice(self._h, _ptr(feats), B, T, _ptr(_i32(frame_pos, B)), lm, _ptr(mel), Tm,
                                                _ptr(labels), self._stream()), "si_codebook_splice")
        return labels

    def codebook_splice_labels(self, labels: torch.Tensor, frame_pos: torch.Tensor, mel: torch.Tensor) -> None:
        """In-place splice of the raw centroids of GIVEN labels (B, Lm) int64 into `mel` (B, D, Tm)."""
        assert _i64(labels).dim() == 2
        B, lm = labels.shape
        assert _f32(mel, 3).shape[0] == B
        self._check(self.lib.si_codebook_splice_labels(self._h, _ptr(labels), B, _ptr(_i32(frame_pos, B)), lm, _ptr(mel), mel.shape[2],
                                                       self._stream()), "si_codebook_splice_labels")

    def codebook_metrics(self, feats: torch.Tensor, frame_pos: torch.Tensor, lm: int, target: torch.Tensor):
        """-> (loss (1,), loss_terms (B, Lm), pred_labels (B, Lm) int64, cos_pred_target (B, Lm))."""
        B, T, D = _f32(feats, 3).shape
        assert tuple(_i64(target).shape) == (B, lm)
        loss, terms, pred, cpt = self._metrics_out(B, lm)
        self._check(self.lib.si_codebook_metrics(self._h, _ptr(feats), B, T, _ptr(_i32(frame_pos)), lm, _ptr(target), _ptr(terms),
                                                 _ptr(loss), _ptr(pred), _ptr(cpt), self._stream()), "si_codebook_metrics")
        return loss, terms, pred, cpt

    def kmeans_assign(self, feats: torch.Tensor, centroids: torch.Tensor, with_distance: bool = False):
        """feats (..., D), centroids (K, D) -> int64 labels (...) [, squared distance to the winner]."""
        assert feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous()
        assert centroids.is_cuda and centroids.dtype == torch.float32 and centroids.is_contiguous() and centroids.dim() == 2
        D = feats.shape[-1]
        assert centroids.shape[1] == D
        rows = feats.numel() // D
        labels = torch.empty(feats.shape[:-1], dtype=torch.int64, device=self.device)
        dist = torch.empty(feats.shape[:-1], dtype=torch.float32, device=self.device) if with_distance else None
        self._check(self.lib.si_kmeans_assign(self._h, _ptr(feats), rows, D, _ptr(centroids), centroids.shape[0], _ptr(labels),
                                              _ptr(dist), self._stream()), "si_kmeans_assign")
        return (labels, dist) if with_distance else labels

    def mel_metrics(self, mel_a: torch.Tensor, mel_b: torch.Tensor, center: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mel_a, mel_b (B, D, L) -> (B, 3) = avg_cosine_sim, avg_d2_dist, rmse of I_ea/metrics.py:38-62 per clip."""
        for m in (mel_a, mel_b):
            assert m.is_cuda and m.dtype == torch.float32 and m.dim() == 3 and m.is_contiguous()
        assert mel_a.shape == mel_b.shape
        B, D, L = mel_a.shape
        assert center is None or (center.is_cuda and center.dtype == torch.float32 and center.numel() == D and center.is_contiguous())
        out = torch.empty(B, 3, dtype=torch.float32, device=self.device)
        self._check(self.lib.si_mel_metrics(self._h, _ptr(mel_a), _ptr(mel_b), B, D, L, _ptr(center), _ptr(out), self._stream()), "si_mel_metrics")
        return out

    def sisdr(self, est: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
        """est, ref (B, n) waveforms -> (B,) SI-SDR in dB (I_ea/metrics.py:127-142)."""
        for m in (est, ref):
            assert m.is_cuda and m.dtype == torch.float32 and m.dim() == 2 and m.is_contiguous()
        assert est.shape == ref.shape
        out = torch.empty(est.shape[0], dtype=torch.float32, device=self.device)
        self._check(self.lib.si_sisdr(self._h, _ptr(est), _ptr(ref), est.shape[0], est.shape[1], _ptr(out), self._stream()), "si_sisdr")
        return out

    def unit_frontend(self, code: torch.Tensor, emb_c: torch.Tensor, f0_code: Optional[torch.Tensor] = None,
                      emb_p: Optional[torch.Tensor] = None, spk_emb: Optional[torch.Tensor] = None) -> torch.Tensor:
        """code (B, Fc) int64, emb_c (Kc, E); optional f0_code (B, Fp) int64 + emb_p (Kp, E); optional spk_emb (B, E)
        -> (B, nparts * E, max(Fc, Fp)) fp32, the CodeGenerator's generator input."""
        assert code.is_cuda and code.dtype == torch.int64 and code.dim() == 2 and code.is_contiguous()
        assert emb_c.is_cuda and emb_c.dtype == torch.float32 and emb_c.dim() == 2 and emb_c.is_contiguous()
        B, Fc = code.shape
        Kc, E = emb_c.shape
        Fp, Kp = 0, 0
        if f0_code is not None:
            assert f0_code.is_cuda and f0_code.dtype == torch.int64 and f0_code.is_contiguous() and f0_code.shape[0] == B
            assert emb_p is not None and emb_p.is_cuda and emb_p.dtype == torch.float32 and emb_p.is_contiguous() and emb_p.shape[1] == E
            Fp, Kp = f0_code.shape[1], emb_p.shape[0]
        if spk_emb is not None:
            assert spk_emb.is_cuda and spk_emb.dtype == torch.float32 and spk_emb.is_contiguous() and tuple(spk_emb.shape) == (B, E)
        nparts = 1 + (f0_code is not None) + (spk_emb is not None)
        out = torch.empty(B, nparts * E, max(Fc, Fp), dtype=torch.float32, device=self.device)
        self._check(self.lib.si_unit_frontend(self._h, _ptr(code), Fc, _ptr(f0_code), Fp, _ptr(spk_emb), _ptr(emb_c), Kc, _ptr(emb_p), Kp,
                                              E, B, _ptr(out), self._stream()), "si_unit_frontend")
        return out

    def f0_encoder(self, desc: "F0EncDesc", weights: torch.Tensor, f0: torch.Tensor) -> torch.Tensor:
        """f0 (B, in_width, T) fp32, weights = the packed encoder parameters (see include/si_hip.h) -> (B, T', out_width)
        fp32 channels-last: the rows the VQ bottleneck quantises (I_da/src/model.py:160-163)."""
        assert f0.is_cuda and f0.dtype == torch.float32 and f0.dim() == 3 and f0.is_contiguous() and f0.shape[1] == desc.in_width
        assert weights.is_cuda and weights.dtype == torch.float32 and weights.dim() == 1 and weights.is_contiguous()
        d = desc.as_struct()
        need = int(self.lib.si_f0_encoder_weight_floats(C.byref(d)))
        if weights.numel() != need:
            raise ValueError(f"F0 encoder weights: {weights.numel()} floats, the descriptor needs {need}")
        B, _, T = f0.shape
        Tp = int(self.lib.si_f0_encoder_frames(C.byref(d), T))
        if Tp <= 0:
            raise ValueError(f"{T} F0 frames are too few for this encoder")
        ws = torch.empty(int(self.lib.si_f0_encoder_workspace_bytes(C.byref(d), B, T)), dtype=torch.uint8, device=self.device)
        out = torch.empty(B, Tp, desc.out_width, dtype=torch.float32, device=self.device)
        self._check(self.lib.si_f0_encoder_forward(self._h, C.byref(d), _ptr(weights), _ptr(f0), B, T, _ptr(out), _ptr(ws), ws.numel(),
                                                   self._stream()), "si_f0_encoder_forward")
        return out

    def resample_poly(self, x: torch.Tensor, taps: torch.Tensor, up: int, down: int, pre_remove: int, n_out: int) -> torch.Tensor:
        """x (B, n_in) -> (B, n_out): upfirdn(taps, x, up, down)[pre_remove : pre_remove + n_out] (see audio.design_resampler)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
        assert taps.is_cuda and taps.dtype == torch.float32 and taps.dim() == 1 and taps.is_contiguous()
        y = torch.empty(x.shape[0], n_out, dtype=torch.float32, device=self.device)
        self._check(self.lib.si_resample_poly(self._h, _ptr(x), x.shape[0], x.shape[1], _ptr(taps), taps.numel(), int(up), int(down),
                                              int(pre_remove), int(n_out), _ptr(y), self._stream()), "si_resample_poly")
        return y

    def resample_sinc(self, x: torch.Tensor, filt: dict, n_out: int, n_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x (B, n_in) -> (B, n_out) by resampy's `kaiser_best` interpolation (librosa 0.9.1's resampler); `filt` holds the DEVICE
        tables of audio.design_kaiser_best (win, dwin, time_reg float64) and its scalars; n_len (B,) int32 device lengths or None."""
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
        for k in ("win", "dwin", "time_reg"):
            assert filt[k].is_cuda and filt[k].dtype == torch.float64 and filt[k].is_contiguous()
        assert n_len is None or (n_len.is_cuda and n_len.dtype == torch.int32 and n_len.numel() == x.shape[0] and n_len.is_contiguous())
        f = SincFilter(C.sizeof(SincFilter), filt["win"].numel(), int(filt["num_table"]), int(filt["step"]), filt["time_reg"].numel(), 0,
                       float(filt["scale"]), float(filt["ratio"]), filt["win"].data_ptr(), filt["dwin"].data_ptr(), filt["time_reg"].data_ptr())
        y = torch.empty(x.shape[0], int(n_out), dtype=torch.float32, device=self.device)
        self._check(self.lib.si_resample_sinc(self._h, _ptr(x), _ptr(n_len), x.shape[0], x.shape[1], C.byref(f), int(n_out), _ptr(y), self._stream()),
                    "si_resample_sinc")
        return y

    def pcm16(self, wav: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 waveform (any shape) -> int16 PCM on the device: `audio * 32768` truncated toward zero (I_ea/predict.py:204-206)."""
        assert wav.is_cuda and wav.dtype == torch.float32 and wav.is_contiguous()
        if out is None:
            out = torch.empty(wav.shape, dtype=torch.int16, device=self.device)
        assert out.is_cuda and out.dtype == torch.int16 and out.is_contiguous() and out.numel() == wav.numel()
        self._check(self.lib.si_pcm16(self._h, _ptr(wav), wav.numel(), _ptr(out), self._stream()), "si_pcm16")
        return out

    def extend_mel(self, mel: torch.Tensor) -> torch.Tensor:
        """(B, D, Tm) -> (B, D, floor(Tm * 441 / 256)): the x441/256 stretch alone (the generator's input with stretch=False)."""
        assert mel.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous() and mel.dim() == 3 and mel.shape[1] == self.desc.num_mels
        B, D, Tm = mel.shape
        hop = 1
        for i in range(self.desc.num_ups):
            hop *= self.desc.up_rates[i]
        out = torch.empty(B, D, self.vocoder_samples(Tm, True) // hop, dtype=torch.float32, device=self.device)
        self._check(self.lib.si_extend_mel(self._h, _ptr(mel), B, Tm, _ptr(out), self._stream()), "si_extend_mel")
        return out

    def hifigan_forward(self, mel: torch.Tensor, stretch: bool = True) -> torch.Tensor:
        assert mel.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous() and mel.dim() == 3
        B, D, Tm = mel.shape
        assert D == self.desc.num_mels
        L = self.vocoder_samples(Tm, stretch)
        out = torch.empty(B, L, dtype=torch.float32, device=self.device)
        ws = self.workspace(B, 0, Tm)
        self._check(self.lib.si_hifigan_forward(self._h, _ptr(mel), B, Tm, int(stretch), _ptr(out), _ptr(ws), ws.numel(),
                                                self._stream()), "si_hifigan_forward")
        return out

    def _mel_workspace(self, B: int, N: int) -> torch.Tensor:
        """The mel front-end's OWN scratch (not the encoder / vocoder workspace: the front-end may run on a side stream under the
        encoder).  Grown only; a buffer that is replaced stays referenced until the next call, so work still queued on it is safe."""
        need = C.c_size_t(0)
        self._check(self.lib.si_mel_workspace_bytes(self._h, B, N, C.byref(need)), "si_mel_workspace_bytes")
        cur = getattr(self, "_ws_mel", None)
        if cur is None or cur.numel() < need.value:
            self._ws_mel_old = cur
            self._ws_mel = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        return self._ws_mel

    def _mel_call(self, name: str, wave22: torch.Tensor, masks, mid, sample_len=None) -> torch.Tensor:
        """The mel front-end entry points: wave22 (B, N22) -> (B, 80, Tm) in the front-end's own workspace.  mid(lens) -> the arguments
        between `wave22` and `B`, lens = the HOST lengths `sample_len` of a ragged batch as a pointer (None without); masks: the
        per-clip int32 (B) device tensors of the one span, both or neither."""
        B, N = _f32(wave22, 2).shape
        lens = None if sample_len is None else self._host_lens(sample_len, B)
        Tm = int(self.lib.si_mel_frames(N))
        if Tm < 1:
            raise ValueError(f"clip of {N} samples is too short for the mel front-end")
        assert len({m is None for m in masks}) <= 1
        for m in masks:
            assert m is None or _i32(m, B) is m
        ws = self._mel_workspace(B, N)
        out = torch.empty(B, 80, Tm, dtype=torch.float32, device=self.device)
        self._check(getattr(self.lib, name)(self._h, _ptr(wave22), *mid(None if lens is None else lens.ctypes.data_as(C.c_void_p)), B, N,
                                            _ptr(out), _ptr(ws), ws.numel(), self._stream()), name)
        return out

    def mel_frontend(self, wave22: torch.Tensor, mask_start: Optional[torch.Tensor] = None,
                     mask_end: Optional[torch.Tensor] = None, normalize: bool = True) -> torch.Tensor:
        """(B, N22) raw 22.05 kHz clips -> (B, 80, Tm) log-mel; the span [mask_start, mask_end) of each clip is zeroed first."""
        return self._mel_call("si_mel_frontend", wave22, (mask_start, mask_end), lambda _: (_ptr(mask_start), _ptr(mask_end), int(normalize)))

    def capture(self, names, capacity=0):
        """Register capture buffers for the named intermediates (sizes come from the previous forward unless
        `capacity` elements is given: one count for all, or {name: count}).  Names ending in ".bf16" / ".f16" are raw
        bf16 / fp16 tensors.  Returns {name: tensor}; the tensors are filled by the next forward."""
        out = {}
        for nm in names:
            n = capacity.get(nm, 0) if isinstance(capacity, dict) else capacity
            n = n or self.lib.si_debug_size(self._h, nm.encode())
            if n < 0:
                raise NativeError(self.lib.si_last_error(self._h).decode())
            dt = torch.bfloat16 if nm.endswith(".bf16") else torch.float16 if nm.endswith(".f16") else torch.float32
            t = torch.zeros(n, dtype=dt, device=self.device)
            self._check(self.lib.si_debug_capture(self._h, nm.encode(), _ptr(t), n), "si_debug_capture")
            out[nm] = t
        self._captures = out
        return out

    def ws_regions(self, which: str):
        """[(name, offset, bytes)] of the most recent carve of the "encoder", "vocoder" or "mel" pass on this context, offsets from
        the workspace pointer of that call (si_debug_ws_regions; a test hook)."""
        arr = (WsRegion * 32)()
        n = C.c_int(0)
        self._check(self.lib.si_debug_ws_regions(self._h, ("encoder", "vocoder", "mel").index(which), arr, 32, C.byref(n)), "si_debug_ws_regions")
        return [(arr[i].name.decode(), int(arr[i].offset), int(arr[i].bytes)) for i in range(n.value)]

    def clear_captures(self):
        for nm in list(getattr(self, "_captures", {})):
            self.lib.si_debug_capture(self._h, nm.encode(), C.c_void_p(0), 0)
        self._captures = {}

    # ---- per-kernel HIP-event timing
    def profile_start(self, max_launches: int = 20000):
        self._check(self.lib.si_profile_start(self._h, int(max_launches)), "si_profile_start")

    def profile_filter(self, family: Optional[str]):
        """Bracket only launches of this kernel family (None: all)."""
        self._check(self.lib.si_profile_filter(self._h, family.encode() if family else None), "si_profile_filter")

    def profile_stop(self):
        """-> list of dicts {name, launches, ms, flops, bytes}; waits for the recorded events."""
        cap = 128
        arr = (ProfileEntry * cap)()
        n = C.c_int(0)
        self._check(self.lib.si_profile_stop(self._h, arr, cap, C.byref(n)), "si_profile_stop")
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, ms=arr[i].ms, flops=arr[i].flops,
                     bytes=arr[i].bytes) for i in range(min(n.value, cap))]
