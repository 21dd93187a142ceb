"""Interleaved multi-channel files: the joint-detection reference and the case builders of tests/test_channels_host.py,
tests/test_gpu_channels.py and tests/test_gpu_channels_route.py.  A plain module, imported by name; importing it needs no GPU.

The reference of everything per channel is the MONO entry point on the de-interleaved channel x[:, c]; only the joint detection has a
definition of its own, and it is one line: a sample time is quiet iff every channel is (tests/detect_ref.py's quiet_mask per element),
so the runs are detect_ref's runs of the 0 / 1 signal "some channel is loud" at threshold 0."""
import numpy as np
import torch

from speech_inpainting_amd import gaps as G
from tests import detect_ref as D

TORCH = {np.float32: torch.float32, np.int16: torch.int16}


def joint_signal(x, thr):
    """x (n, ch) -> float32 (n,): 0 where every channel is quiet under thr, 1 where some channel is loud."""
    return (~np.all(D.quiet_mask(x, thr), axis=1)).astype(np.float32)


def joint_runs_ref(x, thr, min_len):
    return D.quiet_runs_ref(joint_signal(x, thr), 0.0, min_len)


def noise(n, dtype, seed, amp):
    """n samples of `dtype` in +-amp (full scale 1.0 for fp32, int16 steps for int16), none of them zero."""
    rng = np.random.default_rng(seed)
    if dtype is np.float32:
        return ((rng.random(n) * 0.9 + 0.1) * amp * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return (rng.integers(max(int(amp) // 10, 1), int(amp) + 1, n) * rng.choice([-1, 1], n)).astype(np.int16)


def around(col, c, ch, seed=0):
    """The host samples `col` (n,) as channel c of an (n, ch) file whose other channels hold independent noise at about ten times
    col's amplitude: whatever leaks from a neighbouring channel shows."""
    dtype = col.dtype.type
    amp = 0.9 if dtype is np.float32 else 30000
    x = np.stack([col if k == c else noise(col.size, dtype, 1000 * seed + k, amp) for k in range(ch)], axis=1)
    return np.ascontiguousarray(x)


def on_device(x, dev, off=0):
    """The host array x ((n,) or (n, ch)) on the device as a contiguous view that starts `off` ELEMENTS past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=dev)
    v = buf[off:off + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v.view(t.shape)


def rate_case(sr, fade_f, n_file=3 * 2048 + 77, amp=0.03, seed=0):
    """tests/test_gpu_rate.py's kernel case on n_file samples at sr: five spans (one whose taps reach before sample 0, two across chunk
    seams, two whose ramps overlap and belong to different windows, one cut by its context's end) over two windows of two contexts,
    + a THIRD window of a third context that no span uses -- another channel's share of a pass.  -> spans, windows (the two), windows3
    (the three), chunks, gen (3, lrow), orig (n_file,) fp32 at amplitude amp, lrow."""
    from tests import rate_ref as R
    P, Q = G.rate_ratio(sr)
    H = R.reach(sr)
    n22 = -(-n_file * P // Q)
    gap = 3 + fade_f // 2
    raw = [(30, 100, 0), (2048 - 60, 150, 0), (2700, 80, 0), (2780 + gap, 90, 1), (3 * 2048 - 100, 150, 1)]
    reg = lambda s, l: (max(s - fade_f, 0), s + l + fade_f)
    len0 = (reg(*raw[2][:2])[1] - 1) * P // Q + 1 + H + 5
    ws1 = reg(*raw[3][:2])[0] * P // Q - H - 3
    lim1 = (3 * 2048 + 6) * P // Q
    windows = [(0, 0, len0, len0), (1, ws1, lim1 + 10 - ws1, lim1)]
    assert ws1 > 0 and lim1 + 10 <= n22
    lims = [min(G.file_lim(w[3], sr), n_file) for w in windows]
    spans = [(s, l, w, lims[w]) for s, l, w in raw]
    regions = G.file_regions([(s, l) for s, l, _, _ in spans], [sp[3] for sp in spans], fade_f)
    chunks = G.region_chunks(regions)
    g = torch.Generator().manual_seed(sr + fade_f + seed)
    lrow = max(w[2] for w in windows) + 3
    gen = ((torch.rand(3, lrow, generator=g) * 2 - 1) * 0.3).contiguous()
    orig = ((torch.rand(n_file, generator=g) * 2 - 1) * amp).contiguous()
    windows3 = windows + [(2, 100, min(lrow, n22 - 100), n22)]
    return dict(spans=spans, windows=windows, windows3=windows3, chunks=chunks, gen=gen, orig=orig, lrow=lrow)
