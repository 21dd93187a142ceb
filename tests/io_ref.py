"""The kernels that take a file in, push PCM out and feed the unit vocoder, restated in numpy float64 with the bound each fp32 result
has to meet: resample_poly_kernel, resample_sinc_kernel, pcm16_kernel (frontend_kernels.hip), extend_mel_cf_kernel / extend_mel_kernel
(vocoder_kernels.hip), and the LDS formula that routes si_f0_encoder_forward.  Pure numpy: no GPU, no torch kernels.

Every reference returns what the bound is made of -- S = the sum of |term| over the same terms, K = the number of terms -- and `near`,
the outputs whose tap window is cut by an end of the input or by a clamp, or that sit on either side of a 256-output block seam.  The
bounds come from the operands alone:
    poly     E = K 2^-24 S (1 + K 2^-24) + 2^-149     one rounding per fmaf of the kernel's chain (Higham's gamma_K to second order)
    sinc     E = 2^-24 |y| + (K + 2) 2^-52 S + 2^-149  the final cast; float64 summation order and a contracted win + eta dwin
    stretch  E = 3 2^-24 (l0 |a| + l1 |b|)             two products and one sum, contracted or not
    pcm      exact
`mistake` plants one wrong reading of a definition; tests/test_io_ref.py shows that each of them leaves E on one of the cases below,
so a kernel that made it would fail tests/test_gpu_io_ops.py.
"""
import math

import numpy as np

from speech_inpainting_amd import audio

U24, U52, TINY = 2.0 ** -24, 2.0 ** -52, 2.0 ** -149
BLOCK = 256                                                # outputs per workgroup of all four kernels

# (sr_in, sr_out) -> n_in: 1, 2, the filter's reach, the 256-output block seam
POLY_CASES = {
    (22050, 16000): (1, 2, 27, 28, 352, 353),             # reach 27..29 inputs; n_out 256, 257
    (16000, 22050): (1, 2, 185, 186, 187),                # n_out 255, 257, 258
    (44100, 16000): (1, 2, 55, 705, 706),                 # reach; n_out 256, 257
    (48000, 22050): (1, 2, 40, 557, 558),                 # reach; n_out 256, 257
    (8000, 22050): (1, 2, 92, 93),                        # n_out 254, 257
    (16000, 8000): (1, 2, 511, 512, 513),                 # 43 taps
    (8000, 16000): (1, 2, 127, 128, 129),
}
POLY_N_OUT = {(22050, 16000, 352): 256, (22050, 16000, 353): 257, (16000, 22050, 185): 255, (16000, 22050, 186): 257,
              (16000, 22050, 187): 258, (44100, 16000, 705): 256, (44100, 16000, 706): 257, (48000, 22050, 557): 256,
              (48000, 22050, 558): 257, (8000, 22050, 92): 254, (8000, 22050, 93): 257}
SINC_CASES = {
    (22050, 16000): (1, 2, 3, 64, 89, 90, 353, 354),      # the window is ~88 inputs wide: below it both wings are cut at once
    (16000, 22050): (1, 2, 64, 65, 186, 187),
    (44100, 16000): (1, 3, 177, 706),
    (48000, 16000): (1, 2, 3, 4, 767, 768, 769, 770),     # every accumulated time is an integer (3 is exact in float64)
    (8000, 16000): (1, 2, 127, 128, 129),                 # every other time is an integer
    (16000, 8000): (1, 2, 3, 511, 512, 513),              # every time is an integer
}
POLY_MISTAKES = ("tap_plus_1", "input_plus_1", "last_tap_dropped", "row0")
SINC_MISTAKES = ("tap_plus_1", "input_plus_1", "last_tap_dropped", "row0")
STRETCH_MISTAKES = ("last_frame_unclamped", "row0")
STRETCH_TM = (1, 2, 3, 148, 149, 150, 500)                # Tout 1, 3, 5, 254, 256, 258, 861
PCM_LENGTHS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 4101)


def clips(B, n, seed):
    """B different fp32 clips of n samples: noise under a slow envelope, peaks near 1."""
    g = np.random.default_rng(seed)
    t = np.arange(n)
    return np.stack([(0.35 * g.standard_normal(n) * (0.6 + 0.4 * np.sin(t / (7.0 + b) + b))) for b in range(B)]).astype(np.float32)


def impulse(n, j0):
    x = np.zeros((1, n), dtype=np.float32)
    x[0, j0] = 1.0
    return x


def _seam(n_out):
    m = np.arange(n_out)
    return (m % BLOCK == 0) | (m % BLOCK == BLOCK - 1)


def ratios(got, ref, E, near):
    """max |got - ref| / E over the near-edge outputs and over the rest (0 / 0 = 0; anything over E = 0 is infinite)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / E)
    near = np.broadcast_to(near, q.shape)
    return float(q[near].max(initial=0.0)), float(q[~near].max(initial=0.0))


# ------------------------------------------------------------------------------------------------------------ polyphase resampler
def poly_ref(x, taps, up, down, pre, n_out, mistake=None):
    """y[m] = sum_j h[(m + pre) down - j up] x[j] over the j in [0, n_in) that keep the tap index in [0, ntaps), h = the fp32 taps of
    audio.design_resampler.  x (B, n_in) fp32 -> (y, S) float64 (B, n_out), K (n_out,), near (n_out,)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32)).astype(np.float64)
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    n_in, ntaps = x.shape[1], h.size
    if mistake == "row0":
        x = np.broadcast_to(x[:1], x.shape)
    m = np.arange(n_out, dtype=np.int64)
    t = (m + pre) * down
    j0 = t // up                                           # newest input that can touch the output
    k0 = t - j0 * up                                       # its tap
    full = np.maximum(-(-(ntaps - k0) // up), 0)           # terms of an input without ends
    i = np.arange(-(-ntaps // up) + 1, dtype=np.int64)[None, :]
    k, j = k0[:, None] + i * up, j0[:, None] - i
    live = (k < ntaps) & (j >= 0) & (j < n_in)
    K = live.sum(1)
    if mistake == "last_tap_dropped":                      # the oldest tap an end of the input leaves is not read
        last = np.where(live, i, -1).max(1)
        live &= ~((i == last[:, None]) & (K < full)[:, None])
    if mistake == "tap_plus_1":
        k = k + 1
        live &= k < ntaps
    xj = j + 1 if mistake == "input_plus_1" else j
    xv = np.where((xj >= 0) & (xj < n_in), x[:, np.clip(xj, 0, n_in - 1)], 0.0)
    terms = np.where(live, h[np.clip(k, 0, ntaps - 1)] * xv, 0.0)
    return terms.sum(-1), np.abs(terms).sum(-1), K, (K < full) | _seam(n_out)


def poly_bound(S, K):
    return K * U24 * S * (1.0 + K * U24) + TINY


def poly_fp32_chain(x, taps, up, down, pre, n_out):
    """The kernel's own chain on the CPU: acc = fmaf(h[k], x[j], acc) from the newest input down, in fp32 (the float64 product of two
    floats is exact, so one rounding of product + acc is the fma up to a double rounding that E covers many times over)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    h = np.asarray(taps, dtype=np.float32)
    n_in, ntaps = x.shape[1], h.size
    y = np.zeros((x.shape[0], n_out), dtype=np.float32)
    for m in range(n_out):
        t = (m + pre) * down
        j = t // up
        k = t - j * up
        if j > n_in - 1:
            k += (j - (n_in - 1)) * up
            j = n_in - 1
        acc = np.zeros(x.shape[0], dtype=np.float32)
        while k < ntaps and j >= 0:
            acc = (np.float64(h[k]) * x[:, j].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            k += up
            j -= 1
        y[:, m] = acc
    return y


# ------------------------------------------------------------------------------------------------------------ sinc resampler
def sinc_ref(x, filt, n_in, mistake=None):
    """resample_sinc_kernel's two wings in float64 from the tables of audio.design_kaiser_best: x (B, stride) or (stride,) fp32, clip b
    holds n_in[b] samples (one int: all of them) -> (y, S, K, near), each (B, len(time_reg)): zero at and past int(n_in ratio)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32)).astype(np.float64)
    B = x.shape[0]
    lens = [int(n_in)] * B if np.ndim(n_in) == 0 else [int(v) for v in n_in]
    win, dwin, tr = filt["win"], filt["dwin"], filt["time_reg"]
    nwin, ntab, step, scale, ratio = win.size, filt["num_table"], filt["step"], filt["scale"], filt["ratio"]
    stride = tr.size
    y, S = np.zeros((B, stride)), np.zeros((B, stride))
    K, near = np.zeros((B, stride), dtype=np.int64), np.zeros((B, stride), dtype=bool)
    i = np.arange(nwin // step + 2, dtype=np.int64)[None, :]
    for b in range(B):
        xb = x[0] if mistake == "row0" else x[b]
        nb = lens[b]
        n_out = min(int(nb * ratio), stride)
        near[b] = _seam(stride)
        near[b, n_out:] = True                             # the zero fill
        if n_out <= 0:
            continue
        time = tr[:n_out]
        n = time.astype(np.int64)                          # (int)time, time >= 0
        frac = scale * (time - n)
        for wing, fr, room in ((0, frac, n + 1), (1, scale - frac, nb - n - 1)):
            idx = fr * ntab
            off = idx.astype(np.int64)
            eta = idx - off
            table = (nwin - off) // step
            cnt = np.minimum(room, table)
            if mistake == "last_tap_dropped":              # the last tap an end of the input leaves is not read
                cnt = np.where(room < table, cnt - 1, cnt)
            live = i < cnt[:, None]
            w = off[:, None] + i * step + (1 if mistake == "tap_plus_1" else 0)
            xi = (n[:, None] - i if wing == 0 else n[:, None] + 1 + i) + (1 if mistake == "input_plus_1" else 0)
            if mistake is None and np.any(live & ((xi < 0) | (xi >= nb) | (w >= nwin))):
                raise IndexError("a tap the counts allow lies outside the clip or the table")
            wc = np.clip(w, 0, nwin - 1)
            xv = np.where((xi >= 0) & (xi < xb.size), xb[np.clip(xi, 0, xb.size - 1)], 0.0)
            terms = np.where(live, (win[wc] + eta[:, None] * dwin[wc]) * xv, 0.0)
            y[b, :n_out] += terms.sum(1)
            S[b, :n_out] += np.abs(terms).sum(1)
            K[b, :n_out] += live.sum(1)
            near[b, :n_out] |= room < table
    return y, S, K, near


def sinc_bound(y, S, K):
    return U24 * np.abs(y) + (K + 2) * U52 * S + TINY


def sinc_filter(sr_in, sr_out, n_in):
    return audio.design_kaiser_best(sr_in, sr_out, n_in)


# ------------------------------------------------------------------------------------------------------------ PCM cast
def pcm_ref(x, mistake=None):
    """p = float32(x) * 32768 (a power of two: exact, in fp32 too unless it overflows to the same infinity); NaN -> 0, otherwise
    clip(trunc(p), -32768, 32767)."""
    with np.errstate(invalid="ignore"):                  # (a signalling NaN among the values)
        p = np.asarray(x, dtype=np.float32).astype(np.float64) * 32768.0
    q = np.rint(p) if mistake == "rounds" else np.trunc(p)
    return np.clip(np.where(np.isnan(p), 0.0, q), -32768.0, 32767.0).astype(np.int16)


def pcm_values():
    """k / 32768 for every int16 k with both fp32 neighbours of each, +-0, subnormals, +-1 and their inner neighbours, values past
    full scale up to +-inf, NaN of either sign."""
    k = (np.arange(-32768, 32768, dtype=np.float64) / 32768.0).astype(np.float32)
    one, inf = np.float32(1.0), np.float32(np.inf)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 1.0, -1.0,
                        np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(0)), 1.0000001, -1.0000001, 2.0, -2.0, 1e30, -1e30,
                        3e38, -3e38, np.inf, -np.inf], dtype=np.float32)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    return np.concatenate([k, np.nextafter(k, inf), np.nextafter(k, -inf), special, nan])


def pcm_mix(n, seed):
    """n values for the length and offset cases: the specials of pcm_values() among samples on and next to the int16 grid."""
    g = np.random.default_rng(seed)
    v = pcm_values()
    x = v[g.integers(0, v.size, n)]
    tail = v[-26:]                                         # specials and NaNs
    x[g.integers(0, n, max(1, n // 8))] = tail[g.integers(0, tail.size, max(1, n // 8))]
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ mel stretch
def stretch_tout(Tm):
    return int(math.floor(float(Tm) * (441 / 256)))


def stretch_ref(mel, mistake=None):
    """The x441/256 bilinear stretch: src, i0, i1, l1, l0 in fp32 exactly as the kernels and the oracle state them (the source index is
    one rounding of the double product: the fma), then y = l0 a + l1 b in float64.  mel (B, D, Tm) fp32 -> (y, E) (B, D, Tout), near.
    i0's own clamp at Tm - 1 never binds: src <= (Tout - 1/2) 256/441 - 1/2 <= Tm - 0.79; the clamp that does is i1's, at the outputs
    whose i0 is the last frame.  `last_frame_unclamped` reads frame Tm there -- the next row's first frame in memory."""
    mel = np.asarray(mel, dtype=np.float32)
    B, D, Tm = mel.shape
    Tout = stretch_tout(Tm)
    rscale = np.float32(1.0 / (441.0 / 256.0))
    dst = np.arange(Tout, dtype=np.float32)
    src = ((dst + np.float32(0.5)).astype(np.float64) * np.float64(rscale) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0.0))
    i0 = np.minimum(np.floor(src).astype(np.int64), Tm - 1)
    i1 = np.minimum(i0 + 1, Tm - 1)
    l1 = np.clip(src - i0.astype(np.float32), np.float32(0.0), np.float32(1.0)).astype(np.float32)
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    x = mel.astype(np.float64)
    if mistake == "row0":
        x = np.broadcast_to(x[:1, :1], x.shape)
    a = x[:, :, i0]
    if mistake == "last_frame_unclamped":
        flat = np.concatenate([x.reshape(-1), [0.0]])
        rows = (np.arange(B * D) * Tm).reshape(B, D, 1)
        b = flat[rows + (i0 + 1)[None, None, :]]
    else:
        b = x[:, :, i1]
    l0, l1 = l0.astype(np.float64), l1.astype(np.float64)
    y = l0 * a + l1 * b
    E = 3.0 * U24 * (l0 * np.abs(x[:, :, i0]) + l1 * np.abs(x[:, :, i1]))
    near = (i0 + 1 > Tm - 1) | (dst == 0) | _seam(Tout)
    return y, E, near


def stretch_mel(B, D, Tm, seed):
    """Values about +-3; row 1 of clip 0 is the constant 1.0 (its stretch is exactly 1.0: fl(1 - l1) + l1 rounds to 1)."""
    g = np.random.default_rng(seed)
    m = (3.0 * g.uniform(-1.0, 1.0, (B, D, Tm))).astype(np.float32)
    m[0, 1 % D] = 1.0
    return m


# ------------------------------------------------------------------------------------------------------------ F0 encoder routes
def f0_fused_lds_bytes(desc, T):
    """si_launch_f0enc_fused's LDS need for a track of T frames, or None where it refuses the descriptor (a width off the 8 grid)."""
    k, pad = desc.down_kernel()
    T1 = (T + 2 * pad - k) // desc.stride_t + 1
    c = max(desc.width, desc.n_state)
    slot = (c * max(T1, 1) + 3) // 4 * 4
    wmax = max(desc.width * max(desc.in_width, desc.width) * k, desc.n_state * desc.width * 3, desc.out_width * desc.width * 3)
    wmax = (wmax + 3) // 4 * 4
    if desc.width % 8 or desc.n_state % 8 or desc.out_width % 8:
        return None
    return (2 * slot + wmax + max(c, desc.out_width)) * 4


def f0_longest_fused(desc, limit=158 * 1024):
    """The largest T the single launch takes (the need grows with T)."""
    T = 1
    while f0_fused_lds_bytes(desc, T + 1) <= limit:
        T += 1
    return T


def f0_launches(desc):
    return desc.down_t * (1 + 2 * desc.depth) + 1
