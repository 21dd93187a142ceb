"""Case tables and input builders that more than one test file uses: the one-stage vocoder architectures and their seeded state,
launch_math restated, the encoder's seeded state and row choices, the unit vocoder's fp16 inputs, patch mode's common shape.
Importing this module needs no GPU (tests/test_vocoder_ref.py composes the fp16 inputs on the CPU)."""
import numpy as np
import torch

from tests import vocoder_ref as V

# ------------------------------------------------------------------------------------------------------------ vocoder side
R1 = {32: 256, 64: 512, 128: 256, 256: 128}           # rows of a pair kernel's tile (see test_gpu_vocoder_ops.py's docstring)
V1_BLOCKS = dict(resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3)


def _arch(C, u=1, k=3, num_mels=80, **kw):
    """One stage of C channels behind an upsampler (u, k).  C = 256 gets a second u = 1 stage of 128 channels behind it: conv_post_kernel
    keeps 262 rows of C + 4 floats in LDS and refuses 256 channels (no generator ends that wide).  num_mels: conv_pre's input width
    (80 mel bins; the unit vocoder's 384 embedding channels)."""
    from speech_inpainting_amd.arch import VocoderArch
    blocks = dict(V1_BLOCKS)
    blocks.update(kw)
    us, ks = ((u, 1), (k, 3)) if C == 256 else ((u,), (k,))
    return VocoderArch(upsample_rates=us, upsample_kernel_sizes=ks, upsample_initial_channel=2 * C, num_mels=num_mels, **blocks)


def _padded(C):
    """The width the fp16 stream carries a stage of C channels at (api.hip, stage_channels: 4 <= C < 32 is padded to 32 with zero weights)."""
    return 32 if 4 <= C < 32 else C


_STATE = {}
_FOLDED = {}


def _state(varch):
    from speech_inpainting_amd import synth
    if repr(varch) not in _STATE:
        _STATE[repr(varch)] = synth.synth_generator_state(varch, 47)
    return _STATE[repr(varch)]


def _w(varch, name):
    """The kernel's fp16 weight of a module, as float64 (vocoder_ref.fold: the packer's fold, rounded once)."""
    if (repr(varch), name) not in _FOLDED:
        _FOLDED[(repr(varch), name)] = V.fold(_state(varch), name)
    return _FOLDED[(repr(varch), name)]


def _mel(B, Tm, seed, num_mels=80):
    """The generator's input: a synthetic log-mel at 80 bins; at any other width (the unit vocoder's 384 channels of concatenated
    embeddings) N(0, 0.5^2), as test_ida_style_generator_geometry_matches_oracle draws it."""
    from speech_inpainting_amd import synth
    if num_mels == 80:
        return synth.synth_mel(B, Tm, 80, seed)
    return torch.randn(B, num_mels, Tm, generator=torch.Generator().manual_seed(seed)) * 0.5


def _interleave(lengths):
    """Long and short clips interleaved: workgroups get different tile counts."""
    lengths = sorted(set(int(v) for v in lengths if v >= 1))
    return lengths[::2] + lengths[1::2][::-1]


def _pair_lengths(C, ks=(3, 7, 11), dils=(1, 3, 5)):
    out = {1, 2, R1[C], R1[C] + 1}
    for k in ks:
        st = R1[C] - (k - 1)
        out |= {k - 1, st - 1, st, st + 1, 2 * st + 1} | {(k - 1) * d for d in dils}
    return out


def _config(math, N, M, ntaps, dil, Cin, stride=1):
    """launch_math (tapgemm.hip) for fp32 inputs (x16 == nullptr) -> (profile name, BM).  MaxA<256, 512> = 6 and MaxA<256> = 12 float4 per
    thread: both caps are 3072 float4, i.e. 384 rows of 32 channels.  N = 16 (a 32-column tile, Npad = 32) and Cin = 16 (BK = 16: a quarter of
    the float4 per row, so the 256-row tile's halo always fits) need no case of their own: tests/test_gpu_unitvoc_ops.py asserts these names there."""
    bk = 32 if Cin % 32 == 0 else 16
    bn = 128 if N >= 128 else 64 if N > 32 else 32
    rows256 = 255 * stride + (ntaps - 1) * abs(dil) + 1
    cap = (3 if ntaps == 1 else 6) * 512
    if bn == 128:
        tall = bk == 32 and M > 256 and rows256 * (bk // 4) <= cap
        return (f"tapgemm_{math}_256x128w8", 256) if tall else (f"tapgemm_{math}_128x128", 128)
    tall = rows256 * (bk // 4) <= cap and M > 128
    return (f"tapgemm_{math}_256x{bn}", 256) if tall else (f"tapgemm_{math}_128x{bn}", 128)


# ------------------------------------------------------------------------------------------------------------ encoder side
_ENC_STATES = {}


def _enc_state(harch):
    from speech_inpainting_amd import synth
    key = repr(harch)                                  # the whole architecture: two of one width may differ in any other shape
    if key not in _ENC_STATES:
        _ENC_STATES[key] = synth.synth_hubert_state(harch, 31)
    return _ENC_STATES[key]


def _sel_rows(M, k=96, seed=0):
    """Rows to check of a long GEMM: the first 8, the last 336 (every last tile of every height, whole), k random ones."""
    if M <= 512:
        return torch.arange(M)
    g = torch.Generator().manual_seed(seed)
    return torch.unique(torch.cat([torch.arange(8), torch.arange(M - 336, M), torch.randint(0, M, (k,), generator=g)]))


def _pick_wave(harch, B, T, bm):
    """A batch of B clips of exactly T frames whose sample count puts as many strided convs as possible at a last tile of 1 or
    bm - 1 rows (every count 320 (T - 1) + 400 + d, d < 320, has T frames)."""
    from speech_inpainting_amd import synth
    best, bestd = -1, 0
    for d in range(320):
        Ls = harch.feat_lengths(320 * (T - 1) + 400 + d)
        score = sum(L % bm in (1, bm - 1) for L in Ls[2:-1])
        if score > best:
            best, bestd = score, d
    N = 320 * (T - 1) + 400 + bestd
    assert harch.num_frames(N) == T
    return synth.synth_wave(B, N, 7 + T).cuda()


# ------------------------------------------------------------------------------------------------------------ the unit vocoder
ONE_K3 = dict(resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1, 3, 5),))
ONE_PAIR = dict(resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1,),))
SWITCH = (127, 128, 129, 255, 256, 257)               # GEMM rows M on both sides of launch_math's 128- and 256-row switches
U5_LIN = (1, 2, 3) + tuple(m - 1 for m in SWITCH)     # u = 5 (and 4): M = Lin + 1
TC_LIN = (1, 190, 191, 192, 254, 255, 256)            # Lin + 1 = BM - 1, BM, BM + 1 for BM = 192, 256


def unit_arch():
    from speech_inpainting_amd.arch import VocoderArch
    return VocoderArch(upsample_rates=(5, 4, 4, 2, 2), upsample_kernel_sizes=(11, 8, 8, 4, 4), upsample_initial_channel=512, num_mels=384,
                       sampling_rate=16000)


def _arch_u5(C):
    return _arch(C, u=5, k=11, **ONE_K3)


def _arch_u4(C):
    return _arch(C, u=4, k=8, **ONE_PAIR)


def _arch_c16(u):
    return _arch(16, u=2, k=4) if u == 2 else _arch(16)


def _arch_pre384():
    return _arch(64, num_mels=384, **ONE_K3)


def _tc_pick(ms, N, cus):
    """gemmcu_tc_pick's cost rule (always = true) over the clips' GEMM rows `ms` -> the tile height it takes."""
    best, pick = None, None
    for bm in (256, 192):
        tiles = sum(-(-m // bm) for m in ms) * (N // 256)
        cost = -(-tiles // cus) * (bm + 256)
        if best is None or cost < best:
            best, pick = cost, bm
    return pick


def _tc_batch(N, cus):
    """(clips, M): the smallest batch of at most 32 equal clips for which the cost rule takes 256-row tiles -- 192-row tiles need one more
    round of the chip.  The issue's batches (32 x 800 at N = 512, 32 x 1600 at N = 256) first: they are the answer on 256 CUs."""
    for B, M in ((32, 800 if N == 512 else 1600),) + tuple((B, M) for M in range(320, 4097, 32) for B in (8, 16, 24, 32)):
        if _tc_pick([M] * B, N, cus) == 256 and _tc_pick([M + 1] * B, N, cus) == 256 and _tc_pick([M - 1] * B, N, cus) == 256:
            return B, M
    return None


C16_PAIR_ROWS = sorted(_pair_lengths(32) | {3, 511, 512, 513, 1025})


def _chain_rows():
    out = {1, 2, 768, 769, 511, 512, 513}
    for k in (3, 7, 11):
        st = 768 - 12 * (k - 1)
        out |= {k - 1, 5 * (k - 1), st - 1, st, st + 1, 2 * st + 1}
    return sorted(out)


def _c16_lens(u, rows):
    """Mel frames that put the stage at `rows` (u = 1), or at the even rows on both sides of each of them (u = 2)."""
    if u == 1:
        return _interleave(rows)
    return _interleave({max(1, r // 2) for r in rows} | {(r + 1) // 2 for r in rows})


def _split(lens, n=32):
    return [lens[i:i + n] for i in range(0, len(lens), n)]


def fp16_inputs(cus=256):
    """Every input the fp16 tests of test_gpu_unitvoc_ops.py run, as (tag, architecture, seed, lens or None, frames, clips checked): what
    the CPU self-test composes the references on.  `lens` None: a uniform batch of one clip twice."""
    out = []
    for C in (256, 32):
        out.append((f"u5 C={C} ragged", _arch_u5(C), 1100 + C, list(_interleave(U5_LIN)), max(U5_LIN), None))
        out += [(f"u5 C={C} uniform", _arch_u5(C), 1200 + C, None, L, [0]) for L in U5_LIN]
    for C in (128, 64):
        out.append((f"u4 C={C} ragged", _arch_u4(C), 1300 + C, list(_interleave(TC_LIN)), max(TC_LIN), None))
        out += [(f"u4 C={C} uniform", _arch_u4(C), 1310 + C, None, L, [0]) for L in TC_LIN[1:]]
        big = _tc_batch(4 * C, cus)
        if big is not None:
            B, M = big
            lens = [M - 1] * B
            lens[B // 2 - 1], lens[B // 2] = M, M - 2
            out.append((f"u4 C={C} {B} clips", _arch_u4(C), 1320 + C, lens, M, [0, B // 2 - 1, B // 2, B - 1]))
        out.append((f"u4 C={C} tap-GEMM", _arch_u4(C), 1300 + C, list(_interleave((1, 191, 256))), 256, None))
    for u in (2, 1):
        for n, lens in enumerate(_split(_c16_lens(u, sorted(set(C16_PAIR_ROWS) | set(_chain_rows()))), 24)):
            out.append((f"c16 u={u} batch {n}", _arch_c16(u), 1400 + 10 * u + n, lens, max(lens), None))
        out.append((f"c16 u={u} uniform", _arch_c16(u), 1430 + u, None, 745 if u == 1 else 372, [0]))
        out.append((f"c16 u={u} tap-GEMM pairs", _arch_c16(u), 1440 + u, list(_interleave((1, 2, 10, 127, 128, 129, 300))), 300, None))
    out += [("pre384 uniform", _arch_pre384(), 1500, None, L, [0]) for L in SWITCH]
    out.append(("unit B=2", unit_arch(), 1600, None, 7, [0]))
    out.append(("unit ragged", unit_arch(), 1601, [7, 1, 4], 7, None))
    return out


# ------------------------------------------------------------------------------------------------------------ patch mode
N_OUT, HOP = 33024, 256                          # test_gpu_patch.py's common shape: samples the generator returns per clip, per frame
FADES = [0, 110, 300]
CHUNK = 2048                                     # PC_CHUNK of patch_kernels.hip: samples per workgroup of the compose kernel


def _patch_engine(voc="fp32"):
    """Tiny HuBERT + V1 generator, as test_windowed_passes_over_merged_windows_equal_full_passes builds them; one per vocoder mode."""
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from tests.harness import build_engine
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", voc, key=("patch", voc))


def _weights64(spans, lim, fade, n):
    """The weight of the generated audio per sample of one clip, float64, written out from the definition (not through gaps.blend_weights):
    the maximum over the spans of {ramp on the rise, 1 inside, mirrored ramp on the fall}, 0 at and past lim; and the index of the span
    that gives it (the first on ties)."""
    from speech_inpainting_amd import gaps as G
    ramp = G.fade_ramp(fade).astype(np.float64)
    w, who = np.zeros(n), np.full(n, -1)
    for k, (s, l) in enumerate(spans):
        if l <= 0 or s >= lim:
            continue
        for m in range(max(s - fade, 0), min(s + l + fade, lim)):
            wk = ramp[m - (s - fade)] if m < s else 1.0 if m < s + l else ramp[s + l + fade - 1 - m]
            if wk > w[m]:
                w[m], who[m] = wk, k
    return w, who
