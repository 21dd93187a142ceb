"""The calls of tests/test_gpu_feed_launches.py, built once for the test and for tools/record_feed_launches.py, which records their
digests (tests/golden/feed_launches.json): every file feed -- cut_rate, cut_pair, cut_clips, each with and without a ceiling -- and
patch_rate, on one file of N_FILE sample times at four rates, in fp32, int16 and packed 24-bit, as (n,), as (n, 1) with channel 0 and as
(n, 2) with channel 1.

The file: a smooth signal of amplitude 0.3 and, per rate, four samples that a ceiling of half of full scale makes invalid: one two file
samples past the seam of cut_rate's tiles 0 | 1 of the clip that starts at 0, one a file sample past the seam of cut_pair's frames 0 | 1,
one in the middle and one three samples before the file's end -- each within H taps of what it names.  fp32: NaN, inf, 0.9 and NaN; PCM:
0.9 of full scale.  Channel 0 of the (n, 2) file is another signal; fp32 and int16 files are device views one element past a 16-byte
boundary (tests/channels_ref.on_device)."""
import hashlib

import numpy as np
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import channels_ref as CH
from tests import pair_ref as PR
from tests import s24_ref as S

N_FILE = 3001
RATES = (48000, 44100, 16000, 8000)
FORMATS = ("f32", "s16", "s24")
LAYOUTS = {"mono": (1, None), "one": (1, 0), "two": (2, 1)}           # name -> (columns of the file, channel)
FULL = {"f32": 1.0, "s16": 32768.0, "s24": 8388608.0}
ESZ = {"f32": 4, "s16": 2, "s24": 3}
TILE, FRAMES, CHUNK = native.CUT_RATE_TILE, native.CUT_PAIR_FRAMES, 2048
L_RATE = TILE + 5                                                     # two tiles, the second partial
L22 = 441 * 2 + 3
L_CLIPS = CHUNK + 7
FADE = 20
REGION = (CHUNK + 10, 100)                                            # its leading cross-fade [2038, 2058) crosses the seam of chunks 0 | 1


def ceiling_of(fmt):
    return float(np.float32(0.5 * FULL[fmt]))


def reach(filt):
    """H = ceil(nwin / step): taps per wing of a filter as the engine holds it; 0 for None."""
    return 0 if filt is None else -(-filt["win"].numel() // int(filt["step"]))


def invalid_positions(sr):
    P, Q = G.rate_ratio(sr)                                           # (22050, sr) / gcd
    return [TILE * Q // P + 2, sr // 50 + 1, 1500, N_FILE - 3]


def column(fmt, sr, seed=0):
    t = np.arange(N_FILE, dtype=np.float64)
    x = 0.3 * np.sin(2 * np.pi * t / (97.0 + 10 * seed)) + 0.05 * np.sin(2 * np.pi * t / 13.0 + seed)
    pos = invalid_positions(sr)
    if fmt == "f32":
        x = x.astype(np.float32)
        if seed == 0:
            x[pos[0]], x[pos[1]], x[pos[2]], x[pos[3]] = np.nan, np.inf, 0.9, np.nan
        return x
    v = np.rint(x * (FULL[fmt] - 1)).astype(np.int32)
    if seed == 0:
        v[pos] = int(0.9 * FULL[fmt]) * np.array([1, -1, 1, -1])
    return v.astype(np.int16) if fmt == "s16" else v


def file_on_device(fmt, layout, sr, dev):
    """The file as the call takes it: (n,), (n, 1) or (n, 2) with the signal in channel 1; packed 24-bit with its trailing 3 bytes."""
    cols, _ = LAYOUTS[layout]
    x = column(fmt, sr)
    x = x if layout == "mono" else x.reshape(N_FILE, 1) if cols == 1 else np.stack([column(fmt, sr, 1), x], axis=1)
    if fmt == "s24":
        return torch.from_numpy(S.pack(x)).to(dev)
    return CH.on_device(x, dev, 1)


def family(base, layout, ceiling):
    """The profile family of one call: the interleaved kernel's for a file with `channel`, except under a ceiling, where the one C entry
    takes an (n, 1) file as the mono file."""
    inter = layout == "two" if ceiling is not None else layout != "mono"
    return base + "_ch" if inter else base


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------ the calls
# Each generator yields (key, call, model): call() -> the output tensors; model = {family: (launches, flops, bytes)} as the launcher
# counts them, written out from C, L, H, cap, the element size and the grid.
def cut_rate_calls(eng, sr):
    ctx, dev = eng.ctx, eng.device
    filt = eng._feed_filter(sr)
    P, Q = G.rate_ratio(sr)
    H = reach(filt)
    cap = (TILE - 1) * Q // P + 2 + 2 * H
    N22 = -(-N_FILE * P // Q)
    starts = [0, N22 - L_RATE]
    Cn, grid_x = len(starts), -(-L_RATE // TILE)
    for fmt in FORMATS:
        for layout, (_, channel) in LAYOUTS.items():
            x = file_on_device(fmt, layout, sr, dev)
            for ceiling in (None, ceiling_of(fmt)):
                def call(x=x, channel=channel, ceiling=ceiling):
                    if ceiling is None:
                        return (ctx.cut_rate(x, sr, starts, L_RATE, filt, channel=channel),)
                    return (ctx.cut_rate_valid(x, sr, starts, L_RATE, filt, ceiling, channel=channel),)
                outs = float(Cn * L_RATE)
                model = {family("cut_rate", layout, ceiling): (1, outs * 8.0 * H, outs * 4.0 + float(grid_x) * Cn * cap * ESZ[fmt])}
                yield f"cut_rate/{sr}/{fmt}/{layout}/{'ceiling' if ceiling else 'plain'}", call, model


def pair_shape(sr):
    """(frames, L16): frame 0 and the last frame that holds L22 samples, L16 the largest the lim16 rule allows that frame."""
    N22, lim = PR.n_axis(N_FILE, sr, 22050), PR.lim16(N_FILE, sr)
    last = (N22 - L22) // 441
    return [0, last], lim - 320 * last


def cut_pair_calls(eng, sr):
    ctx, dev = eng.ctx, eng.device
    f22, f16 = eng._feed_filter(sr), eng._feed_filter16(sr)
    H22, H16 = reach(f22), reach(f16)
    cap = -(-FRAMES * sr // 50) + 2 + 2 * max(H22, H16)
    frames, L16 = pair_shape(sr)
    Cn, grid_x = len(frames), max(-(-L22 // (441 * FRAMES)), -(-L16 // (320 * FRAMES)))
    for fmt in FORMATS:
        for layout, (_, channel) in LAYOUTS.items():
            x = file_on_device(fmt, layout, sr, dev)
            for ceiling in (None, ceiling_of(fmt)):
                def call(x=x, channel=channel, ceiling=ceiling):
                    if ceiling is None:
                        return ctx.cut_pair(x, sr, frames, L22, L16, f22, f16, channel=channel)
                    return ctx.cut_pair_valid(x, sr, frames, L22, L16, f22, f16, ceiling, channel=channel)
                o22, o16 = float(Cn * L22), float(Cn * L16)
                model = {family("cut_rate", layout, ceiling): (1, o22 * 8.0 * H22 + o16 * 8.0 * H16,
                                                               (o22 + o16) * 4.0 + float(grid_x) * Cn * cap * ESZ[fmt])}
                yield f"cut_pair/{sr}/{fmt}/{layout}/{'ceiling' if ceiling else 'plain'}", call, model


def cut_clips_calls(eng):
    """The fp32 (n,) file of 48 kHz; the view starts one element past a 16-byte boundary, so start 3 is an aligned source row and start 0
    is not; L is odd, so the second destination row is unaligned as well."""
    ctx, dev = eng.ctx, eng.device
    x = file_on_device("f32", "mono", 48000, dev)
    starts = [3, 0]
    assert (x.data_ptr() + 4 * starts[0]) % 16 == 0 and (x.data_ptr() + 4 * starts[1]) % 16 != 0 and max(starts) + L_CLIPS <= N_FILE
    for ceiling in (None, ceiling_of("f32")):
        def call(ceiling=ceiling):
            if ceiling is None:
                return (ctx.cut_clips(x, starts, L_CLIPS),)
            return (ctx.cut_clips_valid(x, starts, L_CLIPS, ceiling),)
        yield f"cut_clips/{'ceiling' if ceiling else 'plain'}", call, {"cut_clips": (1, 0.0, 8.0 * len(starts) * L_CLIPS)}


def rate_table(sr, H):
    """One region whose cross-fade crosses a chunk seam, as tests/test_gpu_rate.py builds its table from gaps: -> (spans, windows, chunks,
    Lrow, N22)."""
    P, Q = G.rate_ratio(sr)
    s, l = REGION
    N22 = -(-N_FILE * P // Q)
    ra, rb = G.file_regions([(s, l)], [N_FILE], FADE)[0]
    ws = max(ra * P // Q - H - 3, 0)
    wl = (rb - 1) * P // Q + 1 + H + 5 - ws
    assert (ra, rb) == (s - FADE, s + l + FADE) and ws + wl <= N22
    chunks = G.region_chunks([(ra, rb)])
    assert [c for c, _, _ in chunks] == [0, 1]
    return [(s, l, 0, N_FILE)], [(0, ws, wl, N22)], chunks, wl + 3, N22


def patch_rate_calls(eng, sr):
    ctx, dev = eng.ctx, eng.device
    filt = eng._rate_filter(sr)
    P, Q = G.rate_ratio(sr)
    H = reach(filt)
    row_cap = (CHUNK - 1) * P // Q + 2 + 2 * H
    spans, windows, chunks, lrow, _ = rate_table(sr, H)
    table = native.RateTable(spans, windows, chunks, 1, FADE, dev)
    gen = ((torch.rand(1, lrow, generator=torch.Generator().manual_seed(sr)) * 2 - 1) * 0.3).to(dev)
    gain = torch.tensor([0.8], dtype=torch.float32, device=dev)
    for fmt in FORMATS:
        for layout, (_, channel) in LAYOUTS.items():
            orig = file_on_device(fmt, layout, sr, dev)
            def call(orig=orig, channel=channel):
                out = orig.clone()
                ctx.patch_rate(orig, sr, table, gen, filt, out, gain, channel=channel)
                return (out,)
            model = {family("patch_rate", layout, None): (1, float(len(chunks)) * CHUNK * 8.0 * H,
                                                          float(len(chunks)) * (CHUNK * 2.0 * ESZ[fmt] + 4.0 * row_cap))}
            yield f"patch_rate/{sr}/{fmt}/{layout}", call, model


def groups():
    """{group name: eng -> generator of (key, call, model)}: the parametrisation of the test, the sections of the fixture."""
    g = {"cut_clips": cut_clips_calls}
    for sr in RATES:
        g[f"cut_rate/{sr}"] = lambda eng, sr=sr: cut_rate_calls(eng, sr)
        g[f"cut_pair/{sr}"] = lambda eng, sr=sr: cut_pair_calls(eng, sr)
        g[f"patch_rate/{sr}"] = lambda eng, sr=sr: patch_rate_calls(eng, sr)
    return g


def profiled(ctx, call):
    """call() -> (its result, {family: (launches, flops, bytes)} of the families that launched)."""
    ctx.profile_start(100)
    try:
        out = call()
    finally:
        prof = {q["name"]: (q["launches"], q["flops"], q["bytes"]) for q in ctx.profile_stop() if q["launches"] > 0}
    return out, prof


def engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from tests.harness import build_engine
    return build_engine(HubertArch.tiny(), VocoderArch.tiny(), 100, key=("test_gpu_feed_launches",))
